"""The batched mask term (csrc/mbox_loss.hip and csrc/lincomb_backward.hip behind layers.lincomb_mask_loss and the ops.mbox_* entries) and the criterion module
layers.MultiBoxLoss on the MI355X, held to the fp64 restatement of tests/mbox_loss_restate.py (which tests/test_mbox_loss_cpu.py pins to the
reference's own run) with its derived bounds, to bit-level contracts against the kernels the project already has, and term by term to the
reference's golden forward (tests/golden/mbox_loss_cases.npz).

Bounds: M given the rows' BCE sums -- mask_alpha * sum_r w_r (8 + n_b) eps |term_r| + 2 eps |M|; M from the inputs adds the mask kernels'
1e-5 * sum|terms| + 1e-7 per row; grad mask_coeff and grad proto 1e-5 * sum|terms| + 1e-7; the other terms keep the bounds of their own
restatements; the shift losses and the stand-in's parameter gradients the end-to-end tolerance of tests/test_gpu_t2s_loss.py, 8 x the stored
fp32 deviation of the reference.  Every test prints its observed fraction (run with -s).

Observed on the MI355X (largest fraction of each bound over the cases; the reference's own fp32 on the CPU in brackets): M given the rows 0.05
(0.10), the BCE rows 0.01 (0.01), M from the inputs 0.01 (0.01), grad mask_coeff 0.02 (0.02), grad proto 0.03 (0.03), the row kernel's grad_proto
against the single-set kernel 0.07, the reduction's adjoint grad_bce 0.49; the module: BIoU 0.02 (0.02), C 0.01 (0.01), center 0.02 (0.03), T 0.04 (0.08), B_shift 0.05 and M_shift
0.12 of the end-to-end tolerance, gradients loc 0.05 (0.05), centerness 0.17 (0.27), conf 0.25 (0.11), track 0.07 (0.09), the stand-in's
parameters 0.11 of the end-to-end tolerance; at the constructed case above 256 tiles (mbox_loss_restate.CONSTRUCTED) C 0.04, B_shift 0.11,
gradients loc 0.06, centerness 0.27, conf 0.42, the stand-in's parameters 0.36, the others no larger.  The per-case figures are in
INTEGRATION.md section 14."""
import functools
import os

import numpy as np
import pytest
import torch

import conf_loss_restate as CR
import layer_grad_restate as LR
import mask_loss_restate as ML
import mbox_loss_restate as R
import oracle
import pos_loss_restate as PR
import t2s_loss_restate as T2S
from stmask_amd import layers, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mbox_loss_cases.npz"))
NAMES = list(R.GOLDEN)
E2E_LOSS = 8 * max(R.scalar(GOLD[f"{n}__e2e_loss"]) for n in NAMES)
E2E_GRAD = 8 * max(R.scalar(GOLD[f"{n}__e2e_grad"]) for n in NAMES)


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    """(inputs of lincomb_mask_loss on the CPU, the fp64 composition of M with g = 1): drawn once, shared, never modified."""
    if name in R.GOLDEN or name in R.CONSTRUCTED:
        spec = R.spec_of(name)
        case = R.draw_case(spec, spec["seed"] if name in R.CONSTRUCTED else int(R.scalar(GOLD[f"{name}__seed"])))
        case["masks"] = sum(case["gt_masks"], [])
    else:
        case = R.functional_case(name)
        case["masks"] = case["gt_masks"]
    comp = R.compose(case["loc"], case["mask_coeff"], case["proto"], case["priors"], case["conf_t"], case["idx_t"], case["masks"], oracle.decode,
                     R.MASK_ALPHA, 1.0)
    return case, comp


def mask_args(name, grad=True):
    case, _ = cpu_case(name)
    coeff, proto = case["mask_coeff"].to(DEV), case["proto"].to(DEV)
    if grad:
        coeff.requires_grad_(), proto.requires_grad_()
    return [case["loc"].to(DEV), coeff, proto, case["priors"].to(DEV), case["conf_t"].to(DEV), case["idx_t"].to(DEV),
            [m.to(DEV) for m in case["masks"]]]


def run_mask_loss(name, max_pos=None, sync_error=False, g=1.0):
    a = mask_args(name)
    old = torch.cuda.get_sync_debug_mode()
    if sync_error:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        loss, status = layers.lincomb_mask_loss(*a, mask_alpha=R.MASK_ALPHA, max_pos=max_pos, want_status=True)
        (loss * g).backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    return loss.detach(), status, a[1].grad, a[2].grad


def sync_messages(fn):
    """The warnings of torch's sync debug mode for one call: one per synchronising operation.  The mode's own notice that it is a prototype
    feature (raised once per process when the mode is first set; it also speaks of synchronising) is not one of them."""
    import warnings
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    return [str(w.message) for w in seen if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message)]


def stage_rows(name, n_rows, max_rows=None):
    """The stages one by one through the ops bindings: (rows of the gather, pred, bce, prefix)."""
    a = mask_args(name, grad=False)
    case, _ = cpu_case(name)
    counts = [int(m.shape[0]) for m in case["masks"]]
    H, W = case["masks"][0].shape[1:]
    prefix, state = ops.mbox_positives(a[4], max_rows=max_rows)
    rows = ops.mbox_gather(state, n_rows, a[0], a[3], a[1], a[5], ops.match_offsets(counts, torch.device(DEV)), sum(counts), H, W)
    pred = ops.lincomb_sigmoid_crop(a[2], rows["coeff"], rows["box"], apply_tanh=True, n_dev=rows["n_dev"], row_proto=rows["img"])
    bce = ops.mask_bce_upsampled(pred, torch.cat(a[6]), rows["idx"])
    return rows, pred, bce, prefix, a


# ------------------------------------------------------------------------------------------ the gather, bit for bit
@pytest.mark.parametrize("name", NAMES + ["gap"])
def test_gather_rows_bit_level(name):
    case, comp = cpu_case(name)
    n = comp["n"]
    B, P = case["conf_t"].shape
    H, W = case["masks"][0].shape[1:]
    rows_d = comp["rows"].to(DEV)
    for n_rows in (n, n + 5):
        g, pred, bce, prefix, a = stage_rows(name, n_rows, max_rows=n_rows)
        assert int(g["n_dev"]) == n and int(g["status"]) == 0
        assert prefix.cpu().tolist() == [0] + torch.cumsum(comp["n_b"], 0).tolist()
        # box_r: the torch expression of :559-563 on ops.decode's output
        want_box = R.crop_box_f32(ops.decode(a[0].reshape(-1, 4)[rows_d].contiguous(), a[3][rows_d % P].contiguous()))
        assert torch.equal(g["box"][:n], want_box) and torch.equal(want_box.cpu(), comp["box"])
        assert torch.equal(g["coeff"][:n], a[1].reshape(B * P, -1)[rows_d])
        assert torch.equal(g["img"][:n].cpu(), comp["img"].int()) and torch.equal(g["idx"][:n].cpu(), comp["idx"])
        w32 = comp["w"].float().to(DEV)
        bw = torch.clamp((want_box[:, 2] - want_box[:, 0]) * W, min=1)
        bh = torch.clamp((want_box[:, 3] - want_box[:, 1]) * H, min=1)
        assert torch.equal(g["scale"][:n], w32 / bw / bh)
        if n_rows > n:                                                                    # the padding rows
            assert torch.equal(g["box"][n:].cpu(), torch.tensor([[0.0, 0.0, 1.0, 1.0]]).expand(5, 4))
            assert not g["coeff"][n:].any() and not g["scale"][n:].any() and not g["idx"][n:].any() and not g["img"][n:].any()
            assert not pred[n:].any()
        # bce_r: the rows lincomb_mask_loss_image forms image by image (generate_mask, then mask_bce_sum)
        offs = np.cumsum([0] + [int(m.shape[0]) for m in case["masks"]])
        for b in sorted(set(comp["img"].tolist())):
            sel = torch.nonzero(comp["img"] == b).reshape(-1).to(DEV)
            local = g["idx"][sel] - int(offs[b])
            per_image = layers.mask_bce_sum(layers.generate_mask(a[2][b], g["coeff"][sel], g["box"][sel]), a[6][b], local)
            assert torch.equal(bce[sel], per_image), (name, b)
    g, _, _, _, _ = stage_rows(name, n - 1, max_rows=n - 1)                              # more positives than rows: said, not faulted
    assert int(g["n_dev"]) == n - 1 and int(g["status"]) == 1


# ------------------------------------------------------------------------------------------ the positive list past 256 tiles and 256 images
@pytest.mark.parametrize("name", list(PR.LIST_CASES))
def test_positive_list_beyond_256_tiles_and_images(name):
    """ops.mbox_positives at the list cases of pos_loss_restate (the scanning workgroup's threads own 2 or 4 tiles and carry the count across
    them; images begin inside a thread's chunk; more than 256 images), through public outputs only.  mask_data holds every prior's own
    flattened row (exact in fp32), so the gathered coefficient rows name the list's priors in its order; with masks of 1 x 1 the box is at most
    one pixel wide and high and the gather's scale is the row's weight itself; the scatter gets row r's number r + 1 and puts it at its prior.
    Everything here is exact."""
    B, P, _ = PR.list_positives(name)
    conf_t = PR.list_targets(name)
    want_rows = np.nonzero(conf_t.reshape(-1).numpy() > 0)[0]
    counts = (conf_t > 0).sum(1).numpy()
    n, M = int(want_rows.size), 8
    assert B * P < 1 << 24 and n >= 20
    dev = torch.device(DEV)
    t = conf_t.to(dev)
    mask_data = torch.arange(B * P, dtype=torch.float32, device=dev).view(B, P, 1).expand(B, P, M).contiguous()
    loc = torch.zeros(B, P, 4, device=dev)
    priors = torch.tensor([0.5, 0.5, 0.25, 0.25], device=dev).expand(P, 4).contiguous()
    idx_t = torch.zeros(B, P, dtype=torch.int64, device=dev)
    offs = ops.match_offsets([1] * B, dev)
    w_img = (1.0 / np.maximum(counts, 1).astype(np.float64)).astype(np.float32)
    pos = (conf_t.reshape(-1) > 0)
    for max_rows, status in ((n - 1, 1), (n, 0), (n + 1, 0)):
        prefix, state = ops.mbox_positives(t, max_rows=max_rows)
        assert prefix.dtype == torch.int32 and prefix.cpu().tolist() == [0] + np.cumsum(counts).tolist()
        g = ops.mbox_gather(state, max_rows, loc, priors, mask_data, idx_t, offs, B, 1, 1)
        live = min(n, max_rows)
        assert int(g["n_dev"]) == live and int(g["status"]) == status
        coeff = g["coeff"].cpu()
        assert bool((coeff == coeff[:, :1]).all())
        assert np.array_equal(coeff[:live, 0].numpy().astype(np.int64), want_rows[:live])              # the list: np.nonzero's rows, in order
        assert np.array_equal(g["img"][:live].cpu().numpy(), (want_rows[:live] // P).astype(np.int32))
        assert np.array_equal(g["idx"][:live].cpu().numpy(), want_rows[:live] // P)                    # one mask per image: the image's own
        assert np.array_equal(g["scale"][:live].cpu().numpy().view(np.uint32), w_img[want_rows[:live] // P].view(np.uint32))
        if max_rows > n:                                                                               # the padding row
            assert not coeff[n:].any() and not g["scale"][n:].any() and not g["idx"][n:].any() and not g["img"][n:].any()
            assert torch.equal(g["box"][n:].cpu(), torch.tensor([[0.0, 0.0, 1.0, 1.0]]))
        grad_rows = torch.arange(1, max_rows + 1, dtype=torch.float32, device=dev).view(-1, 1).expand(-1, M).contiguous()
        grad = ops.mbox_scatter_coeff(grad_rows, t, state, g["n_dev"], g["status"]).cpu().view(B * P, M)
        assert not grad[~pos].any()                                                                    # exact zeros at every other prior
        if status == 0:
            want = torch.arange(1, n + 1, dtype=torch.float32).view(-1, 1).expand(-1, M)
            assert torch.equal(grad[pos], want)                                                        # row r back at its prior
        else:                                                                                          # more positives than rows: said, not faulted
            assert bool(torch.isnan(grad[pos]).all())


# ------------------------------------------------------------------------------------------ the loss and its gradients, both forms
@pytest.mark.parametrize("name", NAMES + ["gap"])
def test_mask_loss_within_the_bounds_both_forms(name):
    case, comp = cpu_case(name)
    n = comp["n"]
    H, W = case["masks"][0].shape[1:]
    loss, status, gc, gp = run_mask_loss(name)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and int(status) == 0
    rows, _, bce, _, _ = stage_rows(name, n)
    red = R.restate_reduce(bce.cpu(), rows["box"].cpu(), comp["w"], comp["n_b"][comp["img"]], H, W, R.MASK_ALPHA)
    f_red = abs(float(loss) - float(red["M"])) / float(red["M_bound"])                  # the reduction given the card's own rows
    f_bce = ML.worst_ratio(bce, comp["bce"], comp["bce_mag"])
    f_in = abs(float(loss) - float(comp["M"])) / float(comp["M_bound"])                  # from the inputs
    rc = LR.worst_ratio(gc, comp["grad_coeff"], comp["grad_coeff_mag"])
    rp = LR.worst_ratio(gp, comp["grad_proto"], comp["grad_proto_mag"])
    print(f"\n{name} max_pos=None: M {float(loss):.6f}: reduction {f_red:.3f}, bce rows {f_bce:.3f}, from the inputs {f_in:.3f} of the bounds; "
          f"grad mask_coeff {rc:.3f}, grad proto {rp:.3f} of 1e-5 * sum|terms| + 1e-7")
    assert max(f_red, f_bce, f_in, rc, rp) <= 1.0
    # exact zeros: rows of grad mask_data that are not positive, images without positives in grad proto
    pos = (case["conf_t"] > 0).to(DEV)
    assert not gc[~pos].any() and bool(gc[pos].abs().sum() > 0)
    for b in range(case["conf_t"].shape[0]):
        assert bool(gp[b].any()) == bool(comp["n_b"][b] > 0), b
    loss2, _, gc2, gp2 = run_mask_loss(name)                                             # bit-identical from run to run
    assert torch.equal(loss, loss2) and torch.equal(gc, gc2) and torch.equal(gp, gp2)
    for K in (n, 2 * n):                                                                  # the padded form: the same bits, no host synchronisation
        lk, sk, gck, gpk = run_mask_loss(name, K, sync_error=True)
        assert int(sk) == 0 and torch.equal(lk, loss) and torch.equal(gck, gc) and torch.equal(gpk, gp), K
    lo, so, gco, gpo = run_mask_loss(name, n - 1)                                         # overflow: NaN and the status word, never a fault
    assert int(so) == 1 and bool(torch.isnan(lo)) and bool(torch.isnan(gco[pos]).all()) and not gco[~pos].any() and bool(torch.isnan(gpo).all())


def test_mask_loss_without_grad_equals_the_autograd_path():
    a = mask_args("tiny", grad=False)
    plain = layers.lincomb_mask_loss(*a, mask_alpha=R.MASK_ALPHA)
    loss, _, _, _ = run_mask_loss("tiny")
    assert plain.grad_fn is None and torch.equal(plain, loss)
    with pytest.raises(RuntimeError, match="double backward"):
        b = mask_args("tiny")
        (gg,) = torch.autograd.grad(layers.lincomb_mask_loss(*b), b[2], create_graph=True)
        gg.sum().backward()


@pytest.mark.parametrize("max_pos", [None, 6])
def test_batch_without_positives_is_exactly_zero(max_pos):
    _, comp = cpu_case("none")
    assert comp["n"] == 0
    loss, status, gc, gp = run_mask_loss("none", max_pos, sync_error=max_pos is not None)
    assert float(loss) == 0.0 and int(status) == 0 and loss.dim() == 0
    assert gc is not None and gp is not None and not gc.any() and not gp.any()           # the backward ran and yielded zeros


# ------------------------------------------------------------------------------------------ the row kernel's prototype gradient
@functools.lru_cache(maxsize=None)
def proto_rows_case(M, sizes=(40, 0, 30), h=20, w=30):
    """600 pixels: three pixel blocks, the last partial (8 row splits at three sets); a set of 40 rows (three 16-row chunks, the last partial),
    one without rows, one of 30; boxes of every kind (layer_grad_restate.mask_boxes).  128 x 176 pixels: 88 pixel blocks x 3 sets, more than
    256 workgroups, so the rows are not split and the kernel writes grad_proto itself."""
    g = torch.Generator().manual_seed(1900 + M)
    n = sum(sizes)
    proto = torch.relu(torch.randn(len(sizes), h, w, M, generator=g))
    coeff, boxes, go = torch.randn(n, M, generator=g), LR.mask_boxes(n, h, w, g), torch.randn(n, h, w, generator=g)
    prefix = torch.tensor(np.cumsum((0,) + sizes), dtype=torch.int32)
    refs = []
    for s in range(len(sizes)):
        sl = slice(int(prefix[s]), int(prefix[s + 1]))
        refs.append(LR.mask_reference(proto[s], coeff[sl], boxes[sl], go[sl]) if sizes[s] else None)
    return proto, coeff, boxes, go, prefix, refs


@pytest.mark.parametrize("M,sizes,hw", [(8, (40, 0, 30), (20, 30)), (32, (40, 0, 30), (20, 30)), (64, (40, 0, 30), (20, 30)),
                                        (8, (6, 0, 5), (128, 176))])
def test_rows_proto_backward_against_the_single_set_kernel(M, sizes, hw):
    proto, coeff, boxes, go, prefix, refs = proto_rows_case(M, sizes, *hw)
    p, c, b, g, pf = proto.to(DEV), coeff.to(DEV), boxes.to(DEV), go.to(DEV), prefix.to(DEV)
    gp = ops.lincomb_rows_proto_backward(g, p, c, b, pf)
    assert torch.equal(gp, ops.lincomb_rows_proto_backward(g, p, c, b, pf))              # fixed-order sums
    worst = 0.0
    for s, ref in enumerate(refs):
        if ref is None:
            assert not gp[s].any()                                                        # a set without rows: exact zeros
            continue
        sl = slice(int(prefix[s]), int(prefix[s + 1]))
        (gp64, _), (mag, _) = ref
        single, _ = ops.lincomb_sigmoid_crop_backward(g[sl], p[s], c[sl], b[sl], need_coeff=False)     # stm_lincomb_backward_f32, set by set
        worst = max(worst, LR.worst_ratio(gp[s], gp64, mag), LR.worst_ratio(gp[s], single.cpu().double(), mag))
        if hw == (128, 176):
            # 88 pixel blocks x 3 sets: no row splits here, one 16-row chunk and so no splits in the single-set kernel either; both add the
            # rows in row order through the one fmaf chain of csrc/lincomb_backward.hip: the same bits
            assert torch.equal(gp[s], single), s
    print(f"\nM={M} {hw[0]}x{hw[1]}: grad_proto of the row kernel, worst |g - g64| and |g - single-set kernel| / (1e-5 * sum|terms| + 1e-7) = {worst:.3f}")
    assert worst <= 1.0
    # a prefix that lies (rows past n, a negative start): clamped, never read outside
    odd = torch.tensor([-5, sizes[0], sizes[0], 10 ** 6], dtype=torch.int32, device=DEV)
    got = ops.lincomb_rows_proto_backward(g, p, c, b, odd)
    assert torch.equal(got[0], gp[0]) and not got[1].any() and torch.equal(got[2], gp[2])
    nan = ops.lincomb_rows_proto_backward(g, p, c, b, pf, torch.ones(1, dtype=torch.int32, device=DEV))
    assert bool(torch.isnan(nan).all())


# ------------------------------------------------------------------------------------------ the module, term by term
@functools.lru_cache(maxsize=None)
def restated_terms(name):
    case, _ = cpu_case(name)
    B = case["conf_t"].shape[0]
    inv = 1.0 / B
    comp = R.compose(case["loc"], case["mask_coeff"], case["proto"], case["priors"], case["conf_t"], case["idx_t"], case["masks"], oracle.decode,
                     R.MASK_ALPHA, inv)
    bx = PR.restate_box(case["loc"], case["priors"], case["gt_boxes_t"], case["conf_t"], case["centerness"], R.ALPHAS["bboxiou_alpha"],
                        R.ALPHAS["center_alpha"], inv, inv)
    cf = CR.restate(case["conf"], case["conf_t"], R.RATIO, R.ALPHAS["conf_alpha"], "reference", inv)
    tr = PR.restate_track(case["track"], case["conf_t"], case["ids_t"], R.ALPHAS["track_alpha"], 1.0)
    t2s = T2S.compose(R.t2s_case(case), R.stand_in_net(R.spec_of(name)["M"], double=True).TemporalNet, oracle.decode, R.ALPHAS["boxshift_alpha"],
                      R.ALPHAS["maskshift_alpha"])
    return comp, bx, cf, tr, t2s


def run_module(name, max_pos=None, sync_error=False, per_image_priors=False, sync_warn=None):
    """sync_warn: a list that receives the messages of torch's sync debug mode ("warn") for this forward + backward."""
    case, _ = cpu_case(name)
    pred = R.predictions(case, DEV, grad=True)
    if per_image_priors:                                                                  # [B,P,4]: what DataParallel hands the reference's criterion
        pred["priors"] = pred["priors"].expand(case["conf_t"].shape[0], -1, 4).contiguous()
    net = R.stand_in_net(R.spec_of(name)["M"], DEV)
    crit = layers.MultiBoxLoss(R.NUM_CLASSES, R.POS_T, R.NEG_T, R.RATIO, max_pos=max_pos)
    gt = R.ground_truth(case, DEV)
    old = torch.cuda.get_sync_debug_mode()
    if sync_error:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        if sync_warn is None:
            losses = crit(net, pred, *gt)
            sum(losses.values()).backward()
        else:
            sync_warn.extend(sync_messages(lambda: sum(crit(net, pred, *gt).values()).backward()))
            losses = {}
    finally:
        torch.cuda.set_sync_debug_mode(old)
    return {k: v.detach() for k, v in losses.items()}, pred, net, gt


@pytest.mark.parametrize("name", NAMES + list(R.CONSTRUCTED))
def test_module_terms_against_the_stand_alone_calls_and_the_golden_forward(name):
    case, _ = cpu_case(name)
    B, P = case["conf_t"].shape
    losses, pred, net, gt = run_module(name)
    assert sorted(losses) == sorted(["BIoU", "M", "C", "center", "B_shift", "M_shift", "T"])
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in losses.values())
    # ---- every term is the stand-alone layers.* call on the same inputs, times the same division
    with torch.no_grad():
        d = {k: v.detach() for k, v in pred.items()}
        pri = d["priors"][0]
        _, conf_t, idx_t, ids_t, gt_boxes_t = layers.match_batch(R.POS_T, R.NEG_T, sum(gt[0], []), sum(gt[1], []), sum(gt[3], []), pri, d["conf"])
        for k, t in (("conf_t", conf_t), ("idx_t", idx_t), ("ids_t", ids_t)):
            assert torch.equal(t.cpu(), case[k]), k                                      # ... which are the reference's targets
        biou, center = layers.box_center_loss(d["loc"], pri, gt_boxes_t, conf_t, d["centerness"], 5.0, 20.0)
        assert torch.equal(losses["BIoU"], biou / B) and torch.equal(losses["center"], center / B)
        assert torch.equal(losses["C"], layers.ohem_conf_loss(d["conf"], conf_t, R.RATIO, 6.125, weights="reference") / B)
        assert torch.equal(losses["T"], layers.track_loss(d["track"], conf_t, ids_t, 5.0))
        assert torch.equal(losses["M"], layers.lincomb_mask_loss(d["loc"], d["mask_coeff"], d["proto"], pri, conf_t, idx_t, sum(gt[2], []), 6.125) / B)
        shift = layers.track_to_segment_loss(net.TemporalNet, d["T2S_concat_feat"], d["loc"][::2], ids_t[::2], d["mask_coeff"][::2], d["proto"][1::2],
                                             pri, gt[0], gt[3], gt[2], boxshift_alpha=5.0, maskshift_alpha=6.125)
        assert torch.equal(losses["B_shift"], shift["B_shift"]) and torch.equal(losses["M_shift"], shift["M_shift"])
    # ---- every term within its bound of the restatement, which holds the reference's golden forward (test_mbox_loss_cpu.py)
    comp, bx, cf, tr, t2s = restated_terms(name)
    inv, e = 1.0 / B, R.EPS
    val = {k: float(v) for k, v in losses.items()}
    fr = dict(M=abs(val["M"] - float(comp["M"]) * inv) / float(comp["M_bound"] * inv + e * comp["M"].abs() * inv),
              BIoU=abs(val["BIoU"] - float(bx["biou"]) * inv) / float(bx["biou_bound"] * inv + e * bx["biou"].abs() * inv),
              center=abs(val["center"] - float(bx["center"]) * inv) / float(bx["center_bound"] * inv + e * bx["center"].abs() * inv),
              C=abs(val["C"] - float(cf["loss"]) * inv) / float(cf["loss_bound"] * inv + e * cf["loss"].abs() * inv),
              T=abs(val["T"] - float(tr["loss"])) / float(tr["loss_bound"]),
              B_shift=abs(val["B_shift"] - float(t2s["B"])) / abs(float(t2s["B"])) / E2E_LOSS,
              M_shift=abs(val["M_shift"] - float(t2s["M"])) / abs(float(t2s["M"])) / E2E_LOSS)
    if name in R.GOLDEN:
        gold = {k: R.scalar(GOLD[f"{name}__loss_{k}"]) for k in val}
        print(f"\n{name}: " + ", ".join(f"{k} {val[k]:.5f} (reference {gold[k]:.5f}) at {fr[k]:.3f}" for k in val) + " of the bounds")
    else:                                                                                 # a constructed case: no run of the reference to show
        print(f"\n{name}: " + ", ".join(f"{k} {val[k]:.5f} at {fr[k]:.3f}" for k in val) + " of the bounds")
    assert max(fr.values()) <= 1.0
    # ---- gradients of the sum of all terms
    pos = bx["pos"]
    g = {k: pred[k].grad.detach().cpu().double() for k in ("loc", "conf", "mask_coeff", "proto", "centerness", "track")}
    gconf = g["conf"].view(-1, R.NUM_CLASSES)
    fg = dict(loc=float(((g["loc"].view(-1, 4) - bx["grad_loc"]).abs()[pos] / bx["grad_loc_bound"][pos]).max()),
              centerness=float(((g["centerness"].view(-1) - bx["grad_cent"]).abs()[pos] / bx["grad_cent_bound"][pos]).max()),
              conf=float(((gconf - cf["grad"]).abs().max(1).values[cf["keep"]] / cf["grad_bound"][cf["keep"]]).max()),
              track=float(((g["track"].view(-1, R.EMBED) - tr["grad"]).abs()[tr["pos"]] / tr["grad_bound"][tr["pos"]]).max()),
              mask_coeff=LR.worst_ratio(g["mask_coeff"], comp["grad_coeff"], comp["grad_coeff_mag"]),
              proto=LR.worst_ratio(g["proto"], comp["grad_proto"], comp["grad_proto_mag"]),
              net=max(float((p.grad.cpu().double() - t2s["grads"][k]).abs().max() / t2s["grads"][k].abs().max())
                      for k, p in net.TemporalNet.named_parameters()) / E2E_GRAD)
    print(f"{name}: gradients " + ", ".join(f"{k} {v:.3f}" for k, v in fg.items()) + " of the bounds")
    assert max(fg.values()) <= 1.0
    assert not g["loc"].view(-1, 4)[~pos].any() and not gconf[~cf["keep"]].any() and not g["mask_coeff"].view(B * P, -1)[~pos].any()


def test_module_with_max_pos_makes_no_host_synchronisation():
    ref, pred0, _, _ = run_module("tiny")
    run_module("tiny", 64)                                                                # (warm-up: MIOpen picks its kernels for this batch size)
    losses, pred, _, _ = run_module("tiny", 64, sync_error=True)                          # forward and backward
    for k in ("BIoU", "M", "C", "center", "T", "B_shift", "M_shift"):
        assert torch.equal(losses[k], ref[k]), k                                          # and the same bits as the exact form
    assert torch.equal(pred["mask_coeff"].grad, pred0["mask_coeff"].grad) and torch.equal(pred["proto"].grad, pred0["proto"].grad)


@pytest.mark.parametrize("name", list(R.CONSTRUCTED))
def test_module_past_256_tiles_agrees_in_both_forms_without_host_synchronisation(name):
    """The constructed batch above both lines of the scans (270 OHEM tiles, 270 list tiles, images that begin inside a scan thread's chunk):
    max_pos=None and max_pos=K give the same bits, and at max_pos=K forward and backward make no host synchronisation."""
    _, comp = cpu_case(name)
    K = comp["n"] + 9
    ref, pred0, _, _ = run_module(name)
    run_module(name, K)                                                                   # (warm-up: MIOpen picks its kernels for this batch size)
    losses, pred, _, _ = run_module(name, K, sync_error=True)
    for k in ("BIoU", "M", "C", "center", "T", "B_shift", "M_shift"):
        assert torch.equal(losses[k], ref[k]), k
    assert torch.equal(pred["mask_coeff"].grad, pred0["mask_coeff"].grad) and torch.equal(pred["proto"].grad, pred0["proto"].grad)


def test_exact_form_makes_one_host_read_per_row_list():
    """max_pos=None after a warm-up: lincomb_mask_loss reads its [B+1] prefix once; the module reads that and the shift loss's prefix: 2."""
    run_mask_loss("tiny")
    a = mask_args("tiny")
    seen = sync_messages(lambda: layers.lincomb_mask_loss(*a, mask_alpha=R.MASK_ALPHA).backward())
    print(f"\nlincomb_mask_loss max_pos=None: {len(seen)} host synchronisation(s): {seen}")
    assert len(seen) == 1
    run_module("tiny")
    seen = []
    run_module("tiny", sync_warn=seen)
    print(f"MultiBoxLoss max_pos=None: {len(seen)} host synchronisation(s): {seen}")
    assert len(seen) == 2
    seen = []
    run_module("tiny", 64, sync_warn=seen)
    assert seen == []


@pytest.mark.parametrize("name", ["tiny", "blocks"])
def test_per_image_priors_give_the_same_bits(name):
    """priors [B,P,4] (the gather's priors_per_image branch, every image holding the same priors) against priors [P,4]."""
    case, comp = cpu_case(name)
    B, n = case["conf_t"].shape[0], comp["n"]
    H, W = case["masks"][0].shape[1:]
    g0, _, _, _, a = stage_rows(name, n + 3)
    counts = [int(m.shape[0]) for m in case["masks"]]
    _, state = ops.mbox_positives(a[4])
    pri_b = a[3][None].expand(B, -1, 4).contiguous()
    g1 = ops.mbox_gather(state, n + 3, a[0], pri_b, a[1], a[5], ops.match_offsets(counts, torch.device(DEV)), sum(counts), H, W)
    assert all(torch.equal(g0[k], g1[k]) for k in g0), [k for k in g0 if not torch.equal(g0[k], g1[k])]
    # ... with different priors per image, image b reads ITS priors: rows of image b equal the [P,4] gather with priors[b]
    shifted = torch.stack([a[3] * (1.0 + 0.03125 * b) for b in range(B)]).contiguous()
    gs = ops.mbox_gather(state, n, a[0], shifted, a[1], a[5], ops.match_offsets(counts, torch.device(DEV)), sum(counts), H, W)
    for b in sorted(set(comp["img"].tolist())):
        sel = torch.nonzero(comp["img"] == b).reshape(-1).to(DEV)
        gb = ops.mbox_gather(state, n, a[0], shifted[b].contiguous(), a[1], a[5], ops.match_offsets(counts, torch.device(DEV)), sum(counts), H, W)
        assert torch.equal(gs["box"][sel], gb["box"][sel]) and torch.equal(gs["scale"][sel], gb["scale"][sel]), b
    l0, _, gc0, gp0 = run_mask_loss(name)
    b_args = mask_args(name)
    b_args[3] = pri_b
    l1 = layers.lincomb_mask_loss(*b_args, mask_alpha=R.MASK_ALPHA)
    l1.backward()
    assert torch.equal(l1.detach(), l0) and torch.equal(b_args[1].grad, gc0) and torch.equal(b_args[2].grad, gp0)
    ref, pred0, net0, _ = run_module(name)                                                 # the module
    got, pred1, net1, _ = run_module(name, per_image_priors=True)
    assert all(torch.equal(got[k], ref[k]) for k in ref), [k for k in ref if not torch.equal(got[k], ref[k])]
    for k in ("loc", "conf", "mask_coeff", "proto", "centerness", "track"):
        assert torch.equal(pred1[k].grad, pred0[k].grad), k


@pytest.mark.parametrize("name,pad", [("tiny", 0), ("blocks", 7), ("gap", 300)])
def test_reduce_adjoint_within_its_bound(name, pad):
    """stm_mbox_reduce_backward_f32 on its own: grad_bce_r = g * mask_alpha * scale_r, one rounding of the double product besides the 6 eps the
    fp32 scale carries and the one of w_r: 8 eps |grad| (mbox_loss_restate.restate_reduce); exact zeros in the padding; NaN under the status word."""
    case, comp = cpu_case(name)
    n = comp["n"]
    H, W = case["masks"][0].shape[1:]
    rows, _, _, _, _ = stage_rows(name, n + pad)
    r = R.restate_reduce(torch.zeros(n), rows["box"][:n].cpu(), comp["w"], comp["n_b"][comp["img"]], H, W, R.MASK_ALPHA, 0.75)
    g = torch.tensor(0.75, device=DEV)
    got = ops.mbox_reduce_backward(g, rows["scale"], rows["n_dev"], rows["status"], R.MASK_ALPHA)
    frac = float(((got[:n].cpu().double() - r["grad_bce"]).abs() / r["grad_bce_bound"]).max())
    print(f"\n{name} pad={pad}: grad_bce at {frac:.3f} of the bound")
    assert frac <= 1.0 and not got[n:].any() and got.shape == (n + pad,)
    assert torch.equal(got, ops.mbox_reduce_backward(g, rows["scale"], rows["n_dev"], rows["status"], R.MASK_ALPHA))
    over = ops.mbox_reduce_backward(g, rows["scale"], rows["n_dev"], torch.ones(1, dtype=torch.int32, device=DEV), R.MASK_ALPHA)
    assert bool(torch.isnan(over).all())
