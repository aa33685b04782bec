"""The temporal-fusion loss (csrc/t2s_loss.hip and csrc/lincomb_backward.hip behind layers.track_to_segment_loss, layers.generate_mask_rows and the ops.t2s_* entries) on the
MI355X, held to the fp64 restatement of tests/t2s_loss_restate.py (which tests/test_t2s_loss_cpu.py pins to the reference's own run) with its
derived bounds, and end to end -- RoIAlign, the stand-in TemporalNet, the mask, its BCE and the reductions -- to the fp64 composition.

End-to-end tolerance: it cannot be derived (MIOpen and the CPU add the convolution's C * 9 = 108 products in different orders), so it is measured:
the fixture stores the relative deviation of the reference's own fp32 CPU run from the fp64 composition (e2e_loss, e2e_grad), and the GPU is
allowed 8 x the largest over the golden cases -- three bits for the different summation order.  Every test prints its observed fraction.

Observed on the MI355X (largest fraction of each bound over the cases): reg_t columns 2-3 0.76, B_shift 0.04, M_shift 0.08, grad_bbox_reg 0.27,
grad_bce 0.16, grad_coeff 0.05 of its tolerance; end to end 0.07 (losses), 0.06 (parameter gradients), 0.07 (grad concat_feat) of the tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

import layer_grad_restate as LR
import oracle
import t2s_loss_restate as R
from stmask_amd import layers, ops
from stmask_amd._lib import StmError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t2s_loss_cases.npz"))
WITH_ROWS = ["p37", "p256_b2", "p257_b3"]
ALL_SPECS = {**R.GOLDEN, **R.constructed_cases()}


def _s(a):
    return float(np.asarray(a).reshape(-1)[0])


E2E_LOSS = 8 * max(_s(GOLD[f"{n}__e2e_loss"]) for n in WITH_ROWS)
E2E_GRAD = 8 * max(_s(GOLD[f"{n}__e2e_grad"]) for n in WITH_ROWS)


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    """(case on the CPU, its restated targets): drawn once, shared, never modified."""
    spec = ALL_SPECS[name]
    if name in R.GOLDEN:
        seed = int(_s(GOLD[f"{name}__seed"]))
    elif "seed" in spec:
        seed = spec["seed"]
    else:                                                                                 # the constructed cases that carry no seed of their own
        seed = 41000 + sorted(n for n, s in R.constructed_cases().items() if "seed" not in s).index(name)
    case = R.draw_case(spec, seed)
    return case, R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])


@functools.lru_cache(maxsize=None)
def composition(name):
    case, _ = cpu_case(name)
    return R.compose(case, R.StandInNet(R.C_FEAT, ALL_SPECS[name]["M"], R.NET_SEED).double(), oracle.decode, R.ALPHA_B, R.ALPHA_M)


def dev_case(name):
    case, _ = cpu_case(name)
    mv = lambda v: v.to(DEV) if isinstance(v, torch.Tensor) else [[t.to(DEV) for t in pair] for pair in v]     # noqa: E731
    return {k: mv(v) for k, v in case.items()}


def flat_gt(d):
    """What the binding concatenates: boxes, ids, counts of both frames."""
    return (torch.cat([b[0] for b in d["gt_bboxes"]]), torch.cat([i[0] for i in d["gt_ids"]]), [b[0].shape[0] for b in d["gt_bboxes"]],
            torch.cat([b[1] for b in d["gt_bboxes"]]), torch.cat([i[1] for i in d["gt_ids"]]), [b[1].shape[0] for b in d["gt_bboxes"]])


def run_targets(d, max_rows=None):
    br, ir, cr, bn, inx, cn = flat_gt(d)
    return ops.t2s_targets(d["ids_t"], br, ir, cr, bn, inx, cn, max_rows=max_rows)


def loss_call(d, net, max_pos=None, **kw):
    return layers.track_to_segment_loss(net, d["concat_feat"], d["loc_ref"], d["ids_t"], d["mask_coeff_ref"], d["proto_next"], d["priors"],
                                        d["gt_bboxes"], d["gt_ids"], d["gt_masks"], boxshift_alpha=R.ALPHA_B, maskshift_alpha=R.ALPHA_M,
                                        max_pos=max_pos, **kw)


# ------------------------------------------------------------------------------------------ stage 1: targets
@pytest.mark.parametrize("name", list(ALL_SPECS))
def test_targets_exact_contracts(name):
    case, t = cpu_case(name)
    d = dev_case(name)
    pos_t, reg_t, idx_next, prefix, _ = run_targets(d)
    bs, P = case["ids_t"].shape
    assert torch.equal(pos_t.cpu(), t["pos"].long())
    assert torch.equal(idx_next.cpu(), t["k_global"])
    reg = reg_t.cpu()
    assert bool((reg[~t["pos"]] == 0).all())                                             # exact zeros where not positive
    assert torch.equal(reg[..., :2][t["pos"]], t["reg01"][t["pos"]])                      # columns 0-1: IEEE fp32, the reference's operand order
    r64, bound = t["reg"][..., 2:][t["pos"]], t["reg_bound"][..., 2:][t["pos"]]
    got = reg[..., 2:][t["pos"]].double()
    fin = torch.isfinite(r64)
    assert torch.equal(got[~fin], r64[~fin])
    frac = float(((got - r64).abs()[fin] / bound[fin]).max()) if bool(fin.any()) else 0.0
    print(f"\n{name}: reg_t columns 2-3 at {frac:.3f} of the bound")
    assert frac <= 1.0
    n_i = t["pos"].sum(1)
    assert prefix.cpu().tolist() == [0] + torch.cumsum(n_i, 0).tolist()
    if name in R.GOLDEN and int(n_i.sum()):                                               # ... and the reference's own targets
        rows = torch.nonzero(t["pos"].reshape(-1)).reshape(-1)
        assert rows.tolist() == GOLD[f"{name}__pos_rows"].tolist()
        assert torch.equal(reg.reshape(-1, 4)[rows][:, :2], torch.from_numpy(GOLD[f"{name}__ref_reg"])[:, :2])


def test_targets_refuse_from_the_shapes():
    d = dev_case("p37")
    br, ir, cr, bn, inx, cn = flat_gt(d)
    many = torch.rand(129, 4, device=DEV)
    with pytest.raises(StmError, match="limit 128"):
        ops.t2s_targets(d["ids_t"], many, torch.arange(129, device=DEV), [129], bn, inx, cn)
    with pytest.raises(StmError):
        ops.t2s_targets(d["ids_t"][:, :0], br, ir, cr, bn, inx, cn)
    with pytest.raises(NotImplementedError):
        loss_call(d, None, mask_loss=False)
    with pytest.raises(NotImplementedError):
        loss_call(d, None, crop=False)
    bad = [[m[0], m[1][:, :-1]] for m in d["gt_masks"]] + [d["gt_masks"][0]]
    with pytest.raises(ValueError):
        layers.track_to_segment_loss(None, d["concat_feat"].repeat(2, 1, 1, 1), d["loc_ref"].repeat(2, 1, 1), d["ids_t"].repeat(2, 1),
                                     d["mask_coeff_ref"].repeat(2, 1, 1), d["proto_next"].repeat(2, 1, 1, 1), d["priors"], d["gt_bboxes"] * 2,
                                     d["gt_ids"] * 2, bad)


# ------------------------------------------------------------------------------------------ stage 2: gather
@pytest.mark.parametrize("name", WITH_ROWS + ["duplicates", "uneven"])
def test_gather_rows_are_the_dense_tensors_through_the_list(name):
    case, t = cpu_case(name)
    d = dev_case(name)
    bs, P = case["ids_t"].shape
    rows, clip, w, n_i = R.row_weights(t["pos"])
    n = rows.numel()
    fh, fw = case["concat_feat"].shape[2:]
    bn = torch.cat([b[1] for b in d["gt_bboxes"]])
    rows_d = rows.to(DEV)
    for n_rows in (n, n + 3):
        _, reg_t, idx_next, _, state = run_targets(d, max_rows=n_rows)
        g = ops.t2s_gather(state, n_rows, d["loc_ref"], d["priors"], d["mask_coeff_ref"], reg_t, idx_next, bn, fh, fw)
        assert int(g["n_dev"]) == n and int(g["status"]) == 0
        want = ops.shift_rois(ops.decode(d["loc_ref"].reshape(-1, 4)[rows_d].contiguous(), d["priors"][rows_d % P].contiguous()),
                              clip.to(DEV).int(), fh, fw)
        assert torch.equal(g["rois"][:n], want)                                           # bit-identical to the inference path's conversion
        assert torch.equal(g["reg"][:n], reg_t.reshape(-1, 4)[rows_d])
        assert torch.equal(g["coeff"][:n], d["mask_coeff_ref"].reshape(bs * P, -1)[rows_d])
        kg = t["k_global"].reshape(-1)[rows]
        assert torch.equal(g["idx"][:n].cpu(), kg) and torch.equal(g["box"][:n], bn[kg.to(DEV)])
        assert torch.equal(g["clip"][:n].cpu(), clip.int())
        assert torch.equal(g["w"][:n].cpu(), (1.0 / n_i[clip].double()).float())
        if n_rows > n:                                                                    # the padding rows
            assert torch.equal(g["rois"][n:].cpu(), torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0]]).expand(3, 5))
            assert torch.equal(g["box"][n:].cpu(), torch.tensor([[0.0, 0.0, 1.0, 1.0]]).expand(3, 4))
            assert not g["reg"][n:].any() and not g["coeff"][n:].any() and not g["w"][n:].any() and not g["idx"][n:].any() and not g["clip"][n:].any()
    _, reg_t, idx_next, _, state = run_targets(d, max_rows=n - 1)                         # more shift-positives than rows: said, not faulted
    g = ops.t2s_gather(state, n - 1, d["loc_ref"], d["priors"], d["mask_coeff_ref"], reg_t, idx_next, bn, fh, fw)
    assert int(g["n_dev"]) == n - 1 and int(g["status"]) == 1


# ------------------------------------------------------------------------------------------ stage 3: reduce and adjoint
@pytest.mark.parametrize("name,pad", [("p37", 0), ("p257_b3", 3), ("uneven", 0), ("uneven", 300)])
def test_reduce_and_adjoint_within_the_derived_bounds(name, pad):
    case, t = cpu_case(name)
    rows, clip, w, n_i = R.row_weights(t["pos"])
    n, bs = rows.numel(), case["ids_t"].shape[0]
    H, W = ALL_SPECS[name]["HW"]
    reg = t["reg"].reshape(-1, 4)[rows].float()
    box = torch.cat([b[1] for b in case["gt_bboxes"]])[t["k_global"].reshape(-1)[rows]]
    w32 = w.float()
    for seed in range(100):                                                               # synthetic bbox_reg / bce, off smooth-L1's kink
        g = torch.Generator().manual_seed(7000 + seed)
        bbox_reg, bce = reg + 1.5 * torch.randn(n, 4, generator=g), 200 * torch.rand(n, generator=g)
        r = R.restate_losses(bbox_reg, reg, bce, box, w32, n_i[clip], bs, H, W, R.ALPHA_B, R.ALPHA_M, 0.75, 1.25)
        if r["min_kink"] > R.KINK:
            break
    padf = lambda v, fill=0.0: torch.cat([v, torch.full((pad, *v.shape[1:]), fill, dtype=v.dtype)]).to(DEV)      # noqa: E731
    a, tg, bc, wr = padf(bbox_reg, 3.0), padf(reg), padf(bce, 7.0), padf(w32)
    bx = torch.cat([box, torch.tensor([[0.0, 0.0, 1.0, 1.0]]).expand(pad, 4)]).to(DEV)
    n_dev, status = torch.tensor([n], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    B, M = ops.t2s_reduce(a, tg, bc, bx, wr, n_dev, status, bs, H, W, R.ALPHA_B, R.ALPHA_M)
    B2, M2 = ops.t2s_reduce(a, tg, bc, bx, wr, n_dev, status, bs, H, W, R.ALPHA_B, R.ALPHA_M)
    assert torch.equal(B, B2) and torch.equal(M, M2) and B.dim() == 0 and B.dtype == torch.float32
    fb, fm = abs(float(B) - float(r["B"])) / float(r["B_bound"]), abs(float(M) - float(r["M"])) / float(r["M_bound"])
    gb, gm = torch.tensor(0.75, device=DEV), torch.tensor(1.25, device=DEV)
    g_reg, g_bce = ops.t2s_reduce_backward(gb, gm, a, tg, bx, wr, n_dev, status, bs, H, W, R.ALPHA_B, R.ALPHA_M)
    fr = float(((g_reg[:n].cpu().double() - r["grad_reg"]).abs() / r["grad_reg_bound"]).max())
    fc = float(((g_bce[:n].cpu().double() - r["grad_bce"]).abs() / r["grad_bce_bound"]).max())
    print(f"\n{name} pad={pad}: B_shift {fb:.3f}, M_shift {fm:.3f}, grad_bbox_reg {fr:.3f}, grad_bce {fc:.3f} of the bounds")
    assert max(fb, fm, fr, fc) <= 1.0
    assert not g_reg[n:].any() and not g_bce[n:].any()                                    # padding rows: exact zeros
    status.fill_(1)                                                                       # the overflow word: NaN, said, not faulted
    B, M = ops.t2s_reduce(a, tg, bc, bx, wr, n_dev, status, bs, H, W)
    g_reg, g_bce = ops.t2s_reduce_backward(gb, gm, a, tg, bx, wr, n_dev, status, bs, H, W)
    assert bool(torch.isnan(B)) and bool(torch.isnan(M)) and bool(torch.isnan(g_reg).all()) and bool(torch.isnan(g_bce).all())


# ------------------------------------------------------------------------------------------ the row-prototype mask and its gradient
@functools.lru_cache(maxsize=None)
def mask_rows_case(M, S=3, n=33, h=20, w=30):
    """600 pixels: three pixel blocks, the last partial; rows of every box kind (layer_grad_restate.mask_boxes), sorted by prototype set."""
    g = torch.Generator().manual_seed(900 + M)
    proto = torch.relu(torch.randn(S, h, w, M, generator=g))
    coeff = torch.randn(n, M, generator=g)
    boxes = LR.mask_boxes(n, h, w, g)
    row_proto = torch.sort(torch.randint(0, S, (n,), generator=g)).values.int()
    go = torch.randn(n, h, w, generator=g)
    return proto, coeff, boxes, row_proto, go, R.rows_mask_reference(proto, coeff, boxes, row_proto, go)


@pytest.mark.parametrize("M", [8, 32, 64])
def test_generate_mask_rows_forward_and_grad_coeff(M):
    proto, coeff, boxes, row_proto, go, (mask64, gc64, mag) = mask_rows_case(M)
    p, b, rp, g = proto.to(DEV), boxes.to(DEV), row_proto.to(DEV), go.to(DEV)
    c = coeff.to(DEV).requires_grad_()
    out = layers.generate_mask_rows(p, c, b, rp)
    for s in range(proto.shape[0]):                                                       # bit-identical to per-clip generate_mask calls
        sel = torch.nonzero(rp == s).reshape(-1)
        assert torch.equal(out[sel], layers.generate_mask(p[s], c.detach()[sel], b[sel]))
    assert float((out.detach().cpu().double() - mask64).abs().max()) < 1e-5
    out.backward(g)
    ratio = LR.worst_ratio(c.grad, gc64, mag)
    print(f"\nM={M}: grad_coeff worst |g - g64| / (1e-5 * sum|terms| + 1e-7) = {ratio:.3f}")
    assert ratio <= 1.0
    again = ops.lincomb_rows_backward(g, p, c.detach(), b, rp)
    assert torch.equal(again, c.grad)                                                     # fixed-order sums
    # all rows on one prototype set: the single-set kernel's bits
    one = ops.lincomb_rows_backward(g, p[1:2], c.detach(), b, torch.zeros_like(rp))
    _, single = ops.lincomb_sigmoid_crop_backward(g, p[1], c.detach(), b, need_proto=False)
    assert torch.equal(one, single)
    # a live count in device memory: rows past it are zeros, the others unchanged
    n_dev = torch.tensor([20], dtype=torch.int32, device=DEV)
    part = ops.lincomb_rows_backward(g, p, c.detach(), b, rp, n_dev)
    assert torch.equal(part[:20], c.grad[:20]) and not part[20:].any()
    with pytest.raises(RuntimeError, match="double backward"):
        c2 = coeff.to(DEV).requires_grad_()
        (gg,) = torch.autograd.grad(layers.generate_mask_rows(p, c2, b, rp), c2, g, create_graph=True)
        gg.sum().backward()


# ------------------------------------------------------------------------------------------ end to end
def _net(name):
    return R.StandInNet(R.C_FEAT, ALL_SPECS[name]["M"], R.NET_SEED).to(DEV)


def _forward_backward(name, max_pos, sync_error=False):
    d = dev_case(name)
    d["concat_feat"] = d["concat_feat"].clone().requires_grad_()
    net = _net(name)
    old = torch.cuda.get_sync_debug_mode()
    if sync_error:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        out = loss_call(d, net, max_pos, want_status=True)
        (out["B_shift"] + out["M_shift"]).backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    return out, {k: v.grad for k, v in net.named_parameters()}, d["concat_feat"].grad


def _e2e_fractions(name, out, grads, gfeat):
    c = composition(name)
    b, m = float(out["B_shift"].detach()), float(out["M_shift"].detach())
    fl = max(abs(b - float(c["B"])) / abs(float(c["B"])), abs(m - float(c["M"])) / abs(float(c["M"])))
    fg = max(float((grads[k].cpu().double() - g).abs().max() / g.abs().max()) for k, g in c["grads"].items())
    ff = float((gfeat.cpu().double() - c["grad_feat"]).abs().max() / c["grad_feat"].abs().max())
    return fl / E2E_LOSS, fg / E2E_GRAD, ff / E2E_GRAD


@pytest.mark.parametrize("name", WITH_ROWS)
def test_loss_end_to_end_both_forms(name):
    n = composition(name)["n"]
    out, grads, gfeat = _forward_backward(name, None)
    assert out["B_shift"].dim() == 0 and out["B_shift"].dtype == torch.float32 and out["M_shift"].is_cuda
    fr = _e2e_fractions(name, out, grads, gfeat)
    print(f"\n{name} max_pos=None: losses {fr[0]:.3f}, parameter gradients {fr[1]:.3f}, grad concat_feat {fr[2]:.3f} of the end-to-end tolerance "
          f"({E2E_LOSS:.2e} / {E2E_GRAD:.2e} relative)")
    assert max(fr) <= 1.0
    out2, grads2, _ = _forward_backward(name, None)                                       # bit-identical from run to run
    assert torch.equal(out["B_shift"], out2["B_shift"]) and torch.equal(out["M_shift"], out2["M_shift"])
    _forward_backward(name, n + 3)                                                        # (warm-up: MIOpen picks its kernels for this batch size)
    for K in (n, n + 3):
        outk, gradsk, gfeatk = _forward_backward(name, K, sync_error=True)                # no host synchronisation, forward or backward
        assert int(outk["status"]) == 0
        frk = _e2e_fractions(name, outk, gradsk, gfeatk)
        print(f"{name} max_pos={K}: losses {frk[0]:.3f}, parameter gradients {frk[1]:.3f}, grad concat_feat {frk[2]:.3f}")
        assert max(frk) <= 1.0
        # the two forms agree to the last bit in the losses
        assert torch.equal(outk["B_shift"], out["B_shift"]) and torch.equal(outk["M_shift"], out["M_shift"]), (K, outk, out)
    over, gover, _ = _forward_backward(name, n - 1)                                       # overflow: NaN and the status word, never a fault
    assert int(over["status"]) == 1 and bool(torch.isnan(over["B_shift"])) and bool(torch.isnan(over["M_shift"]))
    assert all(bool(torch.isnan(g).any()) for g in gover.values())


def test_loss_without_grad_equals_the_autograd_path():
    d = dev_case("p256_b2")
    net = _net("p256_b2")
    with torch.no_grad():
        a = loss_call(d, net)
    b = loss_call(d, net)
    assert not a["B_shift"].requires_grad and b["B_shift"].requires_grad
    assert torch.equal(a["B_shift"], b["B_shift"]) and torch.equal(a["M_shift"], b["M_shift"])


def test_zero_width_next_box_gives_inf_as_the_reference():
    d = dev_case("p300_zero_width")
    with torch.no_grad():
        for K in (None, 8):
            out = loss_call(d, _net("p300_zero_width"), K)
            assert float(out["B_shift"]) == float("inf") and float(out["M_shift"]) == float("inf")
    assert _s(GOLD["p300_zero_width__B"]) == float("inf") and _s(GOLD["p300_zero_width__M"]) == float("inf")


@pytest.mark.parametrize("max_pos", [None, 4])
def test_batch_without_shift_positives_is_exactly_zero(max_pos):
    out, grads, gfeat = _forward_backward("p300_none", max_pos, sync_error=False)
    assert float(out["B_shift"]) == 0.0 and float(out["M_shift"]) == 0.0 and int(out["status"]) == 0
    assert all(g is None or not g.any() for g in grads.values()) and (gfeat is None or not gfeat.any())
