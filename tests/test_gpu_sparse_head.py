"""The sparse head (planar.PlanarGraph._sparse_head, csrc/head_sparse.hip): the bbox / mask / track branches of the shared prediction head at the
positions with a prior that passes the class threshold, against the dense head.

Equality is bit equality (torch.equal).  Split-K is pinned off for both sides (STM_CONV_SPLITK=1): how a launch cuts K follows from the size of
its grid, which differs between a dense launch, a launch of one branch and a launch over patches by construction -- at the workload's size no
launch of the head is cut -- while the claim under test is that each output value is the same sum in the same order.
Frames are 96 x 160 (levels 12x20, 6x10, 3x5, 2x3, 1x2), two per batch."""
import pytest
import torch

from stmask_amd import ops, synthetic
from stmask_amd.pipeline import BatchedClipPipeline
from test_gpu_parity import build

pytestmark = pytest.mark.gpu

H, W, B, K = 96, 160, 2, 3
SIZES = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
NAME = "STMask_plus_resnet50_config"
N_PIPE = 100        # kept priors of the first frame in the pipeline tests: the tracker then reports a dozen instances per step, and the
                    # positions (at most two per kept prior) fit the capacity (256)
_cache = {}


def net_and_frames():
    if "net" not in _cache:
        _cache["net"] = build(NAME, planar="fp16x2")
        clip = synthetic.synthetic_clip(6, H, W, seed=0)
        clip2 = synthetic.synthetic_clip(6, H, W, seed=7)
        _cache["frames"] = [torch.stack([clip[t], clip2[t]]).cuda().contiguous(memory_format=torch.channels_last) for t in range(6)]
    return _cache["net"], _cache["frames"]


def level_tables():
    start, off, s, o = [], [], 0, 0
    for h, w in SIZES:
        start.append(s)
        off.append(o)
        s += B * h * w
        o += K * h * w
    return start, off, s, o


def rows_of_pixel(m):
    """(image, prior rows n_k, centerness rows) of pixel m of the concatenated levels."""
    start, off, _, _ = level_tables()
    l = max(i for i in range(len(SIZES)) if m >= start[i])
    hw = SIZES[l][0] * SIZES[l][1]
    b, p = divmod(m - start[l], hw)
    return b, [off[l] + p * K + k for k in range(K)], [off[l] + k * hw + p for k in range(K)]


def pixels_read_for(keep):
    """The pixels whose head outputs the detection stage reads for the kept priors keep [B, N]: the prior's own pixel, and -- centerness
    [B, N, 1] being in (level, k, pixel) order while the stage reads it at the prior's row -- pixel r % hw for row r of the prior's level."""
    start, off, _, _ = level_tables()
    px = set()
    for b, n in keep.nonzero().tolist():
        l = max(i for i in range(len(SIZES)) if n >= off[i])
        hw = SIZES[l][0] * SIZES[l][1]
        r = n - off[l]
        px.add(start[l] + b * hw + r // K)
        px.add(start[l] + b * hw + r % hw)
    return px


def head(net, x, sparse):
    pg = net._planar
    pg.sparse = sparse
    try:
        with torch.no_grad():
            _, pred = net.forward_single(x)
        torch.cuda.synchronize()
    finally:
        pg.sparse = None
    return pred


def dense_head(net, x):
    if "dense" not in _cache:
        pred = head(net, x, None)
        p = torch.softmax(pred["conf"], -1)[..., 1:].amax(-1)             # generate_candidate's statistic, [B, N]
        _cache["dense"] = (pred, p)
    return _cache["dense"]


def thresh_for(p, n_kept):
    s = torch.sort(p.reshape(-1), descending=True).values
    return 0.5 * (s[n_kept - 1].item() + s[n_kept].item())


def check_rows(pred, ref, keep):
    """keep [B, N] bool: the four tensors must be equal at those rows (the rows the detection stage reads for a kept prior: row n of each)."""
    assert keep.any()
    for k in ("loc", "mask_coeff", "track", "centerness"):
        assert torch.equal(pred[k][keep], ref[k][keep]), k


@pytest.mark.parametrize("n_kept", [6, 40])
def test_kept_rows_equal_the_dense_head(tunables, n_kept):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    ref, p = dense_head(net, frames[0])
    thr = thresh_for(p, n_kept)
    pred = head(net, frames[0], (thr, None))
    ctl = net._planar.sparse_ctl.tolist()
    keep = p > thr
    assert int(keep.sum()) == n_kept
    # the positions found are exactly the pixels read for the kept priors, each once
    want = pixels_read_for(keep)
    got = net._planar.sparse_list[:ctl[ops.HEAD_CTL_N]].tolist()
    assert ctl[ops.HEAD_CTL_RAW] == ctl[ops.HEAD_CTL_N] == len(want) and len(got) == len(set(got)) and set(got) == want
    assert ctl[ops.HEAD_CTL_OVERFLOW] == 0
    assert torch.equal(pred["conf"], ref["conf"])
    check_rows(pred, ref, keep)


def test_border_and_coarse_level_positions(tunables, monkeypatch):
    """Positions whose 9 x 9 patch is partly or mostly outside the map: the four corners and an edge pixel of the finest level, every pixel of the
    two coarsest levels (2x3, 1x2).  They are forced by raising a foreground logit of those pixels in front of the candidate kernel."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    ref, p = dense_head(net, frames[0])
    start, _, ntot, _ = level_tables()
    h0, w0 = SIZES[0]
    forced = [0, w0 - 1, (h0 - 1) * w0, h0 * w0 - 1, 5 * w0, h0 * w0 + 7, h0 * w0 + (h0 - 1) * w0 + 9] + list(range(start[3], ntot))
    real = ops.head_candidates

    def bumped(cls_logits, *a, **kw):
        cls_logits[1][torch.tensor(forced, device="cuda"), 1] += 60.0
        return real(cls_logits, *a, **kw)

    monkeypatch.setattr(ops, "head_candidates", bumped)
    pred = head(net, frames[0], (thresh_for(p, 6), None))
    ctl = net._planar.sparse_ctl.tolist()
    listed = set(net._planar.sparse_list[:ctl[ops.HEAD_CTL_N]].tolist())
    assert set(forced) <= listed
    keep = torch.zeros_like(p, dtype=torch.bool)
    cen_keep = torch.zeros_like(keep)
    for m in listed:
        b, rows, cen_rows = rows_of_pixel(m)
        keep[b, rows] = True                                                       # every prior of a listed pixel is computed
        cen_keep[b, cen_rows] = True
    for k in ("loc", "mask_coeff", "track"):
        assert torch.equal(pred[k][keep], ref[k][keep]), k
    assert torch.equal(pred["centerness"][cen_keep], ref["centerness"][cen_keep])
    # conf: everywhere but at the rows whose logit the test itself raised (kernel shape 1 of the forced pixels)
    same = torch.ones_like(p, dtype=torch.bool)
    for m in forced:
        b, rows, _ = rows_of_pixel(m)
        same[b, rows[1]] = False
    assert torch.equal(pred["conf"][same], ref["conf"][same])


def drive(net, frames, sparse, graph=False, capacity=None, nan_fill=False):
    pipe = BatchedClipPipeline(net, B)
    pipe.sparse_head, pipe.sparse_capacity, pipe.use_graph, pipe.sparse_min_clips = sparse, capacity, graph, 1
    counts = []
    if nan_fill:
        detect = pipe._detect

        def filled(pred):
            pg = net._planar
            ctl = pg.sparse_ctl.tolist()
            keep = torch.zeros(B, pred["loc"].shape[1], dtype=torch.bool, device="cuda")
            cen_keep = torch.zeros_like(keep)
            for m in pg.sparse_list[:ctl[ops.HEAD_CTL_N]].tolist():
                b, rows, cen_rows = rows_of_pixel(m)
                keep[b, rows] = True
                cen_keep[b, cen_rows] = True
            for k in ("loc", "mask_coeff", "track"):
                pred[k][~keep] = float("nan")
            pred["centerness"][~cen_keep] = float("nan")
            return detect(pred)

        pipe._detect = filled
    ys = []
    for t, x in enumerate(frames):
        ys.append(pipe.step(x, is_first=(t == 0)).clone())
        if sparse and not graph:
            counts.append(net._planar.sparse_ctl.tolist())
    torch.cuda.synchronize()
    return ys, counts


def pipeline_thresh(net, frames, n_kept):
    _, p = dense_head(net, frames[0])
    return thresh_for(p, n_kept)


@pytest.fixture
def conf_thresh():
    net, _ = net_and_frames()
    old = net.cfg.eval_conf_thresh

    def set_(v):
        net.cfg.eval_conf_thresh = v
    yield set_
    net.cfg.eval_conf_thresh = old


def dense_steps(net, frames, thr, n):
    key = ("steps", thr, n)
    if key not in _cache:
        _cache[key] = drive(net, frames[:n], False)[0]
    return _cache[key]


def test_rows_that_are_not_kept_are_never_read(tunables, conf_thresh):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    thr = pipeline_thresh(net, frames, N_PIPE)
    conf_thresh(thr)
    ref = dense_steps(net, frames, thr, 3)
    ys, counts = drive(net, frames[:3], True, nan_fill=True)
    assert all(c[ops.HEAD_CTL_N] > 0 for c in counts) and any(y.abs().sum().item() > 0 for y in ref)
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))


def test_no_candidates_and_overflow(tunables, conf_thresh):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    # nothing passes: empty patch launches, no detections
    conf_thresh(0.999999)
    ys, counts = drive(net, frames[:1], True)
    assert counts[0][ops.HEAD_CTL_RAW] == 0 and counts[0][ops.HEAD_CTL_GATE_A] == 0 and counts[0][ops.HEAD_CTL_DENSE] == 0
    assert ys[0].abs().sum().item() == 0                        # (packed rows [B, top_k, 40]: an empty slot is a row of zeros)
    # more positions than the capacity: the step's head comes from the dense launches
    thr = pipeline_thresh(net, frames, N_PIPE)
    conf_thresh(thr)
    ref = dense_steps(net, frames, thr, 3)
    ys, counts = drive(net, frames[:3], True, capacity=4)
    assert all(c[ops.HEAD_CTL_OVERFLOW] == 1 and c[ops.HEAD_CTL_N] == 0 and c[ops.HEAD_CTL_RAW] > 4 for c in counts)
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))


def test_graph_replay_equals_the_eager_dense_pipeline(tunables, conf_thresh):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    thr = pipeline_thresh(net, frames, N_PIPE)
    conf_thresh(thr)
    # two eager warm-up steps, one capture + replay per slot, then every slot replayed again (what a replay leaves behind -- the list, the counts,
    # the flags, rows of other frames' positions -- meets the next one)
    n = 2 + BatchedClipPipeline(net, B).n_graph_slots + 3
    frames = [frames[t % len(frames)] for t in range(n)]
    ref = drive(net, frames[:n], False)[0]
    _, counts = drive(net, frames[:n], True)
    assert len({c[ops.HEAD_CTL_N] for c in counts[2:]}) > 2, counts      # the replayed steps see different candidate counts
    ys, _ = drive(net, frames[:n], True, graph=True)
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))


# ---- gated convolution launches (ops.conv_set_pixel_gate) on each kernel the sparse head's launches reach at the workload's size --------------------
def _gated_case(kind):
    """(conv, planes, shape, M): a layer that lands on the kx-reuse kernel for narrow layers / on conv_planar_kx3_kernel / on conv_planar_kernel's
    128 x 64 tiles, over 5 x 5 or 9 x 9 maps as the patch launches are."""
    from stmask_amd.planar import PlanarConv
    g = torch.Generator().manual_seed(11)
    if kind == "kxr":
        C, G, cg, real, hw, n = 64, 2, 64, [5, 32], (5, 5), 400
        w = torch.randn(G * cg, C, 3, 5, generator=g) * (C * 15) ** -0.5
        for i in range(G):
            w[i * cg + real[i]:(i + 1) * cg] = 0.0
        conv = PlanarConv(w.cuda(), torch.randn(G * cg, generator=g).cuda(), 1, (1, 2), relu=False, groups=G, group_cout=real, tile_n=64, fmt=1)
        assert conv.kxr
        kw = dict(kxr=True)
    elif kind == "kx3":
        C, G, hw, n = 64, 1, (9, 9), 320
        w = torch.randn(256, C, 3, 3, generator=g) * (C * 9) ** -0.5
        conv = PlanarConv(w.cuda(), torch.randn(256, generator=g).cuda(), 1, 1, relu=True, fmt=1)
        kw = {}
    else:
        C, G, hw, n = 64, 1, (5, 5), 400
        w = torch.randn(128, C, 3, 3, generator=g) * (C * 9) ** -0.5
        conv = PlanarConv(w.cuda(), torch.randn(128, generator=g).cuda(), 1, 1, relu=False, tile_n=64, fmt=1)
        kw = dict(kxr=False)
    M = n * hw[0] * hw[1]
    x = ops.split_planes(torch.randn(M, G * C, generator=g).cuda(), 1)
    return conv, x, ("levels", n, [hw]), M, kw


@pytest.mark.parametrize("kind", ["kxr", "kx3", "planar64"])
def test_gated_launches_equal_the_ungated_ones_below_the_gate(kind):
    """Gates of 0, a multiple of every tile height, a value inside a tile, all pixels and more: rows below the gate equal the ungated launch, a
    row past it is either untouched or -- its tile started below the gate (tiles are at most 1 024 pixels high) -- the ungated value, and no row
    from 1 024 past the gate on is written."""
    from stmask_amd import _lib
    conv, x, shape, M, kw = _gated_case(kind)
    n0 = _lib.lib().stm_debug_launch_count(0)
    ref = conv(x, shape, out="f32", splitk=False, **kw)
    if kind == "kx3":
        assert _lib.lib().stm_debug_launch_count(0) == n0 + 1          # the layer did land on conv_planar_kx3_kernel
    ctl = torch.zeros(8, dtype=torch.int32, device="cuda")
    for gate in (0, 2048, 3000, M - 7, M, M + 100):
        ctl[3] = gate
        out = torch.full_like(ref, 12345.0)
        conv(x, shape, out="f32", out_f32=out, gate=(ctl, 3), **kw)
        torch.cuda.synchronize()
        lo = min(gate, M)
        cols = slice(0, ref.shape[1]) if kind != "kxr" else None
        if kind == "kxr":
            # (the kernel writes whole 16-channel tiles of a group: the real channels are what is compared)
            keep = torch.zeros(ref.shape[1], dtype=torch.bool, device="cuda")
            keep[0:5] = True
            keep[64:96] = True
            r, o = ref[:, keep], out[:, keep]
        else:
            r, o = ref[:, cols], out[:, cols]
        assert torch.equal(o[:lo], r[:lo]), (kind, gate)
        past = o[lo:]
        assert bool(((past == 12345.0) | (past == r[lo:])).all()), (kind, gate)
        assert bool((o[min(M, lo + 1024):] == 12345.0).all()), (kind, gate)
        if gate == 0:
            assert bool((out == 12345.0).all())


def test_gated_kxr_launch_over_several_levels_runs_nothing_or_everything():
    """The form of the dense launches of the three branches: several levels in one launch, gate 0 (no overflow) or all pixels (overflow)."""
    from stmask_amd.planar import PlanarConv
    g = torch.Generator().manual_seed(12)
    sizes, Bn, C = [(12, 20), (6, 10), (3, 5)], 8, 64
    M = sum(Bn * h * w for h, w in sizes)
    w = torch.randn(64, C, 3, 3, generator=g) * (C * 9) ** -0.5
    w[41:] = 0.0
    conv = PlanarConv(w.cuda(), torch.randn(64, generator=g).cuda(), 1, 1, relu=False, group_cout=[41], tile_n=64, fmt=1)
    assert conv.kxr
    x = ops.split_planes(torch.randn(M, C, generator=g).cuda(), 1)
    shape = ("levels", Bn, sizes)
    ref = conv(x, shape, out="f32", kxr=True)
    ctl = torch.zeros(8, dtype=torch.int32, device="cuda")
    for gate in (0, M):
        ctl[5] = gate
        out = torch.full_like(ref, 12345.0)
        conv(x, shape, out="f32", out_f32=out, gate=(ctl, 5), kxr=True)
        torch.cuda.synchronize()
        assert bool((out == 12345.0).all()) if gate == 0 else torch.equal(out[:, :41], ref[:, :41])


def test_a_changed_threshold_recaptures_the_trunk_graphs(tunables, conf_thresh):
    """eval_conf_thresh is baked into a captured trunk graph while the detection stage reads it live: lowering it between steps must not leave the
    stage reading rows the sparse head did not write."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    hi, lo = pipeline_thresh(net, frames, 40), pipeline_thresh(net, frames, N_PIPE)
    outs = {}
    for sparse in (False, True):
        pipe = BatchedClipPipeline(net, B)
        pipe.sparse_head, pipe.use_graph, pipe.sparse_min_clips = sparse, True, 1
        ys = []
        for t in range(8):
            conf_thresh(hi if t < 4 else lo)
            ys.append(pipe.step(frames[t % len(frames)], is_first=(t == 0)).clone())
        torch.cuda.synchronize()
        outs[sparse] = ys
    assert any(y.abs().sum().item() > 0 for y in outs[False][4:])
    assert all(torch.equal(a, b) for a, b in zip(outs[True], outs[False]))
