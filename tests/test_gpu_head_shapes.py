"""The sparse head's shapes form (planar.PlanarGraph._sparse_patches_shapes, SparseHead.shapes; csrc/head_sparse.hip with K << 28 added to the
capacity; the gated window set of csrc/conv_bf16x.hip): the list holds (pixel, kernel shape) entries, one segment per shape, and the patch towers
run over the rectangle that shape's output layers read at the centre -- kh x kw of tower 2, (kh + 2) x (kw + 2) of tower 1.

The head alone on random `up` planes: 2 frames, three levels of 12x20, 6x10 and 3x5 (on the last every footprint crosses a border), 256 channels,
the class logits overwritten in front of the candidate kernel so that the kept set is the test's.  Every buffer the head allocates is pre-filled
with NaN, so a row or patch pixel the form does not compute shows.  Comparisons are torch.equal against the dense head's rows: per output pixel
the same products in the same order, nothing to bound.  STM_CONV_SPLITK=1 on both sides as in test_gpu_sparse_head.py, whose net is used."""
import pytest
import torch

from stmask_amd import ops, planar
from stmask_amd.pipeline import BatchedClipPipeline
from test_gpu_sparse_head import B as PIPE_B
from test_gpu_sparse_head import N_PIPE, conf_thresh, net_and_frames, pipeline_thresh  # noqa: F401

pytestmark = pytest.mark.gpu

B, K = 2, 3
SIZES = [(12, 20), (6, 10), (3, 5)]
HW = [h * w for h, w in SIZES]
START = [0, B * HW[0], B * (HW[0] + HW[1]), B * sum(HW)]
OFF = [0, K * HW[0], K * (HW[0] + HW[1])]
N = K * sum(HW)
NTOT = START[3]
SEG, OWN = ops.HEAD_CTL_SEG, ops.HEAD_CTL_OWN
_cache = {}


def pixel(l, b, y, x):
    return START[l] + b * HW[l] + y * SIZES[l][1] + x


def split_pixel(m):
    l = max(i for i in range(len(SIZES)) if m >= START[i])
    b, p = divmod(m - START[l], HW[l])
    return l, b, p


def entries_of(kept):
    """kept = {(pixel, shape)} -> (own entries, partner entries): centerness is stored in (level, k, pixel) order and read at the prior's row
    r = p K + k, so the value that goes with a kept prior is shape r // hw at pixel r % hw of its level and image."""
    own, partner = set(kept), set()
    for m, k in kept:
        l, b, p = split_pixel(m)
        r = p * K + k
        partner.add((START[l] + b * HW[l] + r % HW[l], r // HW[l]))
    return own, partner


def row(m, k):
    l, b, p = split_pixel(m)
    return b * N + OFF[l] + p * K + k


def cen_row(m, k):
    l, b, p = split_pixel(m)
    return b * N + OFF[l] + k * HW[l] + p


def setup(kx=False):
    """(planar graph, levels, up planes, dense head (conf, loc, mask, track, centerness)), once per kernel family of the output layers."""
    if "up" not in _cache:
        net, _ = net_and_frames()
        g = torch.Generator().manual_seed(5)
        up = ops.split_planes((torch.randn(NTOT, 256, generator=g).clamp_(min=0) * 0.5).cuda(), 1)
        lv = planar._Levels(B, tuple(SIZES), tuple(START), NTOT, torch.device("cuda", torch.cuda.current_device()))
        _cache["pg"], _cache["lv"], _cache["up"] = net._planar, lv, up
    pg, lv, up = _cache["pg"], _cache["lv"], _cache["up"]
    assert pg.fmt == 1 and pg.sparse_supported() and [(f.small.kh, f.small.kw) for f in pg.finals] == [(3, 3), (3, 5), (5, 3)]
    if ("dense", kx) not in _cache:
        outs = pg._dense_head(up, lv, lambda name: None)
        head = pg.head
        _cache["dense", kx] = ops.head_assemble([o[0] for o in outs], [o[1] for o in outs], B, SIZES, head.num_classes, head.mask_dim, head.embed_dim,
                                                pg.GROUP_PAD)
        torch.cuda.synchronize()
    return pg, lv, up, _cache["dense", kx]


def run_head(monkeypatch, pg, lv, up, kept, capacity=None, shapes=True):
    """The sparse head with the class logits forced: background 30 everywhere, a foreground logit of 90 at the kept (pixel, shape) priors, threshold
    0.5.  torch.empty hands out NaN (floating point) or 85 (integers) while the head runs."""
    real_cand, real_empty = ops.head_candidates, torch.empty

    def forced(cls_logits, *a, **kw):
        for t in cls_logits:
            t.zero_()
            t[:, 0] = 30.0
        for m, k in kept:
            cls_logits[k][m, 1] = 90.0
        return real_cand(cls_logits, *a, **kw)

    def filled(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(85)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "head_candidates", forced)
        mp.setattr(torch, "empty", filled)
        pg.sparse = (0.5, capacity, True, True, shapes)
        try:
            with torch.no_grad():
                out = pg._sparse_head(up, lv, lambda name: None)
            torch.cuda.synchronize()
        finally:
            pg.sparse = None
    ops.check_planar_range()           # no tower launch met a value it had not been given
    return out


def written(t):
    return ~torch.isnan(t.reshape(B * N, -1)).any(1)


def rows_mask(rows):
    m = torch.zeros(B * N, dtype=torch.bool, device="cuda")
    m[torch.tensor(sorted(rows), dtype=torch.long, device="cuda")] = True
    return m


def check_shapes_run(pg, out, ref, kept, cap):
    """Segments, counts and gates of the control block; exactly the rows of the entries are written, and they hold the dense head's values."""
    own, partner = entries_of(kept)
    ent = own | partner
    ctl, lst, seg_cap = pg.sparse_segments
    assert seg_cap == cap
    c, lst = ctl.tolist(), lst.tolist()
    assert len(c) == SEG * (K + 1)
    px = [((kh + 2) * (kw + 2), kh * kw) for kh, kw in ((3, 3), (3, 5), (5, 3))]
    for k in range(K):
        for base, es in ((0, ent), (OWN, own)):
            n = sum(1 for _, kk in es if kk == k)
            fill = min(cap, -(-n // 256) * 256)
            got = c[SEG * (k + 1) + base:SEG * (k + 1) + base + 8]
            assert got == [n, n, fill, fill * px[k][0], fill * px[k][1], 0, 0, n], (k, base, got)
        n_own, n = c[SEG * (k + 1) + OWN + 1], c[SEG * (k + 1) + 1]
        assert sorted(lst[k * cap:k * cap + n_own]) == sorted(m for m, kk in own if kk == k)
        assert sorted(lst[k * cap + n_own:k * cap + n]) == sorted(m for m, kk in partner - own if kk == k)
    assert c[:8] == [len(ent), len(ent)] + [sum(c[SEG * (k + 1) + i] for k in range(K)) for i in (2, 3, 4)] + [0, 0, len(ent)]
    assert pg.sparse_ctl.tolist() == c[:SEG] and sorted(pg.sparse_list.tolist()) == sorted(m for m, _ in ent)
    _, loc, mask, track, cen = out
    _, rloc, rmask, rtrack, rcen = ref
    want = {"loc": rows_mask({row(m, k) for m, k in ent}), "mask": rows_mask({row(m, k) for m, k in own}),
            "track": rows_mask({row(m, k) for m, k in own}), "cen": rows_mask({cen_row(m, k) for m, k in ent})}
    assert {row(m, k) for m, k in kept} <= {cen_row(m, k) for m, k in ent}          # the centerness the detection stage reads with a kept prior
    for name, t, r in (("loc", loc, rloc), ("mask", mask, rmask), ("track", track, rtrack), ("cen", cen, rcen)):
        w = written(t)
        assert torch.equal(w, want[name]), (name, int(w.sum()), int(want[name].sum()))
        assert torch.equal(t.reshape(B * N, -1)[w], r.reshape(B * N, -1)[w]), name


@pytest.fixture
def kxr_everywhere(monkeypatch):
    """The output layers on the kx-reuse kernel at this size as well (the family they run on at the workload's): dense and sparse side alike."""
    monkeypatch.setattr(planar.PlanarConv, "kxr_rule_pixels", lambda self: 0)


# ---- interior, corners, edges; the 3x5 level ----------------------------------------------------------------------------------------------
def position_cases(k):
    h, w = SIZES[0]
    px = [(5, 9), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 7), (h - 1, 7), (5, 0), (5, w - 1)]
    kept = {(pixel(0, 0, y, x), k) for y, x in px}
    kept |= {(pixel(2, 1, y, x), k) for y in range(SIZES[2][0]) for x in range(SIZES[2][1])}       # every pixel of the 3x5 level, second image
    kept |= {(pixel(1, 1, 2, 3), k), (pixel(1, 0, 5, 9), k)}
    return kept


@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_shape_at_interior_corner_and_edge_pixels(tunables, monkeypatch, k):
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup()
    kept = position_cases(k)
    out = run_head(monkeypatch, pg, lv, up, kept)
    check_shapes_run(pg, out, ref, kept, 256)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_output_layers_on_the_kx_reuse_kernel(tunables, monkeypatch, kxr_everywhere, k):
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup(kx=True)
    kept = position_cases(k)
    out = run_head(monkeypatch, pg, lv, up, kept)
    check_shapes_run(pg, out, ref, kept, 256)


def test_pixels_with_two_and_three_shapes(tunables, monkeypatch):
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup()
    a, b3, c = pixel(0, 0, 4, 4), pixel(0, 1, 0, 19), pixel(2, 0, 1, 2)
    kept = {(a, 0), (a, 2), (b3, 0), (b3, 1), (b3, 2), (c, 1), (c, 2)}
    out = run_head(monkeypatch, pg, lv, up, kept)
    ctl, lst, cap = pg.sparse_segments
    n = [ctl[SEG * (k + 1) + 1].item() for k in range(K)]
    assert sum(b3 in lst[k * cap:k * cap + n[k]].tolist() for k in range(K)) == 3 and sum(a in lst[k * cap:k * cap + n[k]].tolist() for k in range(K)) >= 2
    check_shapes_run(pg, out, ref, kept, 256)


def test_partner_entry_at_a_pixel_that_is_an_own_entry_of_another_shape(tunables, monkeypatch):
    """Prior (pixel 100 of image 0 on level 0, shape 1) is row 301: its centerness is shape 1 at pixel 61.  Pixel 61 keeps shape 2 only: it is
    an own entry of segment 2 and a partner-only entry of segment 1."""
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup()
    m, mp_ = pixel(0, 0, 5, 0), pixel(0, 0, 3, 1)
    assert (m - START[0]) * K + 1 == 301 and 301 % HW[0] == mp_ - START[0] and 301 // HW[0] == 1
    kept = {(m, 1), (mp_, 2)}
    own, partner = entries_of(kept)
    assert (mp_, 1) in partner - own and (mp_, 2) in own
    out = run_head(monkeypatch, pg, lv, up, kept)
    check_shapes_run(pg, out, ref, kept, 256)


def test_zero_candidates(tunables, monkeypatch):
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup()
    out = run_head(monkeypatch, pg, lv, up, set())
    assert pg.sparse_segments[0].tolist() == [0] * (SEG * (K + 1))
    for t in out[1:]:
        assert not written(t).any()


def test_one_segment_over_its_capacity(tunables, monkeypatch):
    """Five priors of shape 0 at pixels below hw / K of level 0 (their partners are shape 0 as well) under 4 entries per segment: segment 0 is
    over, the two others are empty -- the dense launches run and every row is the dense head's."""
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup()
    kept = {(pixel(0, 0, 0, x), 0) for x in (2, 5, 8, 11, 14)}
    own, partner = entries_of(kept)
    assert all(k == 0 for _, k in own | partner)
    out = run_head(monkeypatch, pg, lv, up, kept, capacity=4)
    ctl, _, cap = pg.sparse_segments
    c = ctl.tolist()
    assert cap == 4 and c[SEG + ops.HEAD_CTL_RAW] == len(own | partner) > 4 and c[2 * SEG] == c[3 * SEG] == 0
    for base in [0, OWN] + [SEG * (k + 1) + o for k in range(K) for o in (0, OWN)]:
        assert c[base + 1:base + 8] == [0, 0, 0, 0, NTOT, 1, 0], (base, c)
    for t, r in zip(out[1:], ref[1:]):
        assert torch.equal(t, r)


def test_switch_off_is_the_split_form(tunables, monkeypatch):
    """The same kept set with the fifth element off: 16 control ints, a list of pixels -- and the same values at the rows both forms compute."""
    tunables.set(STM_CONV_SPLITK=1)
    pg, lv, up, ref = setup()
    kept = position_cases(1) | {(pixel(0, 0, 4, 4), 0), (pixel(0, 0, 4, 4), 2)}
    on = run_head(monkeypatch, pg, lv, up, kept)
    off = run_head(monkeypatch, pg, lv, up, kept, shapes=False)
    assert pg.sparse_segments is None and len(pg.sparse_ctl) == 16
    own, partner = entries_of(kept)
    assert pg.sparse_ctl[ops.HEAD_CTL_N].item() == len({m for m, _ in own | partner})
    for a, b_ in zip(on[1:], off[1:]):
        w = written(a)
        assert w.any() and not (w & ~written(b_)).any()
        assert torch.equal(a.reshape(B * N, -1)[w], b_.reshape(B * N, -1)[w])


# ---- through the pipeline: graph replay, and the switch ------------------------------------------------------------------------------------
def drive(net, frames, shapes, graph=False, sparse=True):
    pipe = BatchedClipPipeline(net, PIPE_B)
    pipe.sparse_head, pipe.head_split, pipe.head_center, pipe.head_shapes, pipe.use_graph, pipe.sparse_min_clips = sparse, True, True, shapes, graph, 1
    ys, counts = [], []
    for t, x in enumerate(frames):
        ys.append(pipe.step(x, is_first=(t == 0)).clone())
        if sparse and not graph:
            pg = net._planar
            assert (pg.sparse_segments is not None) == shapes
            counts.append(tuple(pg.sparse_ctl.tolist()[i] for i in (ops.HEAD_CTL_N, OWN + ops.HEAD_CTL_N)))
    torch.cuda.synchronize()
    return ys, counts


def test_graph_replay_and_the_switch_against_the_eager_dense_pipeline(tunables, conf_thresh):
    """Two eager warm-up steps, one capture + replay per slot, then every slot replayed again, the kept set changing from step to step: what a
    replay leaves behind (flags, cursors, every block, the segments, patch pixels outside this step's windows) meets the next one."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    conf_thresh(pipeline_thresh(net, frames, N_PIPE))
    n = 2 + BatchedClipPipeline(net, PIPE_B).n_graph_slots + 3
    frames = [frames[t % len(frames)] for t in range(n)]
    ref, _ = drive(net, frames, False, sparse=False)
    on, counts = drive(net, frames, True)
    assert len(set(counts[2:])) > 2 and all(0 < o < a for a, o in counts), counts
    assert all(torch.equal(a, b) for a, b in zip(on, ref)) and any(y.abs().sum().item() > 0 for y in ref)
    off, _ = drive(net, frames[:3], False)                     # STM_HEAD_SHAPES=0 on the same inputs
    assert all(torch.equal(a, b) for a, b in zip(off, on))
    ys, _ = drive(net, frames, True, graph=True)
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))


# ---- the gated window set alone ------------------------------------------------------------------------------------------------------------
WINDOWS = {"t1": [(5, 5, 1, 1), (5, 7, 1, 0), (7, 5, 0, 1)], "t2g": [(3, 3, 1, 1), (3, 5, 1, 0), (5, 3, 0, 1)]}


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("case", ["t1", "t2g"])
def test_gated_window_set_equals_the_full_window_gated_launch(case, rot):
    """One window per segment, counts 0 / 13 (the gate ends inside the second 256-pixel tile) / all 40 images dealt to the segments in turn: a window
    row below its segment's gate equals that row of the single gated launch over the whole map; a row from the gate up to the end of the tile the
    gate lies in is either that value or untouched; everything else -- the map outside the window, other slabs -- stays NaN.  t1: tower 1's
    geometry (9x9 -> 7x7, one group); t2g: tower 2's of the mask + track branches (7x7 -> 5x5, two groups reading from channel 256 of 768, written
    from slab 8 of 24)."""
    gen = torch.Generator().manual_seed(3 + rot)
    cap, S_in = 40, (9 if case == "t1" else 7)
    S_out, G = S_in - 2, (1 if case == "t1" else 2)
    tot = 3 * cap
    w = torch.randn(G * 256, 256, 3, 3, generator=gen) * (256 * 9) ** -0.5
    conv = planar.PlanarConv(w.cuda(), torch.randn(G * 256, generator=gen).cuda(), 1, 0, relu=True, groups=G, fmt=1)
    x_ch, slab0, slabs_out, c_in = (0, 0, 8, 256) if case == "t1" else (256, 8, 24, 768)
    x = ops.split_planes(torch.randn(tot * S_in * S_in, c_in, generator=gen).cuda(), 1)
    counts = [[0, 13, cap][(k + rot) % 3] for k in range(3)]
    ctl = torch.zeros(64, dtype=torch.int32, device="cuda")
    for k, (ho, wo, _, _) in enumerate(WINDOWS[case]):
        ctl[3 + 16 * k] = counts[k] * ho * wo
    ctl[60] = tot * S_out * S_out
    nan16 = lambda: torch.full((2, slabs_out, tot * S_out * S_out, 32), float("nan"), dtype=torch.float16, device="cuda")
    ref, out = nan16(), nan16()
    conv(x, ("img", tot, S_in, S_in), out="planes", out_planes=ref, x_ch_off=x_ch, out_slab_off=slab0, window=(0, 0, S_out, S_out, 0, 0, S_out, S_out),
         gate=(ctl, 60))
    conv.window_segments(x, tot, S_in, S_in, WINDOWS[case], out, S_out, (ctl, 3), x_ch_off=x_ch, out_slab_off=slab0)
    torch.cuda.synchronize()
    ops.check_planar_range()
    nsl = G * 8
    assert not torch.isnan(ref[:, slab0:slab0 + nsl]).any()
    # per pixel of the output maps: 2 = must be written, 1 = may be written, 0 = must stay NaN
    need = torch.zeros(tot, S_out, S_out, dtype=torch.int8)
    for k, (ho, wo, y0, x0) in enumerate(WINDOWS[case]):
        gate = counts[k] * ho * wo
        upto = min(-(-gate // 256) * 256, cap * ho * wo)
        m = torch.arange(cap * ho * wo).view(cap, ho, wo)
        need[k * cap:(k + 1) * cap, y0:y0 + ho, x0:x0 + wo] = (m < gate).to(torch.int8) * 2 + ((m >= gate) & (m < upto)).to(torch.int8)
    need = need.view(-1).cuda()
    got = out.view(torch.int16)
    isn = torch.isnan(out)
    assert isn[:, :slab0].all() and isn[:, slab0 + nsl:].all()
    o, r, isn = got[:, slab0:slab0 + nsl], ref.view(torch.int16)[:, slab0:slab0 + nsl], isn[:, slab0:slab0 + nsl]
    px_nan = isn.all(3).all(1).all(0)                       # a pixel is untouched: NaN in every plane, slab and channel
    px_eq = (o == r).all(3).all(1).all(0)
    assert (px_nan | px_eq).all()
    assert px_eq[need == 2].all() and px_nan[need == 0].all()
    assert int((need == 2).sum()) == sum(counts[k] * WINDOWS[case][k][0] * WINDOWS[case][k][1] for k in range(3)) > 0
