"""The sparse head's split form (planar.PlanarGraph._sparse_head with a fourth setting element, csrc/head_sparse.hip with a negative capacity):
the mask and track branches at the OWN positions only -- the pixels with a kept prior of their own, in front of the list -- and the bbox branch
alone at the positions that are listed only as the centerness partner of a kept prior.

Bit equality throughout, STM_CONV_SPLITK=1 and the 96 x 160 frames of test_gpu_sparse_head.py (levels 12x20 ... 1x2, 646 pixels, two frames per
batch), whose helpers are used."""
import pytest
import torch

from stmask_amd import ops
from stmask_amd.pipeline import BatchedClipPipeline
from test_gpu_sparse_head import (B, K, N_PIPE, SIZES, conf_thresh, dense_head, dense_steps, head, level_tables, net_and_frames,  # noqa: F401
                                  pipeline_thresh, rows_of_pixel, thresh_for)

pytestmark = pytest.mark.gpu

OWN = ops.HEAD_CTL_OWN
CTL = dict(raw=ops.HEAD_CTL_RAW, n=ops.HEAD_CTL_N, fill=ops.HEAD_CTL_FILL, a=ops.HEAD_CTL_GATE_A, b=ops.HEAD_CTL_GATE_B, dense=ops.HEAD_CTL_DENSE,
           over=ops.HEAD_CTL_OVERFLOW, pos=ops.HEAD_CTL_GATE_POS)


def split_sets(keep):
    """keep [B, N] bool -> (pixels with a kept prior of their own, centerness partner pixels without one)."""
    start, off, _, _ = level_tables()
    own, partner = set(), set()
    for b, n in keep.nonzero().tolist():
        l = max(i for i in range(len(SIZES)) if n >= off[i])
        hw = SIZES[l][0] * SIZES[l][1]
        r = n - off[l]
        own.add(start[l] + b * hw + r // K)
        partner.add(start[l] + b * hw + r % hw)
    return own, partner - own


def check_blocks(ctl, n_own, n, capacity):
    """Both control blocks against the counts: block 0 over all listed positions, block 1 the same fields over the own ones."""
    assert len(ctl) == 16
    for base, cnt in ((0, n), (OWN, n_own)):
        fill = min(capacity, -(-cnt // 256) * 256)
        got = {k: ctl[base + i] for k, i in CTL.items()}
        assert got == dict(raw=cnt, n=cnt, fill=fill, a=fill * 49, b=fill * 25, dense=0, over=0, pos=cnt), (base, got)


def split_head(net, x, thr, capacity=None):
    pred = head(net, x, (thr, capacity, True, True))
    pg = net._planar
    ctl = pg.sparse_ctl.tolist()
    lst = pg.sparse_list[:ctl[CTL["n"]]].tolist()
    return pred, ctl, lst[:ctl[OWN + CTL["n"]]], lst[ctl[OWN + CTL["n"]]:]


def check_split_rows(pred, ref, own, listed):
    """loc / mask_coeff / track at every prior row of the own pixels, centerness at the centerness rows of every listed pixel."""
    keep = torch.zeros(B, ref["loc"].shape[1], dtype=torch.bool, device="cuda")
    cen_keep = torch.zeros_like(keep)
    for m in listed:
        b, rows, cen_rows = rows_of_pixel(m)
        cen_keep[b, cen_rows] = True
        if m in own:
            keep[b, rows] = True
    assert keep.any() and cen_keep.any()
    for k in ("loc", "mask_coeff", "track"):
        assert torch.equal(pred[k][keep], ref[k][keep]), k
    assert torch.equal(pred["centerness"][cen_keep], ref["centerness"][cen_keep])


def bump(monkeypatch, priors):
    """Raise a foreground logit of the priors [(pixel, shape), ...] in front of the candidate kernel: they pass any threshold."""
    real = ops.head_candidates

    def bumped(cls_logits, *a, **kw):
        for k in sorted({k for _, k in priors}):
            cls_logits[k][torch.tensor([m for m, kk in priors if kk == k], device="cuda"), 1] += 60.0
        return real(cls_logits, *a, **kw)

    monkeypatch.setattr(ops, "head_candidates", bumped)


def forced_keep(keep, priors):
    keep = keep.clone()
    for m, k in priors:
        b, rows, _ = rows_of_pixel(m)
        keep[b, rows[k]] = True
    return keep


# ---- 1, 2: list, counts, kept rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_kept", [6, 40])
def test_list_counts_and_kept_rows(tunables, n_kept):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    ref, p = dense_head(net, frames[0])
    thr = thresh_for(p, n_kept)
    keep = p > thr
    assert int(keep.sum()) == n_kept
    own, partner = split_sets(keep)
    pred, ctl, got_own, got_partner = split_head(net, frames[0], thr)
    assert sorted(got_own) == sorted(own) and sorted(got_partner) == sorted(partner)           # exactly those pixels, each once
    check_blocks(ctl, len(own), len(own) + len(partner), net._planar.sparse_capacity(B, SIZES))
    assert torch.equal(pred["conf"], ref["conf"])
    for k in ("loc", "mask_coeff", "track", "centerness"):
        assert torch.equal(pred[k][keep], ref[k][keep]), k                                     # the rows the detection stage reads
    check_split_rows(pred, ref, own, own | partner)


def test_forced_partner_cases(tunables, monkeypatch):
    """A prior whose partner is its own pixel (level pixel 0, shape 0: row 0 -> pixel 0), and a partner pixel that has a kept prior itself
    (pixel 0 shape 1: row 1 -> pixel 1, with a prior of pixel 1 forced): listed once, in the own block."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    ref, p = dense_head(net, frames[0])
    start, _, _, _ = level_tables()
    priors = [(start[0], 0), (start[0], 1), (start[0] + 1, 1), (start[1], 0)]
    thr = thresh_for(p, 6)
    keep = forced_keep(p > thr, priors)
    own, partner = split_sets(keep)
    assert {start[0], start[0] + 1, start[1]} <= own and start[0] + 4 in partner              # (pixel 1 shape 1: row 4 -> pixel 4)
    bump(monkeypatch, priors)
    pred, ctl, got_own, got_partner = split_head(net, frames[0], thr)
    assert sorted(got_own) == sorted(own) and sorted(got_partner) == sorted(partner)
    check_blocks(ctl, len(own), len(own) + len(partner), net._planar.sparse_capacity(B, SIZES))
    for k in ("loc", "mask_coeff", "track", "centerness"):
        assert torch.equal(pred[k][keep], ref[k][keep]), k
    check_split_rows(pred, ref, own, own | partner)


def test_border_and_coarse_level_positions(tunables, monkeypatch):
    """The four corners and an edge pixel of the finest level, every pixel of the two coarsest levels (2x3, 1x2) as own positions; their partners
    land on borders as well."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    ref, p = dense_head(net, frames[0])
    start, _, ntot, _ = level_tables()
    h0, w0 = SIZES[0]
    forced = [0, w0 - 1, (h0 - 1) * w0, h0 * w0 - 1, 5 * w0, h0 * w0 + 7, h0 * w0 + (h0 - 1) * w0 + 9] + list(range(start[3], ntot))
    priors = [(m, 1) for m in forced]
    thr = thresh_for(p, 6)
    keep = forced_keep(p > thr, priors)
    own, partner = split_sets(keep)
    assert set(forced) <= own and partner
    bump(monkeypatch, priors)
    pred, ctl, got_own, got_partner = split_head(net, frames[0], thr)
    assert sorted(got_own) == sorted(own) and sorted(got_partner) == sorted(partner)
    for k in ("loc", "mask_coeff", "track", "centerness"):
        assert torch.equal(pred[k][keep], ref[k][keep]), k
    check_split_rows(pred, ref, own, own | partner)


# ---- 3 .. 6: through the pipeline ------------------------------------------------------------------------------------------------------------
def drive(net, frames, split=True, graph=False, capacity=None, nan_fill=False):
    """Packed outputs of BatchedClipPipeline over the frames with the split head, and (eager) each step's 16 control ints."""
    pipe = BatchedClipPipeline(net, B)
    pipe.sparse_head, pipe.head_split, pipe.sparse_capacity, pipe.use_graph, pipe.sparse_min_clips = True, split, capacity, graph, 1
    counts = []
    if nan_fill:
        detect = pipe._detect

        def filled(pred):
            pg = net._planar
            ctl = pg.sparse_ctl.tolist()
            lst = pg.sparse_list[:ctl[CTL["n"]]].tolist()
            own_rows = torch.zeros(B, pred["loc"].shape[1], dtype=torch.bool, device="cuda")
            rows_l, cen_l = torch.zeros_like(own_rows), torch.zeros_like(own_rows)
            for i, m in enumerate(lst):
                b, rows, cen_rows = rows_of_pixel(m)
                rows_l[b, rows] = True
                cen_l[b, cen_rows] = True
                if i < ctl[OWN + CTL["n"]]:
                    own_rows[b, rows] = True
            for k in ("mask_coeff", "track"):
                pred[k][~own_rows] = float("nan")
            pred["loc"][~rows_l] = float("nan")
            pred["centerness"][~cen_l] = float("nan")
            return detect(pred)

        pipe._detect = filled
    ys = []
    for t, x in enumerate(frames):
        ys.append(pipe.step(x, is_first=(t == 0)).clone())
        if not graph:
            counts.append(net._planar.sparse_ctl.tolist())
    torch.cuda.synchronize()
    return ys, counts


def test_nothing_else_is_read(tunables, conf_thresh):
    """NaN in front of detection: mask_coeff / track at every row that is not an own position's, loc at every row of an unlisted pixel,
    centerness at every row that is not a listed pixel's."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    thr = pipeline_thresh(net, frames, N_PIPE)
    conf_thresh(thr)
    ref = dense_steps(net, frames, thr, 3)
    ys, counts = drive(net, frames[:3], nan_fill=True)
    assert all(len(c) == 16 and 0 < c[OWN + CTL["n"]] < c[CTL["n"]] for c in counts) and any(y.abs().sum().item() > 0 for y in ref)
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))


def test_own_fill_below_fill(tunables, conf_thresh):
    """More than 256 listed positions with at most 256 own ones under a capacity of 768: the mask / track launches cover 256 patches, the bbox
    launches 512 -- the one case at this size where the two gate sets differ."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    _, p = dense_head(net, frames[0])
    thr = None
    for n_kept in range(150, 257):
        t = thresh_for(p, n_kept)
        own, partner = split_sets(p > t)
        if len(own) <= 256 < len(own) + len(partner):
            thr = t
            break
    assert thr is not None, "no threshold from 150 kept priors on lists more than 256 positions with at most 256 own ones"
    conf_thresh(thr)
    dense = dense_steps(net, frames, thr, 3)
    ys, counts = drive(net, frames[:3], capacity=768)
    c = counts[0]
    assert c[CTL["over"]] == 0 and c[OWN + CTL["fill"]] == 256 and c[CTL["fill"]] == 512 and c[OWN + CTL["n"]] <= 256 < c[CTL["n"]], c
    assert c[OWN + CTL["a"]] == 256 * 49 and c[CTL["a"]] == 512 * 49 and c[OWN + CTL["b"]] == 256 * 25 and c[CTL["b"]] == 512 * 25
    assert all(torch.equal(a, b) for a, b in zip(ys, dense))


def test_no_candidates_all_own_and_overflow(tunables, conf_thresh, monkeypatch):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    # nothing passes: both blocks are zeros (counts, fills, gates, dense gate, overflow flag), no detections
    conf_thresh(0.999999)
    ys, counts = drive(net, frames[:1])
    assert counts[0] == [0] * 16
    assert ys[0].abs().sum().item() == 0
    # more positions than the capacity: the step's head comes from the dense launches, both blocks say so
    thr = pipeline_thresh(net, frames, N_PIPE)
    conf_thresh(thr)
    ref = dense_steps(net, frames, thr, 3)
    ys, counts = drive(net, frames[:3], capacity=4)
    ntot = level_tables()[2]
    for c in counts:
        assert c[CTL["raw"]] > 4 and c[OWN + CTL["raw"]] > 0
        for base in (0, OWN):
            assert [c[base + CTL[k]] for k in ("n", "fill", "a", "b", "dense", "over", "pos")] == [0, 0, 0, 0, ntot, 1, 0], c
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))
    # every partner is itself an own position: shape 0 of level pixel 0 (row 0 -> pixel 0) of three levels and both images, nothing else kept
    start, _, _, _ = level_tables()
    ref1, p = dense_head(net, frames[0])
    priors = [(start[l] + b * SIZES[l][0] * SIZES[l][1], 0) for l in (0, 2, 4) for b in range(B)]
    bump(monkeypatch, priors)
    pred, ctl, got_own, got_partner = split_head(net, frames[0], 0.999999)
    assert sorted(got_own) == sorted(m for m, _ in priors) and got_partner == []
    check_blocks(ctl, len(priors), len(priors), net._planar.sparse_capacity(B, SIZES))
    check_split_rows(pred, ref1, set(got_own), set(got_own))


def test_graph_replay_equals_the_eager_dense_pipeline(tunables, conf_thresh):
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    thr = pipeline_thresh(net, frames, N_PIPE)
    conf_thresh(thr)
    # two eager warm-up steps, one capture + replay per slot, then every slot replayed again: what a replay leaves behind -- flags, cursors, both
    # blocks, the list, mask / track rows of other frames' positions -- meets the next one
    n = 2 + BatchedClipPipeline(net, B).n_graph_slots + 3
    frames = [frames[t % len(frames)] for t in range(n)]
    pipe = BatchedClipPipeline(net, B)
    pipe.sparse_head = False
    ref = []
    for t, x in enumerate(frames):
        ref.append(pipe.step(x, is_first=(t == 0)).clone())
    _, counts = drive(net, frames)
    assert len({(c[CTL["n"]], c[OWN + CTL["n"]]) for c in counts[2:]}) > 2, counts      # the replayed steps see different counts
    ys, _ = drive(net, frames, graph=True)
    assert all(torch.equal(a, b) for a, b in zip(ys, ref))


# ---- 7: a setting without the split element ---------------------------------------------------------------------------------------------------
def test_unsplit_form_is_unchanged(tunables):
    """(thresh, capacity, center): 8 control ints, and all three branches at every listed pixel, the centerness partners included."""
    tunables.set(STM_CONV_SPLITK=1)
    net, frames = net_and_frames()
    ref, p = dense_head(net, frames[0])
    thr = thresh_for(p, 40)
    own, partner = split_sets(p > thr)
    assert partner
    for setting in ((thr, None), (thr, None, True), (thr, None, True, False)):
        pred = head(net, frames[0], setting)
        pg = net._planar
        ctl = pg.sparse_ctl.tolist()
        assert len(ctl) == 8 and ctl[CTL["n"]] == len(own) + len(partner)
        listed = set(pg.sparse_list[:ctl[CTL["n"]]].tolist())
        assert listed == own | partner
        check_split_rows(pred, ref, listed, listed)           # every listed pixel as an own one: all four tensors at all its rows
