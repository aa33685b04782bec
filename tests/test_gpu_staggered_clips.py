"""Per-clip is_first / active in BatchedClipPipeline on the MI355X: clips that start and stop on different frames share one batch.

Scenario (B = 3, 7 steps, 128x192 synthetic clips): slot 0 plays video A (4 frames) then A2 (3) from t = 4; slot 1 plays B (7) throughout; slot 2
plays C (2), is idle (a frame of zeros, active = False) at t = 2..3 and plays C2 (3) from t = 4.
* isolation: slot 1 -- and every slot before its first change -- is bit-identical to the same frame batches run with a scalar is_first at t = 0
  only (eager, and with graph-replayed trunks plus look-ahead);
* reset slot: from t = 4 on, slots 0 and 2 are bit-identical to the same batches run with a scalar is_first=True at t = 4;
* semantics: every video's frames match the module path on that video alone (STMask.forward, test_host_model_cpu.run_clip).
Both bit-identity checks rest on every tail kernel computing a row from that row's inputs alone (not from its index in the concatenated tracked
set or from what the other clips hold).  One stage does not: the planar TemporalNet (planar.PlanarTemporalNet.forward_planes) takes another
arithmetic path -- border-class convolutions with the pooled fc -- once the step's tracked set reaches 16384 RoI pixels (335 rows of 7x7), so a clip's
rows depend on the OTHER clips' row count when the two compared runs fall on different sides of that switch (FCB-ada here: 291 against 426 rows).
From that step on the check is bounded instead: ids and classes exact, every value within 1e-5 (measured on the MI355X: at most 1.0e-6)."""
import pytest
import torch

from stmask_amd import synthetic
from stmask_amd.pipeline import BatchedClipPipeline
from test_gpu_parity import build
from test_host_model_cpu import run_clip

pytestmark = pytest.mark.gpu

NETS = [("STMask_plus_resnet50_config", True), ("STMask_plus_resnet50_ada_config", True), ("STMask_plus_resnet50_config", False)]
IDS = ["r50_fca_tf", "r50_fcb_ada_tf", "r50_non_tf"]
H, W, T = 128, 192, 7
TN_SWITCH_ROWS = -(-16384 // 49)     # planar.PlanarTemporalNet.forward_planes: the row count from which TemporalNet takes its other path
BOUND = 1e-5

_nets = {}


def net_for(name, tf, planar=None):
    key = (name, tf, planar)
    if key not in _nets:
        _nets[key] = build(name, planar=planar, temporal_fusion=tf)
    return _nets[key]


def videos():
    return {"A": synthetic.synthetic_clip(4, H, W, seed=0), "A2": synthetic.synthetic_clip(3, H, W, seed=3),
            "B": synthetic.synthetic_clip(7, H, W, seed=5), "C": synthetic.synthetic_clip(2, H, W, seed=9),
            "C2": synthetic.synthetic_clip(3, H, W, seed=11)}


# per step: (video, frame) per slot, None = idle
SLOTS = [[("A", t) if t < 4 else ("A2", t - 4) for t in range(T)],
         [("B", t) for t in range(T)],
         [("C", t) if t < 2 else (None if t < 4 else ("C2", t - 4)) for t in range(T)]]
STAG_FIRST = [True, [False] * 3, [False] * 3, [False] * 3, [True, False, True], [False] * 3, [False] * 3]
STAG_ACTIVE = [None, None, [True, True, False], [True, True, False], None, None, None]


def batches(v, slots, channels_last=False):
    z = torch.zeros(3, H, W)
    out = []
    for t in range(len(slots[0])):
        x = torch.stack([z if s[t] is None else v[s[t][0]][s[t][1]] for s in slots]).cuda()
        out.append(x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous())
    return out


def drive(net, xs, firsts, actives=None, graph=False, depth=0):
    pipe = BatchedClipPipeline(net, xs[0].shape[0])
    pipe.use_graph = graph
    res = []
    for t, x in enumerate(xs):
        nxt = xs[t + 1:t + 1 + depth] if depth else None
        y = pipe.step(x, is_first=firsts[t], next_frames=nxt or None, active=None if actives is None else actives[t])
        res.append((y.clone(), pipe.detections(), list(pipe.prev_n)))
    torch.cuda.synchronize()
    return res


def same_slot(r1, r2, b):
    (y1, d1, _), (y2, d2, _) = r1, r2
    if not torch.equal(y1[b], y2[b]):
        return False
    if not d1[b] or not d2[b]:
        return (not d1[b] or d1[b]["box"].shape[0] == 0) and (not d2[b] or d2[b]["box"].shape[0] == 0)
    return d1[b].keys() == d2[b].keys() and all(torch.equal(d1[b][k], d2[b][k]) for k in d1[b])


def empty(d):
    return not d or d["box"].shape[0] == 0


def close_slot(r1, r2, b):
    """The bounded form of same_slot (see the module docstring)."""
    (y1, d1, _), (y2, d2, _) = r1, r2
    if (y1[b] - y2[b]).abs().max().item() > BOUND:
        return False
    if empty(d1[b]) or empty(d2[b]):
        return empty(d1[b]) and empty(d2[b])
    return (torch.equal(d1[b]["box_ids"], d2[b]["box_ids"]) and torch.equal(d1[b]["class"], d2[b]["class"])
            and all((d1[b][k] - d2[b][k]).abs().max().item() <= BOUND for k in ("box", "score", "mask_coeff", "mask")))


def shift_rows(res, firsts, actives):
    """Rows of the tracked set CandidateShift runs TemporalNet on, per step (after that step's per-clip drops)."""
    out, prev = [], [0] * 3
    for t in range(len(res)):
        f, a = firsts[t], (actives[t] if actives is not None else None)
        if f is True:
            out.append(0)
        else:
            drop = {b for b in range(3) if isinstance(f, list) and f[b]} | {b for b in range(3) if a is not None and not a[b]}
            out.append(sum(prev[b] for b in range(3) if b not in drop))
        prev = res[t][2]
    return out


def split_step(tf, rows1, rows2):
    """First step whose TemporalNet takes different paths in the two runs (len when none): from there the comparison is bounded."""
    for t, (n1, n2) in enumerate(zip(rows1, rows2)):
        if tf and (n1 >= TN_SWITCH_ROWS) != (n2 >= TN_SWITCH_ROWS):
            return t
    return len(rows1)


def matches(r1, r2, b, t, split):
    return same_slot(r1, r2, b) if t < split else close_slot(r1, r2, b)


def check_isolation(net, graph, depth):
    xs = batches(videos(), SLOTS, channels_last=graph)
    f_ref, f_rst = [True] + [False] * (T - 1), [t in (0, 4) for t in range(T)]
    stag = drive(net, xs, STAG_FIRST, STAG_ACTIVE, graph, depth)
    ref = drive(net, xs, f_ref, None, graph, depth)
    rst = drive(net, xs, f_rst, None, graph, depth)
    tf, n_stag = net.cfg.temporal_fusion_module, shift_rows(stag, STAG_FIRST, STAG_ACTIVE)
    s_ref, s_rst = split_step(tf, n_stag, shift_rows(ref, f_ref, None)), split_step(tf, n_stag, shift_rows(rst, f_rst, None))
    for t in range(T):
        assert matches(stag[t], ref[t], 1, t, s_ref), ("slot 1", t, s_ref)
        if t < 4:
            assert matches(stag[t], ref[t], 0, t, s_ref), ("slot 0 before its reset", t, s_ref)
        else:
            assert matches(stag[t], rst[t], 0, t, s_rst), ("slot 0 after its reset", t, s_rst)
            assert matches(stag[t], rst[t], 2, t, s_rst), ("slot 2 after its start", t, s_rst)
        if t < 2:
            assert matches(stag[t], ref[t], 2, t, s_ref), ("slot 2 before idling", t)
        elif t < 4:
            y, d, n = stag[t]
            assert not y[2].any() and n[2] == 0 and empty(d[2]), ("idle slot 2 reports nothing", t)
    return stag


@pytest.mark.parametrize("name,tf", NETS, ids=IDS)
def test_staggered_isolation_and_reset_eager(name, tf):
    check_isolation(net_for(name, tf, planar="fp16x2"), False, 0)


@pytest.mark.parametrize("name,tf", NETS, ids=IDS)
def test_staggered_semantics_equal_module_path(name, tf):
    net = net_for(name, tf)
    stag = drive(net, batches(videos(), SLOTS), STAG_FIRST, STAG_ACTIVE)
    # semantics: every video against the module path on that video alone
    v = videos()
    refs = {k: run_clip(net, clip.cuda(), "cuda") for k, clip in v.items()}
    seen = 0
    for b in range(3):
        for t in range(T):
            s = SLOTS[b][t]
            if s is None:
                continue
            r, d = refs[s[0]][s[1]], stag[t][1][b]
            if r["box"].shape[0] == 0:
                assert empty(d), (b, t)
                continue
            assert torch.equal(d["box_ids"], r["box_ids"]) and torch.equal(d["class"], r["class"]), (b, t)
            if tf:   # tolerances of test_batched_pipeline_equals_per_clip_driver_on_gpu
                assert (d["box"] - r["box"]).abs().max() < 1e-4 and (d["mask"] - r["mask"]).abs().max() < 2e-5, (b, t)
            else:    # ... and of test_batched_pipeline_non_tf_equals_model_forward_and_reference
                assert (d["box"] - r["box"]).abs().max() < 1e-5 and (d["score"] - r["score"]).abs().max() < 1e-6, (b, t)
                assert torch.equal(d["mask"], r["mask"]), (b, t)
            seen += r["box"].shape[0]
    assert seen > 20


@pytest.mark.parametrize("name,tf", NETS, ids=IDS)
def test_staggered_isolation_graph_replay_with_lookahead(name, tf):
    """The same checks on the optimized inference graph, trunks replayed from HIP graphs, three batches of look-ahead."""
    net = net_for(name, tf, planar="fp16x2")
    check_isolation(net, True, 3)


@pytest.mark.parametrize("name,tf", NETS, ids=IDS)
def test_all_true_and_all_false_lists_equal_scalar_forms(name, tf):
    net = net_for(name, tf, planar="fp16x2")
    xs = batches(videos(), [SLOTS[1], SLOTS[1], SLOTS[1]], channels_last=True)
    a = drive(net, xs[:4], [True, False, False, True])
    b = drive(net, xs[:4], [[True] * 3, [False] * 3, torch.zeros(3, dtype=torch.bool), torch.ones(3, dtype=torch.bool)],
              [None, [True] * 3, None, torch.ones(3, dtype=torch.bool)])
    for t in range(4):
        assert all(same_slot(a[t], b[t], k) for k in range(3)) and a[t][2] == b[t][2], t


@pytest.mark.parametrize("name,tf", NETS, ids=IDS)
def test_short_videos_and_simultaneous_resets_match_each_video_alone(name, tf):
    """1-frame videos, videos shorter than the look-ahead depth, two slots resetting on one step -- graph replay with look-ahead 3 -- against
    each video alone through a scalar-reset pipeline on the same graph (B = 3, the video in every slot; ids and classes exact)."""
    net = net_for(name, tf, planar="fp16x2")
    v = {"P": synthetic.synthetic_clip(1, H, W, seed=21), "Q": synthetic.synthetic_clip(1, H, W, seed=22),
         "R": synthetic.synthetic_clip(4, H, W, seed=23), "S": synthetic.synthetic_clip(6, H, W, seed=24),
         "U": synthetic.synthetic_clip(2, H, W, seed=25), "V": synthetic.synthetic_clip(4, H, W, seed=26)}
    slots = [[("P", 0), ("Q", 0), ("R", 0), ("R", 1), ("R", 2), ("R", 3)],
             [("S", t) for t in range(6)],
             [("U", 0), ("U", 1), ("V", 0), ("V", 1), ("V", 2), ("V", 3)]]
    firsts = [True, [True, False, False], [True, False, True], [False] * 3, [False] * 3, [False] * 3]
    xs = batches(v, slots, channels_last=True)
    stag = drive(net, xs, firsts, None, True, 3)
    # reference per video: the video in all three slots of a scalar-reset pipeline (same batch size, same graph)
    for b in range(3):
        t = 0
        while t < 6:
            name_v, t0 = slots[b][t][0], t
            n = v[name_v].shape[0]
            one = [x.contiguous(memory_format=torch.channels_last) for x in
                   [torch.stack([v[name_v][k]] * 3).cuda() for k in range(n)]]
            ref = drive(net, one, [True] + [False] * (n - 1), None, True, 3)
            for k in range(n):
                d, r = stag[t0 + k][1][b], ref[k][1][0]
                if empty(r):
                    assert empty(d), (b, name_v, k)
                    continue
                assert torch.equal(d["box_ids"], r["box_ids"]) and torch.equal(d["class"], r["class"]), (b, name_v, k)
                assert (d["box"] - r["box"]).abs().max() < 1e-4 and (d["score"] - r["score"]).abs().max() < 1e-6, (b, name_v, k)
            t += n


@pytest.mark.parametrize("name,tf", NETS, ids=IDS)
def test_reset_on_a_step_without_detections(name, tf):
    """A reset step on which no clip detects anything (threshold above every score): the reset clip's rows are dropped all the same
    (the non-TF path returns early on D == 0), it holds nothing until it detects again, and from the next step on it equals a pipeline that
    starts there; the other clips equal a run without the reset."""
    net = net_for(name, tf, planar="fp16x2")
    xs = batches(videos(), [SLOTS[1], [("A", t % 4) for t in range(T)], [("C", t % 2) for t in range(T)]], channels_last=True)
    thr = net.cfg.eval_conf_thresh

    def run(firsts, start=0):
        pipe = BatchedClipPipeline(net, 3)
        res = [None] * start
        try:
            for t in range(start, 6):
                net.cfg.eval_conf_thresh = 2.0 if t == 3 else thr
                y = pipe.step(xs[t], is_first=firsts[t])
                res.append((y.clone(), pipe.detections(), list(pipe.prev_n), [list(x) for x in pipe.tracked]))
        finally:
            net.cfg.eval_conf_thresh = thr
        return res

    f_stag, f_ref, f_fresh = [True, False, False, [True, False, False], False, False], [True] + [False] * 5, [None] * 4 + [True, False]
    stag, ref, fresh = run(f_stag), run(f_ref), run(f_fresh, start=4)
    y, d, n, trk = stag[3]
    assert n[0] == 0 and trk[0] == [] and not y[0].any() and empty(d[0])
    n_stag = shift_rows(stag, f_stag, None)
    s_ref = split_step(tf, n_stag, shift_rows(ref, f_ref, None))
    s_fresh = 4 + split_step(tf, n_stag[4:], shift_rows(fresh[4:], [True, False], None))
    for t in range(6):
        assert matches(stag[t][:3], ref[t][:3], 1, t, s_ref) and matches(stag[t][:3], ref[t][:3], 2, t, s_ref), t
        if t < 3:
            assert matches(stag[t][:3], ref[t][:3], 0, t, s_ref), t
        elif t > 3:
            assert matches(stag[t][:3], fresh[t][:3], 0, t, s_fresh), t


def test_range_fallback_repeats_a_step_with_a_per_clip_reset():
    """test_fp16_plane_graph_out_of_range_falls_back_to_bf16x3 with slot 0 starting a new video on the overflowing step: the repeated step must
    start from the tracked set as it was before the drop, and the run must equal a bf16x3 pipeline from the start."""
    def make(planes):
        net = build("STMask_plus_resnet50_config", planar=planes)
        return net, BatchedClipPipeline(net, 2)

    clip = torch.stack([synthetic.synthetic_clip(4, H, W, seed=s) for s in (2, 7)]).cuda()
    clip[:, 2] *= 1e5
    frames = [clip[:, t].contiguous(memory_format=torch.channels_last) for t in range(4)]
    firsts = [True, False, [True, False], False]
    (net_a, a), (net_b, b) = make("fp16x2"), make("bf16x3")
    seen = 0
    for t in range(4):
        pa, pb = a.step(frames[t], is_first=firsts[t]), b.step(frames[t], is_first=firsts[t])
        assert a.fell_back == (t >= 2) and not b.fell_back
        assert a.prev_n == b.prev_n, t
        da, db = a.detections(), b.detections()
        for c in range(2):
            assert torch.equal(da[c]["box_ids"], db[c]["box_ids"]) and torch.equal(da[c]["class"], db[c]["class"]), (t, c)
            if da[c]["box"].numel():
                assert (da[c]["box"] - db[c]["box"]).abs().max() < 1e-4 and (da[c]["mask"] - db[c]["mask"]).abs().max() < 1e-3
                seen += da[c]["box"].shape[0]
        if t >= 2:
            assert torch.isfinite(pa).all()
    assert seen > 10 and net_a._planar_planes == "bf16x3"
