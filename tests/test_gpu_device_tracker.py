"""BatchedClipPipeline(device_tracker=True) on the MI355X: the tracker's greedy resolution and per-clip drop plan as kernels
(csrc/track_resolve.hip, include/stmask_hip_tracker.h), and the pipeline mode that keeps the counters and row offsets on the device.

* the kernels against the host functions they replace (track_host.match_tf / keep_rows / clip_offsets, themselves held to the reference's
  goldens): plans, offsets, counters and the zero padding exactly, on clips whose rows and detections both exceed one 256-thread pass;
* mode against mode: a host-mode and a device-mode pipeline on one net over a staggered schedule (per-clip resets, an idle slot, a step
  without detections), with and without max_instances -- packed output, detections(), prev_n, tracked, every state row tensor and the bit
  words equal after every step; eager and under graph replay with look-ahead; through a range fallback;
* device mode builds no per-row host structure: it runs with track_host.match_tf / keep_rows replaced by functions that raise;
* tracked_rows() never waits and never reports a padding row; VideoBatcher's batched output stage yields the default pipeline's records."""
import random

import pytest
import torch

import test_gpu_staggered_clips as sc
from stmask_amd import ops, synthetic, track_host
from stmask_amd.pipeline import BatchedClipPipeline
from test_gpu_parity import build

pytestmark = pytest.mark.gpu

H, W, T = sc.H, sc.W, 8


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
def resolve_case(prev_n, counts, seed, p_new=0.4, null_match=False):
    """Host lists of one step: several detections hit one row (a clip of 5 rows takes 260 detections), scores are multiples of 1/8 so that
    equal scores meet on one row, counters in 0..15."""
    rng = random.Random(seed)
    off = track_host.clip_offsets(prev_n)
    ids, scores = [], []
    for b, n in enumerate(counts):
        for _ in range(n):
            new = null_match or prev_n[b] == 0 or rng.random() < p_new
            ids.append(0 if new else 1 + off[b] + rng.randrange(prev_n[b]))
            scores.append(rng.randint(1, 8) / 8.0)
    tracked = [[rng.randint(0, 15) for _ in range(n)] for n in prev_n]
    return ids, scores, tracked


def run_resolve(prev_n, counts, ids, scores, tracked, cap, null_match=False):
    Pn, D = sum(prev_n), sum(counts)
    i32 = dict(dtype=torch.int32, device="cuda")
    match = None if null_match else torch.tensor(ids, **i32)
    tm = torch.tensor([v for t in tracked for v in t], **i32) if Pn else None
    return ops.track_resolve_tf(match, torch.tensor(scores, device="cuda"), torch.tensor(counts, **i32),
                                torch.tensor(track_host.clip_offsets(prev_n), **i32), tm, Pn, D, cap)


def check_resolve(prev_n, counts, seed, cap, p_new=0.4, null_match=False):
    ids, scores, tracked = resolve_case(prev_n, counts, seed, p_new, null_match)
    want_plan, want_n, want_tm = track_host.match_tf(prev_n, tracked, counts, ids, scores, cap)
    plan, new_off, new_tm = run_resolve(prev_n, counts, ids, scores, tracked, cap, null_match)
    again = run_resolve(prev_n, counts, ids, scores, tracked, cap, null_match)
    R, total = len(want_plan), sum(prev_n) + sum(counts)
    assert plan.shape[0] == new_tm.shape[0] == total
    assert new_off.tolist() == track_host.clip_offsets(want_n)
    assert plan.tolist() == want_plan + [0] * (total - R)                 # the padding names row 0
    assert new_tm.tolist() == [v for t in want_tm for v in t] + [0] * (total - R)
    assert all(torch.equal(x, y) for x, y in zip((plan, new_off, new_tm), again))
    return want_n, ids


PREV_N, COUNTS = [0, 3, 300, 5], [4, 0, 70, 260]


@pytest.mark.parametrize("cap", [0, 4, 301])
def test_resolve_kernel_equals_match_tf(cap):
    want_n, ids = check_resolve(PREV_N, COUNTS, 1, cap)
    off = track_host.clip_offsets(COUNTS)
    hit = [i for i in ids[off[3]:off[4]] if i]
    assert len(hit) > 5 * len(set(hit)) and 0 in ids[off[2]:off[3]]      # several detections per row; unmatched ones beside them
    if cap == 0:
        assert want_n[2] > 300 and want_n[3] > 5
    elif cap == 4:
        assert want_n == [4, 3, 300, 5]                                   # a clip at or over the cap opens no track
    else:
        assert want_n[2] == 301 and want_n[3] > 5


@pytest.mark.parametrize("variant", ["null_match", "all_matched", "one_clip"])
def test_resolve_kernel_variants(variant):
    if variant == "null_match":
        for cap in (0, 4, 301):
            want_n, _ = check_resolve(PREV_N, COUNTS, 2, cap, null_match=True)
            assert cap or want_n == [p + c for p, c in zip(PREV_N, COUNTS)]
    elif variant == "all_matched":
        prev_n = [2, 3, 300, 5]
        want_n, ids = check_resolve(prev_n, COUNTS, 3, 0, p_new=0.0)
        assert want_n == prev_n and all(ids)
    else:
        for cap in (0, 8):
            check_resolve([7], [9], 4, cap)
        check_resolve([0], [300], 5, 0)
        check_resolve([300], [0], 6, 0)


@pytest.mark.parametrize("gone", [(), (0,), (2,), (1, 3), (0, 1, 2, 3)], ids=["none", "c0", "c2", "c1_c3", "all"])
def test_drop_plan_kernel_equals_keep_rows(gone):
    i32 = dict(dtype=torch.int32, device="cuda")
    want = track_host.keep_rows(PREV_N, set(gone))
    left = [0 if b in gone else n for b, n in enumerate(PREV_N)]
    keep, new_off = ops.track_drop_plan(torch.tensor(track_host.clip_offsets(PREV_N), **i32), torch.tensor([int(b in gone) for b in range(4)], **i32),
                                        len(want))
    assert keep.tolist() == want and new_off.tolist() == track_host.clip_offsets(left)


# ---- mode against mode ---------------------------------------------------------------------------------------------------------------------
# slot 0: video A (3 frames), then A2 from t = 3; slot 1: B throughout; slot 2: C (2 frames), idle at t = 2..3, C2 from t = 4; at t = 6 every
# slot gets a frame of zeros: a step without detections
SLOTS = [[("A", t) if t < 3 else ("A2", t - 3) for t in range(T)],
         [("B", t) for t in range(T)],
         [("C", t) if t < 2 else (None if t < 4 else ("C2", t - 4)) for t in range(T)]]
FIRST = [True, [False] * 3, [False] * 3, [True, False, False], [False, False, True], [False] * 3, [False] * 3, [False] * 3]
ACTIVE = [None, None, [True, True, False], [True, True, False], None, None, None, None]
ZERO_STEP = 6
_batches = {}
_host_runs = {}


def frame_batches(channels_last):
    if channels_last not in _batches:
        v = {"A": synthetic.synthetic_clip(3, H, W, seed=0), "A2": synthetic.synthetic_clip(5, H, W, seed=3),
             "B": synthetic.synthetic_clip(T, H, W, seed=5), "C": synthetic.synthetic_clip(2, H, W, seed=9),
             "C2": synthetic.synthetic_clip(4, H, W, seed=11)}
        xs = sc.batches(v, SLOTS, channels_last=channels_last)
        xs[ZERO_STEP] = torch.zeros_like(xs[ZERO_STEP])
        _batches[channels_last] = xs
    return _batches[channels_last]


def net():
    return sc.net_for("STMask_plus_resnet50_config", True, planar="fp16x2")


def state_of(pipe):
    prev = pipe.prev
    rows = {} if prev is None else {k: v.clone() for k, v in prev.items()}
    return rows, None if pipe._bits is None else pipe._bits.clone()


def drive(device_tracker, cap, graph=False, depth=0, light=False):
    """-> per step (packed output, detections(), prev_n, tracked, state rows, bit words); light: the packed output and prev_n alone, so that
    the soft masks of the tracked set stay deferred from step to step (nothing reads them), and the full record after the last step."""
    xs = frame_batches(graph)
    pipe = BatchedClipPipeline(net(), 3, device_tracker=device_tracker)
    assert pipe.device_tracker == device_tracker
    pipe.use_graph, pipe.max_instances = graph, cap
    res = []
    for t, x in enumerate(xs):
        nxt = xs[t + 1:t + 1 + depth] if depth else None
        y = pipe.step(x, is_first=FIRST[t], next_frames=nxt or None, active=ACTIVE[t])
        if light and t < T - 1:
            res.append((y.clone(), None, list(pipe.prev_n), None, None, None))
        else:
            res.append((y.clone(), pipe.detections(), list(pipe.prev_n), [list(v) for v in pipe.tracked]) + state_of(pipe))
    torch.cuda.synchronize()
    assert pipe.graph_active == graph and not pipe.fell_back
    return res


def host_run(cap, graph=False, depth=0, light=False):
    key = (cap, graph, depth, light)
    if key not in _host_runs:
        _host_runs[key] = drive(False, cap, graph, depth, light)
    return _host_runs[key]


def same_bits(a, b):
    """torch.equal on the bit patterns: state rows that are not reported may hold NaN (a frame scaled out of range), equal to itself here."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def same_dets(d1, d2):
    assert len(d1) == len(d2)
    for a, b in zip(d1, d2):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


def assert_same_run(host, dev, cap):
    seen = 0
    for t, (h, d) in enumerate(zip(host, dev)):
        assert torch.equal(h[0], d[0]), ("packed", t)
        assert h[2] == d[2], ("prev_n", t, h[2], d[2])
        if h[1] is None:
            continue
        same_dets(h[1], d[1])
        assert h[3] == d[3], ("tracked", t)
        assert h[4].keys() == d[4].keys(), t
        for k in h[4]:
            assert h[4][k].shape[0] == sum(h[2]) and same_bits(h[4][k], d[4][k]), ("state", t, k)
        assert (h[5] is None) == (d[5] is None) and (h[5] is None or torch.equal(h[5][:sum(h[2])], d[5][:sum(h[2])])), ("bits", t)
        seen += sum(x["box"].shape[0] for x in h[1] if x)
        if cap:
            assert max(h[2]) <= cap
    # the scenario is what it says: clips held rows, the idle slot and the reset slots held none, the zero step detected nothing
    full = [h for h in host if h[3] is not None]
    assert seen > (10 if len(full) == len(host) else 0) and all(h[2][2] == 0 for h in host[2:4])
    if len(full) == len(host):
        before, after = host[ZERO_STEP - 1], host[ZERO_STEP]
        assert after[2] == before[2] and sum(after[2]) > 0 and after[3] == [[v + 1 for v in c] for c in before[3]]


@pytest.mark.parametrize("cap", [0, 5], ids=["uncapped", "max_instances_5"])
def test_device_mode_equals_host_mode_eager(cap):
    assert_same_run(host_run(cap), drive(True, cap), cap)


@pytest.mark.parametrize("cap", [0, 5], ids=["uncapped", "max_instances_5"])
def test_device_mode_equals_host_mode_graph_replay_with_lookahead(cap):
    assert_same_run(host_run(cap, True, 3), drive(True, cap, True, 3), cap)
    # ... and with nothing reading the soft masks between the steps: the deferred mask gather stays deferred through the drops
    assert_same_run(host_run(cap, True, 3, True), drive(True, cap, True, 3, True), cap)


@pytest.mark.parametrize("cap", [0, 5], ids=["uncapped", "max_instances_5"])
def test_device_mode_builds_no_per_row_host_structure(cap, monkeypatch):
    host = host_run(cap)

    def boom(*a, **k):
        raise AssertionError("device_tracker called a per-row host function")

    monkeypatch.setattr(track_host, "match_tf", boom)
    monkeypatch.setattr(track_host, "keep_rows", boom)
    assert_same_run(host, drive(True, cap), cap)
    with pytest.raises(AssertionError):                  # (the patch bites: host mode does call them)
        drive(False, cap)


def test_device_tracker_needs_temporal_fusion():
    with pytest.raises(ValueError):
        BatchedClipPipeline(sc.net_for("STMask_plus_resnet50_config", False), 3, device_tracker=True)


def test_range_fallback_repeats_a_step_with_a_per_clip_reset_in_device_mode():
    """The scenario of test_gpu_staggered_clips.test_range_fallback_repeats_a_step_with_a_per_clip_reset, device mode beside host mode: both fall
    back on the overflowing step (slot 0 starts a new video on it) and stay equal in everything."""
    def make(device_tracker):
        n = build("STMask_plus_resnet50_config", planar="fp16x2")
        return n, BatchedClipPipeline(n, 2, device_tracker=device_tracker)

    clip = torch.stack([synthetic.synthetic_clip(4, H, W, seed=s) for s in (2, 7)]).cuda()
    clip[:, 2] *= 1e5
    frames = [clip[:, t].contiguous(memory_format=torch.channels_last) for t in range(4)]
    firsts = [True, False, [True, False], False]
    (net_a, a), (net_b, b) = make(True), make(False)
    seen = 0
    for t in range(4):
        pa, pb = a.step(frames[t], is_first=firsts[t]), b.step(frames[t], is_first=firsts[t])
        assert a.fell_back == b.fell_back == (t >= 2)
        assert torch.equal(pa, pb) and torch.isfinite(pa).all(), t
        assert a.prev_n == b.prev_n and a.tracked == b.tracked, t
        same_dets(a.detections(), b.detections())
        (ra, ba), (rb, bb) = state_of(a), state_of(b)
        assert ra.keys() == rb.keys() and torch.equal(ba, bb), t
        for k in ra:
            assert same_bits(ra[k], rb[k]), (t, k, int((ra[k] != rb[k]).sum()), int(torch.isnan(ra[k].float()).sum()))
        seen += sum(d["box"].shape[0] for d in a.detections() if d)
    assert seen > 10 and net_a._planar_planes == net_b._planar_planes == "bf16x3"


# ---- tracked_rows() and the batched output stage -------------------------------------------------------------------------------------------
def test_tracked_rows_never_report_a_padding_row():
    xs = frame_batches(False)
    host, dev = BatchedClipPipeline(net(), 3), BatchedClipPipeline(net(), 3, device_tracker=True)
    padded = kept = 0
    for t, x in enumerate(xs):
        for p in (host, dev):
            p.step(x, is_first=FIRST[t], active=ACTIVE[t])
        unsettled = dev._unsettled is not None
        rd, rh = dev.tracked_rows(), host.tracked_rows()
        assert (dev._unsettled is not None) == unsettled                 # tracked_rows() did not settle, i.e. did not wait
        if rh is None:
            assert rd is None or not rd["keep"].any(), t
            continue
        n_dev = rd["keep"].shape[0]
        assert all(rd[k].shape[0] == n_dev for k in rd)
        padded += n_dev > sum(dev.prev_n)                                # (reading prev_n settles: after the rows were taken)
        kd, kh = rd["keep"], rh["keep"]
        for k in ("mask", "box", "score", "class", "frame", "box_id"):
            assert torch.equal(rd[k][kd], rh[k][kh]), (t, k)
        kept += int(kh.sum())
    assert padded >= 2 and kept > 10                                     # steps whose capacity exceeded their row count were among them


def test_video_batcher_batched_output_on_a_device_mode_pipeline():
    from scripts.run_video_demo import synthetic_video_u8
    from stmask_amd.serve import VideoBatcher
    from test_gpu_serve import demo_net
    n = demo_net()
    vids = [(50 - i, synthetic_video_u8(1, T_, *((720, 1280) if i % 2 == 0 else (480, 854)), seed=60 + i)[0].cuda()) for i, T_ in enumerate([2, 4, 1, 2])]
    want = VideoBatcher(n, 3, batched_output=True).run(vids)
    got = VideoBatcher(n, 3, batched_output=True, pipeline=BatchedClipPipeline(n, 3, device_tracker=True)).run(vids)
    assert len(want) > 3 and got == want
