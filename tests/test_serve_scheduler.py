"""stmask_amd.serve.VideoBatcher without a GPU: a fake pipeline records what the driver hands it, pre-processing is the CPU oracle, and the
output stage is replaced by a stand-in that tags every object with its video, slot and frame.  Checks the FIFO slot assignment (per-step
is_first / active vectors), that the look-ahead batches are the very objects later passed as frames, and the record assembly."""
import pytest
import torch

import oracle
from stmask_amd import preprocess, serve


class FakePipe:
    def __init__(self, B, depth=2):
        self.B, self.prefetch_depth, self.use_graph = B, depth, False
        self.calls = []

    def step(self, frames, is_first=None, next_frames=None, active=None):
        self.calls.append({"frames": frames, "is_first": list(is_first), "active": list(active), "next": list(next_frames or [])})

    def detections(self):
        frames = self.calls[-1]["frames"]
        # one object per busy slot; its "class" carries the slot's first pixel (which video / frame the slot was fed)
        return [{"box": torch.zeros(1, 4), "score": torch.ones(1), "class": frames[b, 0, 0, 0].reshape(1), "box_ids": torch.zeros(1, dtype=torch.long)}
                for b in range(self.B)]


def cpu_prep(frames, frame_ids):
    out = torch.zeros(len(frames), 3, 384, 640)
    metas = [None] * len(frames)
    for b, f in enumerate(frames):
        if f is not None:
            out[b] = oracle.preprocess_frames(f[None], mode=0)[0]
            metas[b] = {"ori_shape": tuple(f.shape), "img_shape": (360, 640, 3), "pad_shape": (384, 640, 3), "frame_id": frame_ids[b]}
    return out, metas


def fake_post(det_output, meta):
    d = det_output["detection"]
    v = int(d["class"][0])
    return {"box": d["box"], "score": d["score"], "class": torch.tensor([v // 50 + 1]), "box_ids": d["box_ids"],
            "segm": [{"size": list(meta["ori_shape"][:2]), "counts": "v%d_f%d" % (v // 50, meta["frame_id"])}]}


def make_videos(lengths):
    vids = []
    for i, T in enumerate(lengths):
        h, w = (36, 64) if i % 2 else (45, 80)
        # constant frames, pixel value 50 * video + frame: the mode-0 resize keeps a constant image exact
        f = torch.stack([torch.full((h, w, 3), 50 * i + t, dtype=torch.uint8) for t in range(T)])
        vids.append(("vid%02d" % (len(lengths) - i), f))    # ids in reverse queue order: records must come back sorted by id
    return vids


@pytest.mark.parametrize("lengths,slots", [([3, 7, 1, 5, 4], 2), ([3, 7, 1, 5, 4], 8)])
def test_schedule_is_fifo_per_slot(lengths, slots):
    plan = serve.schedule(lengths, slots)
    seen = {}
    for s, row in enumerate(plan):
        assert len(row) == slots
        for b, c in enumerate(row):
            if c is None:
                continue
            v, f = c
            seen.setdefault(v, []).append((s, b, f))
    for v, T in enumerate(lengths):
        steps = seen[v]
        assert [f for _, _, f in steps] == list(range(T))                           # every frame once, in order
        assert len({b for _, b, _ in steps}) == 1                                   # one slot per video
        assert [s for s, _, _ in steps] == list(range(steps[0][0], steps[0][0] + T))  # consecutive steps
    starts = [seen[v][0][0] for v in range(len(lengths))]
    assert starts == sorted(starts)                                                 # FIFO
    if slots == 2:
        # slot 0: v0 (3) then v2 (1) then v3 (5); slot 1: v1 (7) then v4 (4)
        assert [[None if c is None else c[0] for c in row] for row in plan] == \
            [[0, 1]] * 3 + [[2, 1]] + [[3, 1]] * 3 + [[3, 4]] * 2 + [[None, 4]] * 2
    else:
        assert len(plan) == max(lengths) and all(plan[0][b] == (b, 0) for b in range(5)) and all(c is None for c in plan[0][5:])


@pytest.mark.parametrize("slots,depth", [(2, 2), (8, 3), (2, 0)])
def test_video_batcher_drives_pipeline(monkeypatch, slots, depth):
    lengths = [3, 7, 1, 5, 4]
    vids = make_videos(lengths)
    monkeypatch.setattr(serve.output_utils, "postprocess_ytbvis", fake_post)
    pipe = FakePipe(slots, depth)
    vb = serve.VideoBatcher(None, slots, prep=cpu_prep, pipeline=pipe, classes=["c%d" % i for i in range(1, 10)])
    records = vb.run(vids)
    plan = serve.schedule(lengths, slots)
    assert len(pipe.calls) == len(plan)
    for s, (call, row) in enumerate(zip(pipe.calls, plan)):
        assert call["is_first"] == [c is not None and c[1] == 0 for c in row]
        assert call["active"] == [c is not None for c in row]
        for b, c in enumerate(row):
            px = call["frames"][b, 0, 0, 0].item()
            assert px == (0.0 if c is None else 50 * c[0] + c[1])                 # the slot's frame, or zeros when idle
        # the look-ahead batches are the very tensors the next steps get as frames
        assert len(call["next"]) == min(depth, len(plan) - 1 - s)
        for k, nf in enumerate(call["next"]):
            assert nf is pipe.calls[s + 1 + k]["frames"]
    assert vb.occupancy() == pytest.approx(sum(lengths) / (len(plan) * slots))
    # one record per video (one object each), sorted by video id, every frame of the video present with its own frame id
    assert [r["video_id"] for r in records] == sorted(v for v, _ in vids)
    by_id = {v: i for i, (v, _) in enumerate(vids)}
    for r in records:
        i = by_id[r["video_id"]]
        assert r["category_id"] == i + 1
        assert [s["counts"] for s in r["segmentations"]] == ["v%d_f%d" % (i, t) for t in range(lengths[i])]
        assert all(s["size"] == list(vids[i][1].shape[1:3]) for s in r["segmentations"])


def test_schedule_rejects_empty_videos():
    with pytest.raises(ValueError):
        serve.schedule([3, 0], 2)


def test_multi_preprocess_meta_without_gpu_is_an_error():
    """No CPU fallback: the device pre-processing refuses host tensors."""
    from stmask_amd.ops import StmError
    with pytest.raises(StmError):
        preprocess.preprocess_eval_frames_multi([torch.zeros(36, 64, 3, dtype=torch.uint8)], [0])
