"""The host half of the batched output stage without a GPU: output_utils.unpack_step_buffer on hand-built step buffers (the layout of
include/stmask_hip_output.h), and VideoBatcher(batched_output=True) with stand-ins for the pipeline, the pre-processing and the output stage."""
import ctypes

import numpy as np
import pytest
import torch

from stmask_amd import _lib, eval_utils, output_utils, serve
from test_serve_scheduler import FakePipe, cpu_prep, fake_post, make_videos

CLASSES = ["c%d" % i for i in range(1, 10)]


def step_buffer(rows, arena_slack=0):
    """rows: dicts with frame, status, cls, box_id, score, box and (kept rows with a string) counts -> the bytes the device would have written:
    the strings compact and in row order."""
    table, arena = [], b""
    for r in rows:
        s = r.get("counts", b"")
        rec = _lib.OutputRow(r["frame"], r["status"], r.get("n_runs", 1 if s else 0), len(arena), len(s), r["cls"], r["box_id"],
                             int(np.float32(r["score"]).view(np.uint32)), (ctypes.c_int * 4)(*r["box"]))
        table.append(bytes(rec))
        arena += s
    head = bytes(_lib.OutputHeader(len(rows), len(arena), len(arena) + arena_slack, 0))
    return np.frombuffer(head + b"".join(table) + arena + b"\xff" * arena_slack, dtype=np.uint8)


def meta(video, frame, h=36, w=64):
    return {"ori_shape": (h, w, 3), "img_shape": (360, 640, 3), "pad_shape": (384, 640, 3), "video_id": video, "frame_id": frame}


def row(frame, box_id, cls, score, box, counts, status=_lib.ROW_KEPT):
    return {"frame": frame, "status": status, "cls": cls, "box_id": box_id, "score": score, "box": box, "counts": counts}


def same_record(got, want):
    """Keys in the same order; every value of the same type and value."""
    assert list(got) == list(want)
    for (kg, g), (kw, w) in zip(got.items(), want.items()):
        assert type(kg) is type(kw) and kg == kw
        if not isinstance(w, dict):
            assert g == w
            continue
        assert list(g) == list(w) == ["bbox", "score", "segm", "label", "category"]
        assert type(g["bbox"]) is type(w["bbox"]) and g["bbox"].dtype == w["bbox"].dtype == np.int64 and g["bbox"].tolist() == w["bbox"].tolist()
        assert type(g["score"]) is type(w["score"]) is np.float32 and g["score"] == w["score"]
        assert type(g["label"]) is type(w["label"]) and g["label"] == w["label"]
        assert g["category"] == w["category"] and g["segm"] == w["segm"]
        assert type(g["segm"]["counts"]) is bytes and type(g["segm"]["size"]) is list


def reference_record(rows, frame, m):
    """bbox2result_with_id on the kept rows of one frame, as postprocess_ytbvis would hand them on."""
    mine = [r for r in rows if r["frame"] == frame and r["status"] & _lib.ROW_KEPT]
    preds = {"box": torch.tensor([r["box"] for r in mine], dtype=torch.int64).reshape(-1, 4), "score": torch.tensor([r["score"] for r in mine]),
             "box_ids": torch.tensor([r["box_id"] for r in mine], dtype=torch.int64), "class": torch.tensor([r["cls"] for r in mine], dtype=torch.int64),
             "segm": [{"size": list(m["ori_shape"][:2]), "counts": r["counts"]} for r in mine]}
    return eval_utils.bbox2result_with_id(preds, m, CLASSES)


def test_unpack_frame_without_rows_and_idle_frame():
    metas = [meta("a", 0), None, meta("b", 3)]
    rows = [row(0, 0, 2, 0.5, [1, 2, 3, 4], b"0X")]
    out = output_utils.unpack_step_buffer(step_buffer(rows), metas, CLASSES)
    assert out[1] is None
    assert out[2] == {"video_id": "b", "frame_id": 3}
    same_record(out[0], reference_record(rows, 0, metas[0]))
    # no rows at all: an empty header, and no bytes
    for buf in (step_buffer([]), np.zeros(0, dtype=np.uint8)):
        assert output_utils.unpack_step_buffer(buf, metas, CLASSES) == [{"video_id": "a", "frame_id": 0}, None, {"video_id": "b", "frame_id": 3}]


def test_unpack_frame_whose_rows_are_all_rejected():
    metas = [meta("a", 0), meta("b", 1)]
    rows = [row(0, 0, 1, 0.9, [0, 0, 0, 0], b"", status=0), row(1, 0, 3, 0.25, [5, 6, 70, 80], b"12345"), row(0, 1, 1, 0.8, [0, 0, 0, 0], b"", status=0)]
    out = output_utils.unpack_step_buffer(step_buffer(rows), metas, CLASSES)
    assert out[0] == {"video_id": "a", "frame_id": 0}
    same_record(out[1], reference_record(rows, 1, metas[1]))


def test_unpack_interleaved_frames_types_and_key_order():
    metas = [meta("a", 4), meta("b", 0, 45, 80)]
    rows = [row(1, 3, 2, 0.75, [0, 1, 80, 45], b"abc"), row(0, 0, 1, 0.125, [1, 2, 3, 4], b"0"), row(1, 0, 9, 1.0, [7, 7, 9, 9], b"PPQQ"),
            row(0, 5, 4, 0.3, [0, 0, 64, 36], b""), row(1, -1, 2, 0.5, [1, 1, 2, 2], b"zz"), row(0, 2, 1, 0.1, [3, 3, 4, 4], b"XYZ")]
    out = output_utils.unpack_step_buffer(step_buffer(rows, arena_slack=7), metas, CLASSES)
    for f in (0, 1):
        same_record(out[f], reference_record(rows, f, metas[f]))
    assert list(out[1])[2:] == [3, 0] and list(out[0])[2:] == [0, 5, 2]           # a frame's objects in row order; the id -1 row is dropped
    assert out[1][3]["segm"] == {"size": [45, 80], "counts": b"abc"} and out[0][5]["segm"]["counts"] == b""


def test_unpack_run_overflow_calls_the_hook_for_that_row_only():
    metas = [meta("a", 0), meta("b", 1)]
    rows = [row(0, 0, 1, 0.5, [1, 2, 3, 4], b"first"), row(1, 1, 2, 0.5, [1, 2, 3, 4], b"", status=_lib.ROW_KEPT | _lib.ROW_RUN_OVERFLOW),
            row(1, 2, 2, 0.5, [1, 2, 3, 4], b"third"), row(0, 3, 2, 0.5, [1, 2, 3, 4], b"", status=_lib.ROW_RUN_OVERFLOW)]
    calls = []

    def hook(r, f):
        calls.append((r, f))
        return {"size": [36, 64], "counts": b"redone"}

    out = output_utils.unpack_step_buffer(step_buffer(rows), metas, CLASSES, reencode=hook)
    assert calls == [(1, 1)]                                                        # not the rejected row 3, whatever its other bits say
    assert out[1][1]["segm"]["counts"] == b"redone" and out[1][2]["segm"]["counts"] == b"third" and out[0][0]["segm"]["counts"] == b"first"
    assert list(out[0]) == ["video_id", "frame_id", 0]
    with pytest.raises(_lib.StmError):
        output_utils.unpack_step_buffer(step_buffer(rows), metas, CLASSES)         # no hook: an error, not a missing mask


def test_unpack_refuses_records_it_cannot_serve():
    metas = [meta("a", 0)]
    with pytest.raises(_lib.StmError):
        output_utils.unpack_step_buffer(step_buffer([row(0, 0, 1, 0.5, [0, 0, 1, 1], b"", status=_lib.ROW_KEPT | _lib.ROW_ARENA_OVERFLOW)]), metas, CLASSES)
    with pytest.raises(_lib.StmError):
        output_utils.unpack_step_buffer(step_buffer([row(1, 0, 1, 0.5, [0, 0, 1, 1], b"x")]), metas, CLASSES)          # frame 1 of 1
    with pytest.raises(_lib.StmError):
        output_utils.unpack_step_buffer(step_buffer([row(0, 0, 1, 0.5, [0, 0, 1, 1], b"abcdef")])[:-3], metas, CLASSES)   # arena cut short


def test_frame_geometry_is_select_rows():
    m = {"ori_shape": (480, 854, 3), "img_shape": (360, 640, 3), "pad_shape": (384, 640, 3)}
    det = {"box": torch.zeros(0, 4), "mask": torch.zeros(0, 96, 160)}
    _, crop_h, crop_w, out_h, out_w = output_utils.select_rows(det, m)
    assert output_utils.frame_geometry(m, 96, 160) == (crop_h, crop_w, out_h, out_w, 640 / 640, 360 / 384)


class RowsPipe(FakePipe):
    def tracked_rows(self):
        return {"step": len(self.calls) - 1, "dets": self.detections()}


class StandInStage:
    """The per-frame stand-in path of test_serve_scheduler.py behind the submit / collect interface."""

    def __init__(self):
        self.submitted, self.collected, self.outstanding = 0, [], 0

    def submit(self, rows, metas):
        ticket = {"k": self.submitted, "rows": rows, "metas": list(metas)}
        assert rows["step"] == self.submitted
        self.submitted += 1
        self.outstanding += 1
        assert self.outstanding <= 2                                               # two pinned buffers
        return ticket

    def collect(self, ticket):
        self.collected.append(ticket["k"])
        self.outstanding -= 1
        return [None if m is None else eval_utils.bbox2result_with_id(fake_post({"detection": d}, m), m, CLASSES)
                for d, m in zip(ticket["rows"]["dets"], ticket["metas"])]


@pytest.mark.parametrize("lengths,slots,depth", [([3, 7, 1, 5, 4], 2, 2), ([3, 7, 1, 5, 4], 8, 3), ([2, 1, 4, 1, 1, 3], 3, 0), ([1], 2, 1)])
def test_video_batcher_batched_output_equals_per_frame_path(monkeypatch, lengths, slots, depth):
    vids = make_videos(lengths)
    monkeypatch.setattr(serve.output_utils, "postprocess_ytbvis", fake_post)
    want = serve.VideoBatcher(None, slots, prep=cpu_prep, pipeline=FakePipe(slots, depth), classes=CLASSES).run(vids)
    stage = StandInStage()
    vb = serve.VideoBatcher(None, slots, prep=cpu_prep, pipeline=RowsPipe(slots, depth), classes=CLASSES, batched_output=True, output_stage=stage)
    got = vb.run(vids)
    assert got == want and len(got) == len(lengths)
    n_steps = len(serve.schedule(lengths, slots))
    assert stage.submitted == n_steps and stage.collected == list(range(n_steps))   # every ticket once, in step order, the last one too
    assert vb.occupancy() == pytest.approx(sum(lengths) / (n_steps * slots))


def test_video_batcher_default_is_the_per_frame_path():
    vb = serve.VideoBatcher(None, 2, prep=cpu_prep, pipeline=FakePipe(2), classes=CLASSES)
    assert vb.batched_output is False and vb.output_stage is None
