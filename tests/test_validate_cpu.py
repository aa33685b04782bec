"""Validation during training without a GPU: the numpy restatement of fuse._fold against torch, InferenceTwin(fold="torch") on a CPU net against
a freshly optimised copy, datasets.YTVISValSet / LazyVideo, the validation() driver with an injected batcher and scorer, the new arguments of
scripts/train_ytvis.py, and the package-private binding of csrc/fold.h."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import abi_header
import fold_restate as R
from kernel_resources import kernel_resources
from validate_helpers import LENGTHS, SIZES, Reader, differing, fresh_copy, full_state, perturb, rng_states, same_rng, same_snapshot, snapshot, val_ann
from stmask_amd import _lib, datasets, eval_utils, fuse, synthetic, validate
from stmask_amd._lib import StmError
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask



# ---- the restatement against fuse._fold on CPU convolutions ------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 3), (64, 32, 1), (7, 3, 3)])
def test_restatement_is_torchs_fold_bit_for_bit(shape, with_bias, eps):
    """running_var = 0, a negative gamma, a variance of +inf and one of NaN are among the channels (fold_restate.seeded_bn)."""
    O, C, k = shape
    gamma, beta, mean, var = R.seeded_bn(O, seed=O * 31 + C, nonfinite=True)
    g = np.random.default_rng(5)
    w = g.normal(0, 0.2, (O, C, k, k)).astype(np.float32)
    b = g.normal(0, 0.2, O).astype(np.float32) if with_bias else None
    conv = nn.Conv2d(C, O, k, bias=with_bias)
    bn = nn.BatchNorm2d(O, eps=eps)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
        if with_bias:
            conv.bias.copy_(torch.from_numpy(b))
        for t, v in ((bn.weight, gamma), (bn.bias, beta), (bn.running_mean, mean), (bn.running_var, var)):
            t.copy_(torch.from_numpy(v))
    fuse._fold(conv, bn)
    assert np.array_equal(R.bits(conv.weight.detach().numpy()), R.bits(R.fold_weight(w, gamma, var, eps)))
    assert np.array_equal(R.bits(conv.bias.detach().numpy()), R.bits(R.fold_bias(b, gamma, beta, mean, var, eps)))
    if O >= 3:
        assert np.isnan(conv.weight[2].detach().numpy()).all() and (conv.weight[1] == 0).all()      # the non-finite variances did travel


# ---- the twin on a CPU net ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def live_and_twin():
    net = STMask(get_cfg("STMask_plus_resnet50_config"))
    synthetic.fill_state_dict(net, seed=0)
    net.train()
    return net, validate.InferenceTwin(net, fold="torch")


def test_twin_refresh_equals_a_freshly_optimised_copy(live_and_twin):
    net, twin = live_and_twin
    gen = twin.generation
    assert not twin.planar and not twin.net.training and net.training
    kinds = [s.kind for s in twin.sources]
    assert kinds.count(validate.WEIGHT) == kinds.count(validate.BIAS) == 53 and kinds.count(validate.BIAS3) == 16
    perturb(net, seed=3)
    before = snapshot(net)
    ptrs = {k: v.data_ptr() for k, v in twin.net.state_dict(keep_vars=True).items()}
    stale = full_state(twin.net)
    twin.refresh()
    assert twin.generation == gen + 1
    got, want = full_state(twin.net), full_state(fresh_copy(net))
    assert any(k.endswith("bias3") for k in got) and differing(got, want) == []
    assert not torch.equal(got["backbone.conv1.weight"], stale["backbone.conv1.weight"])          # the refresh did write
    assert same_snapshot(before, snapshot(net))                                                     # the live net is as it was
    assert ptrs == {k: v.data_ptr() for k, v in twin.net.state_dict(keep_vars=True).items()}      # in place: no parameter was reallocated
    twin.refresh()
    again = full_state(twin.net)
    assert differing(got, again) == [] and twin.generation == gen + 2


def test_a_twin_tensor_without_a_source_raises(live_and_twin):
    _, twin = live_and_twin
    twin.net.register_buffer("stray", torch.zeros(3), persistent=False)
    try:
        with pytest.raises(StmError, match="stray"):
            twin.bind()
    finally:
        del twin.net._buffers["stray"]
    twin.net.proto_net[0].register_parameter("extra", nn.Parameter(torch.zeros(2)))
    try:
        with pytest.raises(StmError, match=r"proto_net\.0\.extra"):
            twin.bind()
    finally:
        del twin.net.proto_net[0]._parameters["extra"]
    twin.bind()


def test_twin_refuses_a_fused_net_and_the_device_fold_on_the_cpu(live_and_twin):
    net, twin = live_and_twin
    with pytest.raises(ValueError, match="optimize_for_inference"):
        validate.InferenceTwin(twin.net, fold="torch")
    with pytest.raises(ValueError, match="fold="):
        validate.InferenceTwin(net, fold="numpy")
    with pytest.raises(StmError, match="fold='torch'"):
        validate.InferenceTwin(net, fold="device")


# ---- YTVISValSet -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_ahead", [0, 4])
def test_val_set_serves_every_frame_once_in_order(tmp_path, read_ahead):
    path = tmp_path / "valid.json"
    path.write_text(json.dumps(val_ann()))
    reader = Reader()
    ds = datasets.YTVISValSet(str(path), img_prefix="root", frame_reader=reader, read_ahead=read_ahead)
    assert len(ds) == 3 and not ds.has_annotations
    assert [(v["id"], v["length"], v["height"], v["width"]) for v in ds.videos_info] == [(10 + i, T, h, w)
                                                                                       for i, (T, (h, w)) in enumerate(zip(LENGTHS, SIZES))]
    videos = ds.videos()
    assert [vid for vid, _ in videos] == [10, 11, 12]
    assert [v.shape for _, v in videos] == [(T, h, w, 3) for T, (h, w) in zip(LENGTHS, SIZES)]
    assert reader.reads == {}                                             # nothing is read before it is asked for
    for i, (_, v) in enumerate(videos):
        for t in range(v.shape[0]):
            f = v[t]
            again = v[t]                                                  # on_frame asks twice within a step
            assert again is f and f.dtype == torch.uint8 and tuple(f.shape) == v.shape[1:] and int(f[0, 0, 0]) == 10 * i + t
    ds.close()
    assert sorted(reader.reads) == sorted(os.path.join("root", n) for v in val_ann()["videos"] for n in v["file_names"])
    assert set(reader.reads.values()) == {1}


def test_lazy_video_keeps_a_window_of_frames():
    reader = Reader()
    ds = datasets.YTVISValSet(val_ann(annotations=[]), frame_reader=reader)
    assert not ds.has_annotations                                          # an empty list scores nothing
    v = ds.videos()[1][1]
    f0, f1 = v[0], v[1]
    assert v[0] is f0 and sorted(v._held) == [0, 1]
    v[2]                                                                   # two later frames have been asked for: frame 0 goes
    assert sorted(v._held) == [1, 2] and v[1] is f1
    v[3]
    assert sorted(v._held) == [2, 3]
    assert torch.equal(v[0], f0) and reader.reads["v1/00000.jpg"] == 2     # asked for again after that: read again
    with pytest.raises(IndexError):
        v[5]
    wide = ds.videos(keep=4)[1][1]
    for t in range(5):
        wide[t]
    assert sorted(wide._held) == [1, 2, 3, 4]


def test_read_ahead_is_bounded():
    reader = Reader()
    ds = datasets.YTVISValSet(val_ann(), frame_reader=reader, read_ahead=100)
    v = ds.videos()[1][1]
    assert ds._pool._max_workers == 8
    v[0]
    ds.close()
    assert len(reader.reads) == 5
    ds = datasets.YTVISValSet(val_ann(), frame_reader=reader, read_ahead=2)
    v = ds.videos()[1][1]
    assert ds._pool._max_workers == 2
    v[0]
    assert sorted(v._held) == [0, 1, 2]
    ds.close()
    with pytest.raises(ValueError):
        datasets.YTVISValSet(val_ann(), read_ahead=-1)


def test_a_frame_of_another_size_names_its_file():
    ds = datasets.YTVISValSet(val_ann(), frame_reader=Reader(wrong="v2/00001.jpg"))
    v = ds.videos()[2][1]
    v[0]
    with pytest.raises(ValueError, match=r"v2/00001\.jpg"):
        v[1]


# ---- validation() with an injected batcher and scorer --------------------------------------------------------------------------------------
class FakeBatcher:
    """run(videos, out_file): one object per video whose score comes from the frame's pixels -> results2json_videoseg, as VideoBatcher.run."""

    def __init__(self):
        self.flat = None

    def run(self, videos, out_file=None):
        flat = []
        for vid, frames in videos:
            for t in range(frames.shape[0]):
                px = int(frames[t][0, 0, 0])
                flat.append({"video_id": vid, "frame_id": t,
                             7: {"bbox": np.array([0, 0, 4, 4], dtype=np.float32), "score": np.float32(px / 64.0), "label": np.int64(1 + px % 3),
                                 "category": "c", "segm": {"size": list(frames.shape[1:3]), "counts": "0%d" % px}}})
        self.flat = flat
        return eval_utils.results2json_videoseg(copy.deepcopy(flat), out_file)


def test_validation_round_trip_with_injected_parts(live_and_twin, tmp_path):
    net, twin = live_and_twin
    ds = datasets.YTVISValSet(val_ann(), frame_reader=Reader())
    out_json, metrics_file, ann_file = str(tmp_path / "w" / "net_1_20.json"), str(tmp_path / "w" / "net_1_20.txt"), str(tmp_path / "valid.json")
    calls = []

    def scorer(ann, dt, output_file=None):
        calls.append((ann, dt, output_file))
        return {"mAP": 0.25}

    before, rng, gen = snapshot(net), rng_states(), twin.generation
    fake = FakeBatcher()
    assert validate.validation(twin, ds, out_json, batcher=fake, scorer=scorer) is None       # no annotation file: nothing is scored
    assert calls == [] and twin.generation == gen + 1
    want = eval_utils.results2json_videoseg(copy.deepcopy(fake.flat), str(tmp_path / "want.json"))
    assert json.load(open(out_json)) == json.load(open(tmp_path / "want.json")) and len(want) == 3
    assert not os.path.exists(metrics_file)
    got = validate.validation(twin, ds, out_json, ann_file=ann_file, metrics_file=metrics_file, batcher=fake, scorer=scorer)
    assert got == {"mAP": 0.25} and calls == [(ann_file, out_json, metrics_file)] and twin.generation == gen + 2
    assert same_snapshot(before, snapshot(net)) and same_rng(rng, rng_states())
    assert sorted(os.listdir(tmp_path / "w")) == ["net_1_20.json"]


def test_a_batcher_of_an_older_generation_is_refused(live_and_twin):
    _, twin = live_and_twin
    fake = FakeBatcher()
    fake.twin_generation = twin.generation
    twin.refresh()
    with pytest.raises(StmError, match="generation"):
        twin.run(fake, [])


def test_result_paths_follow_the_checkpoint():
    assert validate.result_paths("weights/STMask_plus_resnet50_3_20000.pth") == ("weights/STMask_plus_resnet50_3_20000.json",
                                                                                "weights/STMask_plus_resnet50_3_20000.txt")
    assert validate.result_paths("a.pth/net_0_7_interrupt.pth") == ("a.pth/net_0_7_interrupt.json", "a.pth/net_0_7_interrupt.txt")


def test_train_script_parses_the_validation_arguments():
    from scripts import train_ytvis
    a = train_ytvis.parse_args(["ann.json", "frames"])
    assert (a.valid_ann, a.valid_img_prefix, a.validation_interval, a.eval_slots, a.eval_planes) == (None, None, 0, 8, "fp16x2")
    a = train_ytvis.parse_args(["ann.json", "frames", "--valid_ann", "valid.json", "--valid_img_prefix", "valid/JPEGImages",
                                "--validation_interval", "5000", "--eval_slots", "4", "--eval_planes", "bf16x3"])
    assert (a.valid_ann, a.valid_img_prefix, a.validation_interval, a.eval_slots, a.eval_planes) == ("valid.json", "valid/JPEGImages", 5000, 4,
                                                                                                    "bf16x3")
    from scripts import validate as validate_script
    b = validate_script.parse_args(["w/net_1_20.pth", "valid.json", "valid/JPEGImages", "--slots", "2"])
    assert (b.ckpt, b.ann, b.img_prefix, b.slots, b.planes, b.out) == ("w/net_1_20.pth", "valid.json", "valid/JPEGImages", 2, "fp16x2", None)


# ---- the private binding -------------------------------------------------------------------------------------------------------------------
def test_row_mirror_has_the_headers_fields_and_size():
    assert abi_header.struct_field_names("fold.h", "stm_fold_row") == [f[0] for f in _lib.FoldRow._fields_]
    size = ctypes.CDLL(_lib.LIB_PATH).stm_fold_struct_bytes
    size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int]
    assert size(0) == ctypes.sizeof(_lib.FoldRow) == 72 and size(1) == 0


def row(**kw):
    r = _lib.FoldRow()
    for k, v in kw.items():
        setattr(r, k, v)
    return (_lib.FoldRow * 1)(r)


def test_fold_entry_refuses_bad_rows_before_any_launch():
    call = lambda rows, n: _lib.private_call("stm_fold_rows_f32", rows, n, None)      # noqa: E731
    call(None, 0)                                                                       # nothing to do: no device, no error
    call(row(kind=_lib.FOLD_COPY, numel=0), 1)
    with pytest.raises(StmError, match="takes 3 arguments"):
        _lib.private_call("stm_fold_rows_f32", None, 0)
    for rows, n, text in ((None, -1, "count"), (None, 65, "at most 64"), (None, 1, "NULL"),
                          (row(kind=_lib.FOLD_COPY, numel=-1), 1, "numel"),
                          (row(kind=_lib.FOLD_COPY, numel=1 << 31, dst=4096, src=8192), 1, "2\\^31"),
                          (row(kind=3, numel=4, dst=4096, src=8192), 1, "kind"),
                          (row(kind=_lib.FOLD_COPY, numel=4, src=8192), 1, "NULL dst"),
                          (row(kind=_lib.FOLD_WEIGHT, numel=4, dst=4096, inner=2, gamma=4096, var=4096), 1, "NULL src"),
                          (row(kind=_lib.FOLD_WEIGHT, numel=4, dst=4096, src=8192, inner=2, gamma=4096), 1, "BatchNorm"),
                          (row(kind=_lib.FOLD_BIAS, numel=4, dst=4096, inner=1, gamma=4096, var=4096, beta=4096), 1, "BatchNorm"),
                          (row(kind=_lib.FOLD_WEIGHT, numel=4, dst=4096, src=8192, inner=3, gamma=4096, var=4096), 1, "whole channels"),
                          (row(kind=_lib.FOLD_WEIGHT, numel=4, dst=4096, src=8192, inner=0, gamma=4096, var=4096), 1, "whole channels")):
        with pytest.raises(StmError, match=text):
            call(rows, n)


def test_fold_kernel_uses_no_scratch_and_no_lds():
    rows = [r for name, r in kernel_resources("fold.hip").items() if "fold_rows_kernel" in name]
    assert len(rows) == 1
    assert rows[0].scratch == 0
    assert rows[0].lds == 0
