"""Validation during training on the MI355X: InferenceTwin.refresh with the device fold against the torch form and against a freshly optimised
copy (state dict, bias3, and the detections of the rebuilt planar graph), the stale-generation refusal, validation() end to end through
datasets.YTVISValSet against VideoBatcher on the same frames held in memory, its scoring against a direct calc_metrics, and a validation() call
between two training steps that leaves the live net, the optimizer and the random generators bit for bit as they were."""
import json

import numpy as np
import pytest
import torch

from validate_helpers import LENGTHS, Reader, differing, fresh_copy, full_state, perturb, raw, rng_states, same_rng, same_snapshot, snapshot, val_ann
from stmask_amd import datasets, eval_utils, layers, synthetic, validate
from stmask_amd._lib import StmError
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.optim import GuardedSGD
from stmask_amd.pipeline import BatchedClipPipeline
from stmask_amd.train import NetLoss, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R50 = "STMask_plus_resnet50_config"
SRC_SIZES = ((72, 128), (48, 86), (72, 128))


def live_net(train=True):
    net = STMask(get_cfg(R50))
    synthetic.fill_state_dict(net, seed=0, seed_detections=True)
    net = net.to(DEV)
    return net.train() if train else net.eval()


def detect(net, frame):
    """One frame through a new BatchedClipPipeline on `net` -> (the packed detections as bytes, the number of tracked instances)."""
    pipe = BatchedClipPipeline(net, 1)
    with torch.no_grad():
        packed = pipe.step(frame, is_first=True)
        packed = packed[0] if isinstance(packed, (tuple, list)) else packed
        det = pipe.detections()[0]
    torch.cuda.synchronize()
    return raw(packed), (int(det["box"].shape[0]) if det else 0), {k: raw(v) for k, v in det.items()} if det else {}


@pytest.mark.parametrize("planes", ["fp16x2", "bf16x3"])
def test_device_refresh_equals_the_torch_form_and_a_fresh_copy(planes):
    net = live_net()
    twin = validate.InferenceTwin(net, planes=planes, fold="device")
    by_torch = validate.InferenceTwin(net, planes=planes, fold="torch")
    assert twin.planar and twin.generation == 0
    frame = synthetic.synthetic_clip(1, 128, 192, seed=0).to(DEV).contiguous(memory_format=torch.channels_last)
    old_packed, old_n, _ = detect(twin.net, frame)
    old_batcher = twin.batcher(2)
    perturb(net, seed=3)
    before = snapshot(net)
    twin.refresh()
    by_torch.write_parameters()
    assert validate.COUNTERS["fold_launches"] == 0                                   # (the torch form's last write)
    assert twin.generation == 1 and same_snapshot(before, snapshot(net))
    fresh = fresh_copy(net, planar=True, planes=planes)
    got, want = full_state(twin.net), full_state(fresh)
    assert any(k.endswith("bias3") for k in got)
    assert differing(got, full_state(by_torch.net)) == [] and differing(got, want) == []
    new_packed, new_n, new_det = detect(twin.net, frame)
    ref_packed, ref_n, ref_det = detect(fresh, frame)
    print(f"\n{planes}: {old_n} tracked instances before the refresh, {new_n} after, {ref_n} on the fresh copy")
    assert ref_n > 0 and new_n == ref_n and torch.equal(new_packed, ref_packed) and differing(new_det, ref_det) == []
    assert not torch.equal(new_packed, old_packed)                                   # the refresh reached the planar graph
    with pytest.raises(StmError, match="generation 0"):
        twin.run(old_batcher, [])
    assert twin.batcher(2).twin_generation == 1


def test_device_write_is_a_handful_of_launches():
    net = live_net(train=False)
    twin = validate.InferenceTwin(net, fold="device")
    twin.write_parameters()
    rows = sum(1 for s in twin.sources if s.kind != validate.BIAS3 and s.dst.dtype == torch.float32)
    assert 1 <= validate.COUNTERS["fold_launches"] == -(-rows // 64) <= 6
    assert differing(full_state(twin.net), full_state(fresh_copy(net, planar=False))) == []


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def split_frames():
    g = np.random.default_rng(11)
    frames = {}
    for i, (T, (h, w)) in enumerate(zip(LENGTHS, SRC_SIZES)):
        base = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for t in range(T):
            frames[(i, t)] = np.ascontiguousarray(np.roll(base, (2 * t, 3 * t), axis=(0, 1)))
    return frames


def test_validation_through_the_lazy_split_equals_the_batcher_on_frames_in_memory(tmp_path):
    net = live_net()
    twin = validate.InferenceTwin(net)
    frames = split_frames()
    reader = Reader(frames=frames, sizes=SRC_SIZES)
    ann = val_ann(sizes=SRC_SIZES)
    ds = datasets.YTVISValSet(ann, frame_reader=reader, read_ahead=4)
    out_json = str(tmp_path / "net_0_1.json")
    assert validate.validation(twin, ds, out_json, n_slots=2) is None and twin.generation == 1
    ds.close()
    assert set(reader.reads.values()) == {1} and len(reader.reads) == sum(LENGTHS)
    held = [(v["id"], torch.stack([torch.from_numpy(frames[(i, t)]) for t in range(v["length"])]).to(DEV)) for i, v in enumerate(ann["videos"])]
    want = twin.batcher(2).run(held, out_file=str(tmp_path / "held.json"))
    got = json.load(open(out_json))
    assert len(want) > 0 and got == json.load(open(tmp_path / "held.json"))
    # scored: ground truth made of the results themselves (every second object dropped), through the hook and directly
    ann["annotations"] = [dict(id=k + 1, video_id=r["video_id"], category_id=r["category_id"], iscrowd=0, segmentations=r["segmentations"])
                          for k, r in enumerate(got) if k % 2 == 0]
    ann_file = str(tmp_path / "valid.json")
    json.dump(ann, open(ann_file, "w"))
    ds = datasets.YTVISValSet(ann_file, frame_reader=Reader(frames=frames, sizes=SRC_SIZES))
    assert ds.has_annotations
    scored_json, metrics_file = validate.result_paths(str(tmp_path / "net_0_2.pth"))
    stats = validate.validation(twin, ds, scored_json, ann_file=ann_file, metrics_file=metrics_file, n_slots=2)
    assert json.load(open(scored_json)) == got
    direct = eval_utils.calc_metrics(ann_file, scored_json, output_file=str(tmp_path / "direct.txt"))
    assert np.array_equal(np.asarray(stats), np.asarray(direct)) and float(np.asarray(stats)[0]) > 0
    assert open(metrics_file).read() == open(tmp_path / "direct.txt").read()


def test_validation_between_two_training_steps_leaves_the_run_as_it_was(tmp_path):
    net = live_net()
    cfg = net.cfg
    nl = NetLoss(net, layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, temporal_fusion=cfg.temporal_fusion_module, max_pos=64))
    opt = GuardedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    batch = synthetic.synthetic_train_batch(2, 128, 192, 0, device=DEV)
    twin = validate.InferenceTwin(net)
    ds = datasets.YTVISValSet(val_ann(sizes=SRC_SIZES), frame_reader=Reader(frames=split_frames(), sizes=SRC_SIZES))
    # MIOpen's deterministic solvers, as in the other train-step tests (the solvers they have already picked in this process are reused)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        train_step(nl, opt, batch)
    torch.cuda.synchronize()

    def run_state():
        return (snapshot(net), {i: raw(s["momentum_buffer"]) for i, s in enumerate(opt.state.values())}, opt.counters(),
                {n: (None if p.grad is None else raw(p.grad)) for n, p in net.named_parameters()})

    before, rng = run_state(), rng_states(cuda=True)
    validate.validation(twin, ds, str(tmp_path / "net_0_1.json"), n_slots=2)
    torch.cuda.synchronize()
    after = run_state()
    assert same_snapshot(before[0], after[0]) and net.training
    assert differing(before[1], after[1]) == [] and before[2] == after[2] == (1, 0)
    assert all((before[3][n] is None and after[3][n] is None) or torch.equal(before[3][n], after[3][n]) for n in before[3])
    assert same_rng(rng, rng_states(cuda=True))
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        train_step(nl, opt, batch)                                                    # ... and the run goes on
    assert opt.counters() == (2, 0)
