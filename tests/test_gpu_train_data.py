"""Training batches on the MI355X (csrc/train_data.hip, stmask_amd/datasets.py) against the numpy restatement of the reference's host chain
(train_data_restate.py): masks byte-equal, frames and boxes bit-equal, then a collated batch through train.train_step."""
import functools
import random

import numpy as np
import pytest
import torch

import train_data_cases as C
import train_data_restate as R
from stmask_amd import datasets, layers, ops, synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.train import NetLoss, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP, WP = 32, 64


@functools.lru_cache(maxsize=None)
def mask_cases():
    """[(name, H0, W0, counts, dense)] over every source size: computed once, shared, read-only."""
    out = []
    for H0, W0 in C.SOURCES:
        for name, counts in C.run_lists(H0, W0).items():
            out.append((f"{H0}x{W0}/{name}", H0, W0, counts, R.dense(counts, H0, W0)))
    return out


def render(rles, sizes, flips, size=C.SIZE, **kw):
    gt = datasets.render_ground_truth(rles, sizes, flips, size=size, divisor=C.DIVISOR, device=DEV, **kw)
    return gt, gt.masks.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("flip", [False, True])
def test_masks_from_run_lists_and_from_strings_equal_the_restatement(flip):
    cases = mask_cases()
    assert {"48x80/stripes_1px", "48x80/checker_1px", "15x22/zero_runs", "50x30/last_pixel", "37x53/empty", "37x53/full"} <= {c[0] for c in cases}
    assert len(dict((c[0], c) for c in cases)["48x80/stripes_1px"][3]) == 3840
    rles = [C.rle(c[3], c[1], c[2], compressed=False) for c in cases] + [C.rle(c[3], c[1], c[2], compressed=True) for c in cases]
    sizes = [(c[1], c[2]) for c in cases] * 2
    datasets.reset_counters()
    gt, got = render(rles, sizes, [flip] * len(rles))
    assert datasets.COUNTERS["launches"] == 3                       # decode, starts, masks (no boxes here)
    gt.status.raise_if_bad()
    assert got.shape == (2 * len(cases), HP, WP) and got.dtype == np.uint8
    for i, (name, H0, W0, counts, dense) in enumerate(cases):
        want = R.mask_target(dense, C.SIZE, C.DIVISOR, flip)
        assert np.array_equal(got[i], want), (name, "list", int((got[i] != want).sum()))
        assert np.array_equal(got[len(cases) + i], want), (name, "string")
    area = gt.area.cpu().numpy()
    assert area[gt.pos].tolist() == [int(c[4].sum()) for c in cases] * 2


def test_masks_are_the_same_bytes_from_run_to_run_and_fill_a_dirty_buffer():
    cases = mask_cases()
    rles = [C.rle(c[3], c[1], c[2]) for c in cases]
    sizes = [(c[1], c[2]) for c in cases]
    flips = [i % 2 == 1 for i in range(len(cases))]                # mixed flips in one launch
    junk = torch.full((len(cases) * HP * WP * 2,), 255, dtype=torch.uint8, device=DEV)     # what the next allocation may reuse
    del junk
    _, a = render(rles, sizes, flips)
    _, b = render(rles, sizes, flips)
    assert a.tobytes() == b.tobytes() and a.max() <= 1
    for i, c in enumerate(cases):
        assert np.array_equal(a[i], R.mask_target(c[4], C.SIZE, C.DIVISOR, flips[i])), c[0]


def test_a_wrong_sum_is_flagged_and_the_other_masks_are_still_right():
    cases = [c for c in mask_cases() if c[0].startswith("37x53/")]
    rles = [C.rle(c[3], c[1], c[2]) for c in cases]
    bad = len(rles) // 2
    rles[bad] = {"size": [37, 53], "counts": list(rles[bad]["counts"][:-1]) + [rles[bad]["counts"][-1] + 3]}
    bad_str = C.rle(cases[0][3], 37, 53, compressed=True)
    bad_str["counts"] = bad_str["counts"] + "o"                    # a string that ends inside a value
    rles.append(bad_str)
    gt, got = render(rles, [(37, 53)] * len(rles), [False] * len(rles), who=lambda i: f"video 10, annotation {500 + i}, frame 1")
    for i, c in enumerate(cases):
        want = R.mask_target(c[4], C.SIZE, C.DIVISOR, False) if i != bad else np.zeros((HP, WP), np.uint8)
        assert np.array_equal(got[i], want), c[0]
    assert not got[-1].any()
    with pytest.raises(ValueError) as e:
        gt.status.raise_if_bad()
    assert f"annotation {500 + bad}" in str(e.value) and "video 10" in str(e.value) and "frame 1" in str(e.value) and "sum" in str(e.value)


def test_masks_at_the_real_size():
    H0, W0 = C.REAL_SOURCE
    rng = np.random.default_rng(5)
    dense = [C.blob(H0, W0, rng, 4), C.blob(H0, W0, rng, 2), rng.random((H0, W0)) < 0.3]
    rles = [C.rle(C.counts_of_mask(m), H0, W0, compressed=(i == 1)) for i, m in enumerate(dense)]
    flips = [False, True, True]
    gt, got = render(rles, [(H0, W0)] * 3, flips, size=C.REAL_SIZE)
    gt.status.raise_if_bad()
    assert got.shape == (3, 384, 640)
    for i, m in enumerate(dense):
        want = R.mask_target(m.astype(np.uint8), C.REAL_SIZE, C.DIVISOR, flips[i])
        assert np.array_equal(got[i], want), i
    assert not got[:, 360:].any() and got[0].any()


# ------------------------------------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def frame_set():
    return [C.frame(H0, W0) for H0, W0 in C.SOURCES]


def test_frames_without_flip_and_to_rgb_are_the_inference_preprocessing():
    dev = [torch.from_numpy(f).to(DEV) for f in frame_set()]
    a = datasets.train_frames(dev, [False] * len(dev), C.SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb=False)
    b = ops.preprocess_frames_multi(dev, size=C.SIZE, divisor=C.DIVISOR, mean=C.MEAN, std=C.STD, mode=1)
    assert a.shape == (len(dev), 3, HP, WP) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("flip,to_rgb", [(False, False), (True, False), (False, True), (True, True)])
def test_frames_equal_the_restatement(flip, to_rgb):
    frames = frame_set()
    dev = [torch.from_numpy(f).to(DEV) for f in frames]
    flips = [flip] * len(dev)
    flips[1] = not flip                                              # a mixed launch: the flag is per frame
    got = datasets.train_frames(dev, flips, C.SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb=to_rgb).cpu().numpy()
    for i, f in enumerate(frames):
        want = R.frame_target(f, C.SIZE, C.DIVISOR, flips[i], to_rgb, C.MEAN, C.STD)
        assert got[i].tobytes() == want.tobytes(), (f.shape, float(np.abs(got[i] - want).max()))
        assert not got[i][:, 24:].any() and not got[i][:, :, 40:].any()


def test_frames_read_crop_views_through_their_row_stride():
    big = torch.from_numpy(C.frame(60, 90, seed=3)).to(DEV)
    crop = big[5:42, 11:64]                                          # 37 x 53, row stride 270 bytes > 3 * 53
    assert crop.stride(0) == 270 and not crop.is_contiguous()
    got = datasets.train_frames([crop, crop], [False, True], C.SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb=True).cpu().numpy()
    src = np.ascontiguousarray(crop.cpu().numpy())
    for i, flip in enumerate((False, True)):
        assert got[i].tobytes() == R.frame_target(src, C.SIZE, C.DIVISOR, flip, True, C.MEAN, C.STD).tobytes()


def test_seventy_frames_take_two_launches():
    frames = frame_set()
    dev = [torch.from_numpy(f).to(DEV) for f in frames]
    many = [dev[i % len(dev)] for i in range(70)]
    flips = [(i // 5) % 2 == 1 for i in range(70)]
    datasets.reset_counters()
    got = datasets.train_frames(many, flips, C.SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb=True).cpu().numpy()
    assert datasets.COUNTERS["launches"] == 2
    want = {(i, f): R.frame_target(frames[i], C.SIZE, C.DIVISOR, f, True, C.MEAN, C.STD) for i in range(len(frames)) for f in (False, True)}
    for i in range(70):
        assert got[i].tobytes() == want[(i % len(frames), flips[i])].tobytes(), i


def test_frame_at_the_real_size():
    f = C.frame(*C.REAL_SOURCE)
    got = datasets.train_frames([torch.from_numpy(f).to(DEV)] * 2, [False, True], C.REAL_SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb=True).cpu().numpy()
    assert got.shape == (2, 3, 384, 640)
    for i, flip in enumerate((False, True)):
        assert got[i].tobytes() == R.frame_target(f, C.REAL_SIZE, C.DIVISOR, flip, True, C.MEAN, C.STD).tobytes()


# ------------------------------------------------------------------------------------------------------------------ boxes
def test_boxes_equal_the_float32_restatement():
    rles, sizes, flips, boxes, want = [], [], [], [], []
    for H0, W0 in C.SOURCES + [C.REAL_SOURCE]:
        b = C.boxes_for(H0, W0)
        for flip in (False, True):
            rles += [C.rle([H0 * W0], H0, W0)] * len(b)
            sizes += [(H0, W0)] * len(b)
            flips += [flip] * len(b)
            boxes.append(b)
            want.append(R.boxes_target(b, H0, W0, C.SIZE, C.DIVISOR, flip))
    boxes, want = np.concatenate(boxes), np.concatenate(want)
    gt = datasets.render_ground_truth(rles, sizes, flips, boxes=boxes, size=C.SIZE, divisor=C.DIVISOR, device=DEV)
    got = gt.boxes.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.abs(got - want).max()
    assert (got == 0).any() and (got[:, 2] == 40 / 64).any() and (got[:, 3] == 24 / 32).any()        # the clip was touched on every side
    # a flipped box at x = 0 lands at w - 1 scaled; at x = W0 - 1 it lands left of it
    k = len(C.boxes_for(24, 40))
    assert got[k + 4, 0] == np.float32(39) / np.float32(64) and got[k + 5, 0] == np.float32(0)


# ------------------------------------------------------------------------------------------------------------------ the collated batch
def dataset(flip_ratio=0.5):
    return datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, size_divisor=C.DIVISOR, flip_ratio=flip_ratio)


def records(ds, picks, seed=0):
    random.seed(seed)
    np.random.seed(seed)
    return [ds[ds.img_ids.index(p)] for p in picks]


def check_batch(recs, batch):
    images, gt_bboxes, gt_labels, gt_masks, gt_ids, img_meta = batch
    assert images.shape == (len(recs), 2, 3, HP, WP) and images.dtype == torch.float32
    for c, r in enumerate(recs):
        H0, W0 = r["size"]
        assert img_meta[c] is r["img_meta"]
        for t in range(2):
            want = R.frame_target(r["frames"][t], C.SIZE, C.DIVISOR, r["flip"], True, C.MEAN, C.STD)
            assert images[c, t].cpu().numpy().tobytes() == want.tobytes()
            G = len(r["segms"][t])
            assert gt_masks[c][t].shape == (G, HP, WP) and gt_masks[c][t].dtype == torch.uint8
            assert gt_bboxes[c][t].shape == (G, 4) and gt_labels[c][t].dtype == torch.int64 and gt_ids[c][t].dtype == torch.int64
            assert gt_labels[c][t].tolist() == r["labels"][t].tolist() and gt_ids[c][t].tolist() == list(r["obj_ids"][t])
            wb = R.boxes_target(r["bboxes"][t], H0, W0, C.SIZE, C.DIVISOR, r["flip"])
            assert np.array_equal(gt_bboxes[c][t].cpu().numpy().view(np.int32), wb.view(np.int32))
            for j, seg in enumerate(r["segms"][t]):
                counts = seg["counts"] if isinstance(seg["counts"], list) else None
                dense = R.dense(counts, H0, W0) if counts is not None else None
                if dense is None:                                   # the compressed track of video 20: the rectangle its box describes
                    x, y, bw, bh = [a for a in C.annotations()["annotations"] if a["id"] == r["obj_ids"][t][j]][0]["bboxes"][r["frame_ids"][t]]
                    dense = C._rect(H0, W0, x, y, bw, bh).astype(np.uint8)
                assert np.array_equal(gt_masks[c][t][j].cpu().numpy(), R.mask_target(dense, C.SIZE, C.DIVISOR, r["flip"]))


def test_collate_device_gives_views_of_one_buffer_per_kind_and_the_same_bytes_twice():
    recs = records(dataset(), [(10, 0), (20, 1), (30, 0)], seed=1)
    assert [r["flip"] for r in recs] == [True, False, True]        # np.random.seed(1) draws 0.417, 0.720, 0.0001: both settings in one batch
    datasets.reset_counters()
    a = datasets.collate_device(recs, DEV)
    assert datasets.COUNTERS["launches"] == 5                      # frames, decode (video 20's strings), starts, masks, boxes
    assert datasets.COUNTERS["uploads"] == 5                       # frames, run lists, characters, descriptors, boxes
    b = datasets.collate_device(recs, DEV)
    check_batch(recs, a)
    for k in range(1, 5):
        base = a[k][0][0].untyped_storage().data_ptr()
        for c in range(len(recs)):
            for t in range(2):
                assert a[k][c][t].untyped_storage().data_ptr() == base
                assert torch.equal(a[k][c][t], b[k][c][t])
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()


def test_a_frame_without_objects_and_max_gt():
    ds = dataset()
    recs = records(ds, [(10, 1), (10, 4)], seed=2)
    recs[0]["segms"][1], recs[0]["bboxes"][1], recs[0]["labels"][1] = [], np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
    recs[0]["obj_ids"][1] = []
    batch = datasets.collate_device(recs, DEV)
    check_batch(recs, batch)
    assert batch[3][0][1].shape == (0, HP, WP) and batch[1][0][1].shape == (0, 4)
    one = datasets.collate_device(recs, DEV, max_gt=1)
    assert [[m.shape[0] for m in clip] for clip in one[3]] == [[min(len(r["segms"][t]), 1) for t in range(2)] for r in recs]
    assert torch.equal(one[3][1][0][0], batch[3][1][0][0]) and torch.equal(one[4][1][0], batch[4][1][0][:1])


def test_collate_device_names_the_record_of_a_malformed_mask():
    recs = records(dataset(), [(10, 0), (30, 0)])
    seg = recs[0]["segms"][1][0]
    recs[0]["segms"][1][0] = {"size": seg["size"], "counts": seg["counts"][:-1] + [seg["counts"][-1] - 1]}
    with pytest.raises(ValueError) as e:
        datasets.collate_device(recs, DEV)
    msg = str(e.value)
    assert "video 10" in msg and f"annotation {recs[0]['obj_ids'][1][0]}" in msg and f"frame {recs[0]['frame_ids'][1]}" in msg


def test_the_kernels_and_a_deferred_collate_never_wait_for_the_device():
    recs = records(dataset(), [(10, 0), (20, 1), (30, 0)])
    dev = [torch.from_numpy(f).to(DEV) for f in frame_set()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        datasets.train_frames(dev, [True] * len(dev), C.SIZE, C.DIVISOR, C.MEAN, C.STD)
        cases = mask_cases()[:6]
        gt = datasets.render_ground_truth([C.rle(c[3], c[1], c[2], compressed=(i % 2 == 0)) for i, c in enumerate(cases)],
                                          [(c[1], c[2]) for c in cases], [False] * 6, boxes=np.zeros((6, 4), np.float32), device=DEV,
                                          size=C.SIZE, divisor=C.DIVISOR)
        *batch, status = datasets.collate_device(recs, DEV, check="deferred")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    status.raise_if_bad()
    gt.status.raise_if_bad()
    check_batch(recs, tuple(batch))


def test_the_loader_feeds_train_step(tmp_path):
    """Three clips from the loader through train.train_step with R50 FCA at 32 x 64: finite loss terms, a gradient for every parameter."""
    cfg = get_cfg("STMask_plus_resnet50_config")
    net = STMask(cfg)
    sd = synthetic.fill_state_dict(net, seed=0)
    path = str(tmp_path / "backbone.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("backbone.")}, path)
    torch.manual_seed(0)
    net.init_weights(path)
    net = net.to(DEV).train()
    nl = NetLoss(net, layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, temporal_fusion=cfg.temporal_fusion_module))
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    random.seed(1)
    np.random.seed(1)
    loader = datasets.TrainLoader(dataset(), 3, seed=0, device=DEV)
    batches = list(loader)
    assert len(batches) == len(loader) == 2 and batches[0][0].shape == (3, 2, 3, HP, WP)
    losses = train_step(nl, opt, batches[0])
    vals = {k: float(v) for k, v in losses.items()}
    print("\n" + "  ".join(f"{k} {v:.4f}" for k, v in vals.items()))
    assert sorted(vals) == sorted(["BIoU", "M", "C", "center", "B_shift", "M_shift", "T"]) and all(np.isfinite(v) for v in vals.values()), vals
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    bad = [n for n, p in net.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    assert missing == [] and bad == []
