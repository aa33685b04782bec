"""ExtraAugmentation on the MI355X (csrc/extra_aug.hip) against the numpy restatement (extra_aug_restate.py) and the runs of the reference's own
code in tests/golden/extra_aug_cases.npz: the augmented source byte for byte, the fused frame kernel bit-equal to the plain transform of the
augmented uint8 source, the fused mask kernel byte-equal, identity parameters, and an augmented batch through collate_device and train_step.
All equalities are exact: the arithmetic is integer or single-rounded fp32 on both sides."""
import functools
import random

import numpy as np
import pytest
import torch

import extra_aug_restate as R
import train_data_cases as C
import train_data_restate as T
from stmask_amd import datasets, layers, synthetic
from stmask_amd import extra_aug as EA
from stmask_amd._lib import StmError
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.train import NetLoss, train_step
from test_extra_aug_cpu import ALL_ON, CASES, sample_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [C.SIZE, (96, 56)]                      # (w, h): 24 x 40 padded to 32 x 64, and 56 x 96 padded to 64 x 96


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ the augmented source
@pytest.mark.parametrize("i", range(len(CASES)))
def test_augmented_source_is_the_references_bytes(i):
    c = CASES[i]
    p = sample_case(c)[0]
    datasets.reset_counters()
    got = datasets.augmented_source(dev(c["img"]), p)
    assert datasets.COUNTERS["launches"] == 1 and datasets.COUNTERS["uploads"] == 1
    assert got.dtype == torch.uint8 and got.shape == c["out_img"].shape
    got = got.cpu().numpy()
    assert np.array_equal(got, c["out_img"]), (int((got != c["out_img"]).sum()), repr(p))


def test_augmented_source_with_cast_clip():
    for c in CASES:
        p = sample_case(c, cast="clip")[0]
        assert np.array_equal(datasets.augmented_source(dev(c["img"]), p).cpu().numpy(), R.augmented_source(c["img"], p))


# ------------------------------------------------------------------------------------------------------------------ the fused kernels
def two_boxes(H0, W0):
    return np.array([[0.15 * W0, 0.2 * H0, 0.65 * W0, 0.8 * H0], [0.55 * W0, 0.3 * H0, 0.85 * W0, 0.7 * H0]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def drawn():
    """[(frame, AugParams, [(counts, dense)])] over the source sizes of train_data_cases, four seeded draws each with all three transforms on:
    computed once, shared, read-only."""
    aug = EA.ExtraAugmentation(**ALL_ON)
    out = []
    for k, (H0, W0) in enumerate(C.SOURCES):
        lists = C.run_lists(H0, W0)
        masks = [(lists[n], T.dense(lists[n], H0, W0)) for n in ("blob_a", "noise", "full", "zero_runs")]
        for s in range(4):
            p = aug.sample(H0, W0, two_boxes(H0, W0), np.array([1, 2]), [1, 2], [None, None], rng=np.random.RandomState(10 * k + s))[0]
            out.append((C.frame(H0, W0, seed=s), p, masks))
    return out


def test_the_draws_reach_every_transform_and_their_combinations():
    ps = [d[1] for d in drawn()]
    assert any(p.expand and p.crop for p in ps) and any(p.expand and not p.crop for p in ps) and any(p.crop and not p.expand for p in ps)
    assert any(p.hue != 0 for p in ps) and any(p.saturation != 1 for p in ps) and any(p.perm != (0, 1, 2) for p in ps)
    assert any(p.alpha != 1 and p.contrast_mode == m for p in ps for m in (0, 1)) and any(p.delta != 0 for p in ps)


@functools.lru_cache(maxsize=None)
def frame_wants(size, flip):
    return [R.frame_target(f, p, size, C.DIVISOR, flip, True, C.MEAN, C.STD) for f, p, _ in drawn()]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("flip", [False, True])
def test_fused_frames_equal_the_transform_of_the_augmented_source(size, flip):
    cases = drawn()
    datasets.reset_counters()
    got = datasets.train_frames([dev(f) for f, _, _ in cases], [flip] * len(cases), size, C.DIVISOR, C.MEAN, C.STD, True, aug=[p for _, p, _ in cases])
    assert datasets.COUNTERS["launches"] == 1 and datasets.COUNTERS["uploads"] == 1
    got = got.cpu().numpy()
    for i, want in enumerate(frame_wants(size, flip)):
        assert got[i].tobytes() == want.tobytes(), (i, cases[i][0].shape, repr(cases[i][1]), float(np.abs(got[i] - want).max()))


def test_fused_frames_without_to_rgb():
    cases = drawn()[:6]
    got = datasets.train_frames([dev(f) for f, _, _ in cases], [i % 2 == 1 for i in range(6)], C.SIZE, C.DIVISOR, C.MEAN, C.STD, False,
                                aug=[p for _, p, _ in cases]).cpu().numpy()
    for i, (f, p, _) in enumerate(cases):
        assert got[i].tobytes() == R.frame_target(f, p, C.SIZE, C.DIVISOR, i % 2 == 1, False, C.MEAN, C.STD).tobytes(), i


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("flip", [False, True])
def test_fused_masks_equal_the_transform_of_the_augmented_mask(size, flip):
    cases = drawn()
    rles, sizes, params, wants = [], [], [], []
    for f, p, masks in cases:
        for j, (counts, dense) in enumerate(masks):
            rles.append(C.rle(counts, p.H0, p.W0, compressed=(j == 1)))
            sizes.append((p.H0, p.W0))
            params.append(p)
            wants.append(R.mask_target(dense, p, size, C.DIVISOR, flip))
    datasets.reset_counters()
    gt = datasets.render_ground_truth(rles, sizes, [flip] * len(rles), size=size, divisor=C.DIVISOR, device=DEV, aug=params)
    assert datasets.COUNTERS["launches"] == 3                        # decode, starts, masks: as without augmentation
    gt.status.raise_if_bad()
    got = gt.masks.cpu().numpy()
    for i, want in enumerate(wants):
        assert np.array_equal(got[i], want), (i, repr(params[i]), int((got[i] != want).sum()))
    assert any(w.any() for w in wants) and any(not w.any() for w in wants)


def test_identity_parameters_give_the_bits_of_the_plain_kernels():
    frames = [C.frame(H0, W0) for H0, W0 in C.SOURCES]
    d = [dev(f) for f in frames]
    flips = [i % 2 == 0 for i in range(len(d))]
    ident = [EA.identity_params(*f.shape[:2]) for f in frames]
    for to_rgb in (False, True):
        a = datasets.train_frames(d, flips, C.SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb)
        b = datasets.train_frames(d, flips, C.SIZE, C.DIVISOR, C.MEAN, C.STD, to_rgb, aug=ident)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for f, p, x in zip(frames, ident, d):
        assert np.array_equal(datasets.augmented_source(x, p).cpu().numpy(), f)
    rles, sizes, params = [], [], []
    for H0, W0 in C.SOURCES:
        for name, counts in C.run_lists(H0, W0).items():
            rles.append(C.rle(counts, H0, W0, compressed=(len(rles) % 3 == 0)))
            sizes.append((H0, W0))
            params.append(EA.identity_params(H0, W0))
    flips = [i % 2 == 1 for i in range(len(rles))]
    a = datasets.render_ground_truth(rles, sizes, flips, size=C.SIZE, divisor=C.DIVISOR, device=DEV)
    b = datasets.render_ground_truth(rles, sizes, flips, size=C.SIZE, divisor=C.DIVISOR, device=DEV, aug=params)
    assert torch.equal(a.masks, b.masks) and a.masks.any()


def test_a_row_strided_source():
    big = dev(C.frame(60, 90, seed=3))
    crop = big[5:42, 11:64]                                          # 37 x 53, row stride 270 bytes > 3 * 53
    assert crop.stride(0) == 270 and not crop.is_contiguous()
    src = np.ascontiguousarray(crop.cpu().numpy())
    ps = [d[1] for d in drawn() if (d[1].H0, d[1].W0) == (37, 53)]
    got = datasets.train_frames([crop] * len(ps), [False] * len(ps), C.SIZE, C.DIVISOR, C.MEAN, C.STD, True, aug=ps).cpu().numpy()
    for i, p in enumerate(ps):
        assert got[i].tobytes() == R.frame_target(src, p, C.SIZE, C.DIVISOR, False, True, C.MEAN, C.STD).tobytes()
        assert np.array_equal(datasets.augmented_source(crop, p).cpu().numpy(), R.augmented_source(src, p))


def test_one_frame_more_than_a_launch_takes_two_and_runs_repeat_the_bytes():
    cases = drawn()
    n = 65
    frames = [dev(f) for f, _, _ in cases]
    pick = [i % len(cases) for i in range(n)]
    datasets.reset_counters()
    run = lambda: datasets.train_frames([frames[i] for i in pick], [True] * n, C.SIZE, C.DIVISOR, C.MEAN, C.STD, True,       # noqa: E731
                                        aug=[cases[i][1] for i in pick])
    a = run()
    assert datasets.COUNTERS["launches"] == 2 and datasets.COUNTERS["uploads"] == 1
    b = run()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a = a.cpu().numpy()
    wants = frame_wants(C.SIZE, True)
    for k in range(n):
        assert a[k].tobytes() == wants[pick[k]].tobytes(), k


def test_the_real_size():
    H0, W0 = C.REAL_SOURCE
    f = C.frame(H0, W0)
    p = EA.AugParams(H0, W0)
    p.photo, p.delta, p.contrast_mode, p.alpha, p.saturation, p.hue, p.perm = True, 21.5, 0, 1.37, 1.41, -11.25, (2, 0, 1)
    p.expand, p.canvas, p.fill = (1.7, 301, 215), (int(H0 * 1.7), int(W0 * 1.7)), C.MEAN[::-1]
    p.crop = (100, 60, 1100, 650)
    got = datasets.train_frames([dev(f)], [True], C.REAL_SIZE, C.DIVISOR, C.MEAN, C.STD, True, aug=[p]).cpu().numpy()
    assert got.shape == (1, 3, 384, 640)
    assert got[0].tobytes() == R.frame_target(f, p, C.REAL_SIZE, C.DIVISOR, True, True, C.MEAN, C.STD).tobytes()
    rng = np.random.default_rng(5)
    dense = [C.blob(H0, W0, rng, 4).astype(np.uint8), (rng.random((H0, W0)) < 0.3).astype(np.uint8)]
    rles = [C.rle(C.counts_of_mask(m), H0, W0, compressed=(i == 1)) for i, m in enumerate(dense)]
    gt = datasets.render_ground_truth(rles, [(H0, W0)] * 2, [True, False], size=C.REAL_SIZE, divisor=C.DIVISOR, device=DEV, aug=[p, p])
    gt.status.raise_if_bad()
    got = gt.masks.cpu().numpy()
    for i, m in enumerate(dense):
        assert np.array_equal(got[i], R.mask_target(m, p, C.REAL_SIZE, C.DIVISOR, i == 0)), i
    assert got[1].any()


# ------------------------------------------------------------------------------------------------------------------ the collated batch
def dataset(**kw):
    return datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, size_divisor=C.DIVISOR, **kw)


def records(ds, picks, seed=0):
    random.seed(seed)
    np.random.seed(seed)
    return [ds[ds.img_ids.index(p)] for p in picks]


def test_collate_device_of_augmented_clips_feeds_train_step(tmp_path):
    picks = [(10, 0), (20, 1), (30, 0)]
    plain = records(dataset(), picks, seed=3)
    recs = records(dataset(extra_aug=ALL_ON), picks, seed=3)
    assert all(len(r["aug"]) == 2 for r in recs) and any(p.crop or p.expand for r in recs for p in r["aug"])
    with pytest.raises(StmError, match="with and without aug"):
        datasets.collate_device([recs[0], plain[1]], DEV)
    datasets.reset_counters()
    datasets.collate_device(plain, DEV, check="deferred")[-1].raise_if_bad()
    base = dict(datasets.COUNTERS)
    torch.cuda.synchronize()
    datasets.reset_counters()
    torch.cuda.set_sync_debug_mode("error")
    try:
        *batch, status = datasets.collate_device(recs, DEV, check="deferred")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert datasets.COUNTERS["launches"] <= base["launches"] and datasets.COUNTERS["uploads"] <= base["uploads"] + 1, (datasets.COUNTERS, base)
    status.raise_if_bad()
    images, gt_bboxes, gt_labels, gt_masks, gt_ids, _ = batch
    anns = {a["id"]: a for a in C.annotations()["annotations"]}
    for c, r in enumerate(recs):
        for t in range(2):
            p = r["aug"][t]
            want = R.frame_target(r["frames"][t], p, C.SIZE, C.DIVISOR, r["flip"], True, r["mean"], r["std"])
            assert images[c, t].cpu().numpy().tobytes() == want.tobytes(), (c, t)
            H0, W0 = r["frames"][t].shape[:2]
            assert gt_masks[c][t].shape[0] == len(r["segms"][t]) == len(r["bboxes"][t]) == gt_bboxes[c][t].shape[0]
            assert gt_ids[c][t].tolist() == r["obj_ids"][t] and gt_labels[c][t].tolist() == r["labels"][t].tolist()
            assert np.array_equal(gt_bboxes[c][t].cpu().numpy(), T.boxes_target(r["bboxes"][t], H0, W0, C.SIZE, C.DIVISOR, r["flip"]))
            for j in range(len(r["segms"][t])):                        # the annotations' masks are their boxes' rectangles
                dense = C._rect(H0, W0, *anns[r["obj_ids"][t][j]]["bboxes"][r["frame_ids"][t]]).astype(np.uint8)
                assert np.array_equal(gt_masks[c][t][j].cpu().numpy(), R.mask_target(dense, p, C.SIZE, C.DIVISOR, r["flip"])), (c, t, j)
    # ... and through one training step
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
    losses = train_step(nl, opt, tuple(batch))
    vals = {k: float(v) for k, v in losses.items()}
    print("\n" + "  ".join(f"{k} {v:.4f}" for k, v in vals.items()))
    assert all(np.isfinite(v) for v in vals.values()), vals
