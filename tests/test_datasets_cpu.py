"""stmask_amd.datasets without a device: YTVISTrainSet's parse and sampling on a hand-built annotation dict, the numpy restatement of the transforms
held to closed-form cases, and the derived bound between the kernel's normalisation and mmcv's fp32 evaluations."""
import random

import numpy as np
import pytest

import train_data_cases as C
import train_data_restate as R
from stmask_amd import datasets


@pytest.fixture(scope="module")
def ds():
    return datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, size_divisor=C.DIVISOR)


# ------------------------------------------------------------------------------------------------------------------ the dataset
def test_img_ids_keep_only_frames_with_a_box(ds):
    # video 10: frame 2 has no objects; frame 3 keeps track 101 (103 has area 0 there).  Video 20: the crowd track alone would not keep a frame.
    assert ds.img_ids == [(10, 0), (10, 1), (10, 3), (10, 4), (20, 0), (20, 1), (20, 2), (30, 0)]
    assert len(ds) == 8
    assert ds.vid_ids == [10, 20, 30] and ds.cat2label == {7: 1, 3: 2, 12: 3}


def test_boxes_are_float32_of_the_double_expression(ds):
    a = ds.get_ann_info(10, 0)
    want = np.array([[3.3, 2.2, 3.3 + 10.7 - 1, 2.2 + 8.1 - 1], [30.0, 20.0, 30.0 + 12.5 - 1, 20.0 + 9.0 - 1]], dtype=np.float32)
    assert a["bboxes"].dtype == np.float32 and a["bboxes"].tobytes() == want.tobytes()
    assert a["labels"].dtype == np.int64 and a["labels"].tolist() == [2, 1] and a["obj_ids"] == [101, 102]
    # bbox None (101 in frame 2, 102 from frame 2 on), area 0 (103 in frame 3)
    assert ds.get_ann_info(10, 2)["bboxes"].shape == (0, 4) and ds.get_ann_info(10, 2)["segms"] == []
    assert ds.get_ann_info(10, 3)["obj_ids"] == [101]
    assert ds.get_ann_info(10, 4)["obj_ids"] == [101, 103] and ds.get_ann_info(10, 4)["labels"].tolist() == [2, 3]


def test_a_crowd_annotation_leaves_masks_and_boxes_aligned(ds):
    a = ds.get_ann_info(20, 1)
    assert a["obj_ids"] == [201] and len(a["segms"]) == len(a["bboxes"]) == len(a["labels"]) == 1
    assert isinstance(a["segms"][0]["counts"], str)                 # kept as the JSON gave it


def test_sample_ref_never_returns_the_frame_itself_when_a_neighbour_exists(ds):
    random.seed(3)
    seen = {idx: set() for idx in ds.img_ids}
    for _ in range(200):
        for idx in ds.img_ids:
            (ref,) = ds.sample_ref(idx)
            seen[idx].add(ref)
    assert seen[(10, 0)] == {1}                  # +-2: frames 1 and 2, and frame 2 is not in img_ids
    assert seen[(10, 1)] == {0, 3}
    assert seen[(10, 3)] == {1, 4} and seen[(10, 4)] == {3}
    assert seen[(20, 1)] == {0, 2} and seen[(20, 0)] == {1, 2}
    assert seen[(30, 0)] == {0}                  # no neighbour: the frame itself


def test_the_pair_is_sorted_and_frame_id_is_the_later_frame(ds):
    random.seed(0)
    np.random.seed(0)
    for _ in range(20):
        for i, (vid, f) in enumerate(ds.img_ids):
            r = ds[i]
            a, b = r["frame_ids"]
            assert a <= b and f in (a, b) and r["video_id"] == vid
            assert r["img_meta"]["frame_id"] == b and r["img_meta"]["is_first"] == (b == 0)
            assert r["img_meta"]["flip"] == r["flip"] and r["img_meta"]["pad_shape"] == (32, 64, 3) and r["img_meta"]["img_shape"] == (24, 40, 3)
            for t, fr in enumerate(r["frame_ids"]):
                assert np.array_equal(r["frames"][t], C.frame_reader()(f"v{vid}/{fr:05d}.jpg"))
                assert r["obj_ids"][t] == ds.get_ann_info(vid, fr)["obj_ids"] and len(r["segms"][t]) == len(r["bboxes"][t])
    r = ds[ds.img_ids.index((30, 0))]
    assert r["frame_ids"] == [0, 0] and r["size"] == (50, 30)
    sf = r["img_meta"]["scale_factor"]
    assert sf.dtype == np.float32 and sf.tobytes() == np.array([40 / 30, 24 / 50, 40 / 30, 24 / 50], dtype=np.float32).tobytes()


def test_flip_frequency_under_a_seeded_generator():
    half = datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, flip_ratio=0.5)
    np.random.seed(11)
    random.seed(11)
    flips = [half[i % len(half)]["flip"] for i in range(400)]
    np.random.seed(11)
    want = [bool(np.random.rand() < 0.5) for _ in range(400)]      # one draw per clip, nothing else reads np.random
    assert flips == want and 150 < sum(flips) < 250
    never = datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, flip_ratio=0.0)
    always = datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, flip_ratio=1.0)
    assert not any(never[i]["flip"] for i in range(len(never))) and all(always[i]["flip"] for i in range(len(always)))


def test_out_of_scope_settings_are_refused():
    with pytest.raises(ValueError):
        datasets.YTVISTrainSet(C.annotations(), img_scale=[(640, 360), (1280, 720)])
    with pytest.raises(ValueError):
        datasets.YTVISTrainSet(C.annotations(), flip_ratio=1.5)
    with pytest.raises(datasets.StmError):
        datasets.collate_device([], device="cpu")


def test_the_loader_drops_the_last_short_batch_and_reshuffles_by_seed(ds):
    a = datasets.TrainLoader(ds, 3, seed=5)
    b = datasets.TrainLoader(ds, 3, seed=5)
    assert len(a) == 8 // 3 == 2
    assert a.order(0) == b.order(0) and sorted(a.order(0)) == list(range(8)) and a.order(0) != a.order(1)
    assert datasets.TrainLoader(ds, 3, shuffle=False).order(4) == list(range(8))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_identity_size_returns_the_mask():
    for name, c in C.run_lists(24, 40).items():
        m = R.dense(c, 24, 40)
        out = R.mask_target(m, C.SIZE, C.DIVISOR, False)
        assert np.array_equal(out[:24, :40], m) and not out[24:].any() and not out[:, 40:].any(), name


def test_restatement_factor_two_picks_every_second_pixel():
    for name, c in C.run_lists(48, 80).items():
        m = R.dense(c, 48, 80)
        assert np.array_equal(R.resize_nearest(m, C.SIZE), m[::2, ::2]), name


def test_restatement_upscaling_by_two_duplicates_pixels():
    rng = np.random.default_rng(0)
    m = (rng.random((12, 20)) < 0.5).astype(np.uint8)
    assert np.array_equal(R.resize_nearest(m, C.SIZE), np.repeat(np.repeat(m, 2, 0), 2, 1))


def test_restatement_full_and_empty_masks_survive_every_size():
    for H0, W0 in C.SOURCES + [(720, 1280)]:
        lists = C.run_lists(H0, W0)
        for flip in (False, True):
            full = R.mask_target(R.dense(lists["full"], H0, W0), C.SIZE, C.DIVISOR, flip)
            assert full[:24, :40].all() and full.sum() == 24 * 40
            assert not R.mask_target(R.dense(lists["empty"], H0, W0), C.SIZE, C.DIVISOR, flip).any()


def test_restatement_flip_of_a_left_half_mask_is_the_right_half():
    for H0, W0 in [(24, 40), (48, 80)]:
        m = np.zeros((H0, W0), dtype=np.uint8)
        m[:, :W0 // 2] = 1
        out = R.mask_target(m, C.SIZE, C.DIVISOR, True)
        assert not out[:24, :20].any() and out[:24, 20:40].all() and not out[:, 40:].any()


def test_restatement_dense_decode_and_zero_length_runs():
    m = R.dense([2, 0, 1, 3, 0, 0, 0], 2, 3)                      # zeros 2, ones 0, zeros 1, ones 3: column-major
    assert m.tolist() == [[0, 0, 1], [0, 1, 1]]
    with pytest.raises(ValueError):
        R.dense([2, 3], 2, 3)
    assert C.counts_of_mask(m) == [3, 3] and C.counts_of_mask(np.ones((2, 2))) == [0, 4]


def test_restatement_boxes_closed_form():
    # identity size, no flip: x / Wp, y / Hp; flipped: x1' = w - x2 - 1
    b = np.array([[4.0, 6.0, 12.0, 18.0]], dtype=np.float32)
    assert R.boxes_target(b, 24, 40, C.SIZE, C.DIVISOR, False).tolist() == [[4 / 64, 6 / 32, 12 / 64, 18 / 32]]
    assert R.boxes_target(b, 24, 40, C.SIZE, C.DIVISOR, True).tolist() == [[27 / 64, 6 / 32, 35 / 64, 18 / 32]]
    assert R.boxes_target(np.array([[-5.0, -5.0, 99.0, 99.0]], np.float32), 24, 40, C.SIZE, C.DIVISOR, False).tolist() == [[0.0, 0.0, 40 / 64, 24 / 32]]


# ------------------------------------------------------------------------------------------------------------------ the normalisation bound
def test_normalisation_stays_within_the_derived_bound_of_mmcv_fp32():
    """The kernel evaluates k = fl32((v - m) / s) with m, s and the arithmetic in double: one rounding, |k - x| <= u |x| with x the exact value
    and u = 2^-24.  mmcv's imnormalize works in fp32 on m32 = fl32(m), s32 = fl32(s): either A = fl32(fl32(v - m32) / s32) or
    B = fl32(fl32(v - m32) * fl32(1 / s32)).  With m32 = m (1 + d_m), s32 = s (1 + d_s) and one factor (1 + d_i), |d| <= u, per operation:
        A = ((v - m) - m d_m) (1 + d_1) (1 + d_2) / (s (1 + d_s))          => |A - x| <= 3 u |x| + u m / s      (+ O(u^2))
        B has one rounding more (the reciprocal)                            => |B - x| <= 4 u |x| + u m / s      (+ O(u^2))
    so |A - k| <= u (4 |x| + m / s) and |B - k| <= u (5 |x| + m / s); the O(u^2) terms (and the 2^-53 roundings of the double evaluation) are
    covered by a factor 1 + 2^-20.  Over v in 0..255 the bound peaks in the third channel at v = 255: u (5 * 2.640 + 1.804) < 9.0e-7."""
    u = 2.0 ** -24
    slack = 1.0 + 2.0 ** -20
    worst, worst_bound = 0.0, 0.0
    for c in range(3):
        m, s = C.MEAN[c], C.STD[c]
        m32, s32 = np.float32(m), np.float32(s)
        r32 = np.float32(1.0) / s32
        for v in range(256):
            x = abs((v - m) / s)
            k = np.float32((np.float64(v) - np.float64(m)) / np.float64(s))
            d = np.float32(v) - m32
            a, b = d / s32, d * r32
            assert a.dtype == b.dtype == np.float32
            bound_a, bound_b = u * (4 * x + m / s) * slack, u * (5 * x + m / s) * slack
            assert abs(float(a) - float(k)) <= bound_a, (c, v, float(a), float(k))
            assert abs(float(b) - float(k)) <= bound_b, (c, v, float(b), float(k))
            worst = max(worst, abs(float(a) - float(k)), abs(float(b) - float(k)))
            worst_bound = max(worst_bound, bound_b)
    print(f"\nlargest |mmcv fp32 - kernel| over 256 x 3 inputs: {worst:.3e}; derived bound {worst_bound:.3e}")
    assert worst <= worst_bound < 9.0e-7
