"""ExtraAugmentation without a GPU: the colour rule in closed form, the cast against numpy's own, ExtraAugmentation.sample + the numpy
restatement against runs of the reference's own code (tests/golden/extra_aug_cases.npz, written by tests/golden/gen_extra_aug.py), the draw order
in YTVISTrainSet.__getitem__, the options, the package-private binding of csrc/extra_aug.h, the refusals that launch nothing, and the compiler's
resource report for csrc/extra_aug.hip."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import abi_header
import extra_aug_restate as R
from kernel_resources import kernel_resources
import train_data_cases as C
from conftest import GOLDEN
from stmask_amd import _lib, datasets
from stmask_amd import extra_aug as EA
from stmask_amd._lib import StmError

ALL_ON = dict(photo_metric_distortion=dict(), expand=dict(mean=C.MEAN, to_rgb=True, ratio_range=(1, 3)), random_crop=dict())


def fixture_cases():
    z = np.load(os.path.join(GOLDEN, "extra_aug_cases.npz"), allow_pickle=False)
    configs = json.loads(str(z["configs_json"]))
    return [dict(seed=int(z["seeds"][i]), config=configs[int(z["configs"][i])], **{k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")})
            for i in range(len(z["seeds"]))]


CASES = fixture_cases()


def sample_case(c, rng=None, **options):
    """The package's draw for a fixture case, from numpy's global stream seeded as the reference's run was (or from `rng`)."""
    if rng is None:
        np.random.seed(c["seed"])
    aug = EA.ExtraAugmentation(**c["config"], **options)
    return aug.sample(c["img"].shape[0], c["img"].shape[1], c["boxes"].copy(), c["labels"], c["ids"].tolist(), list(c["masks"]), rng=rng)


# ---- the colour rule ----------------------------------------------------------------------------------------------------------------------
def test_pure_colours_and_grey_in_closed_form():
    px = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [77, 77, 77], [0, 0, 0]], dtype=np.float32)        # BGR: red, green, blue, grey, black
    hsv = R.bgr2hsv(px)
    assert hsv.dtype == np.float32
    assert hsv.tolist() == [[0.0, 1.0, 255.0], [120.0, 1.0, 255.0], [240.0, 1.0, 255.0], [0.0, 0.0, 77.0], [0.0, 0.0, 0.0]]
    assert np.array_equal(R.hsv2bgr(hsv), px)
    # s == 0 returns v whatever the hue says
    assert R.hsv2bgr(np.array([[123.0, 0.0, 50.0]], dtype=np.float32)).tolist() == [[50.0, 50.0, 50.0]]


def test_hue_360_is_hue_0_and_a_negative_hue_wraps():
    """6.f / 360.f rounds up, so 360 * hscale is a little above 6: the hue wraps by -6 into sector 0 with a fraction of 5e-7, not exactly 0."""
    at = lambda h: R.hsv2bgr(np.array([[h, 0.5, 200.0]], dtype=np.float32))      # noqa: E731
    assert at(0.0).tolist() == [[100.0, 100.0, 200.0]]
    assert np.float32(360.0) * R.HSCALE > 6 and np.abs(at(360.0) - at(0.0)).max() < 1e-3
    assert np.abs(at(-60.0) - at(300.0)).max() < 1e-3 and np.abs(at(420.0) - at(60.0)).max() < 1e-3
    assert np.abs(at(60.0) - np.float32([100.0, 200.0, 200.0])).max() < 1e-3      # sector 1, h = 0: (tab[1], tab[0], tab[2])
    assert np.abs(at(300.0) - np.float32([200.0, 100.0, 200.0])).max() < 1e-3     # sector 5, h = 0: (tab[2], tab[1], tab[0])


def test_round_trip_within_1e_3():
    rng = np.random.default_rng(3)
    px = rng.uniform(0, 255, (4096, 3)).astype(np.float32)
    px[:64] = np.floor(px[:64])
    back = R.hsv2bgr(R.bgr2hsv(px))
    assert np.abs(back - px).max() < 1e-3


# ---- the cast -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cast_rule_is_numpys_own_assignment(dtype):
    """300.7 -> 44 and -5.5 -> 251: truncation toward zero, then the low 8 bits.  Checked against this machine's numpy over [-600, 900]."""
    x = np.arange(-600 * 8, 900 * 8 + 1, dtype=np.float64) / 8
    x = np.concatenate([x, [300.7, -5.5, 255.999, 256.0, -0.999, -1.0]]).astype(dtype)
    own = np.zeros(x.shape, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        own[...] = x
        assert np.array_equal(x.astype(np.uint8), own)
    assert np.array_equal(R.cast_reference(x), own)
    assert R.cast_reference(np.array([300.7, -5.5])).tolist() == [44, 251]
    assert R.cast_clip(np.array([300.7, -5.5, 44.9, 255.5])).tolist() == [255, 0, 44, 255]


# ---- sample() + restatement against the reference's own runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_sample_and_restatement_reproduce_the_reference(i):
    c = CASES[i]
    p, boxes, labels, ids, masks = sample_case(c)
    assert np.random.random_sample() == float(c["tail"])                      # numpy's stream stands where the reference left it
    assert np.array_equal(R.augmented_source(c["img"], p), c["out_img"])
    got = np.stack([R.augmented_mask(m, p) for m in masks])
    assert got.dtype == np.uint8 and np.array_equal(got, c["out_masks"])
    assert boxes.dtype == np.float32 and boxes.shape == c["out_boxes"].shape
    assert np.array_equal(boxes.view(np.int32), c["out_boxes"].view(np.int32))
    assert np.array_equal(labels, c["out_labels"]) and ids == c["out_ids"].tolist()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_a_random_state_draws_what_the_global_stream_draws(i):
    c = CASES[i]
    a, b = sample_case(c), sample_case(c, rng=np.random.RandomState(c["seed"]))
    assert repr(a[0]) == repr(b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]


def test_the_fixture_reaches_wrapping_values_and_every_transform():
    wrapped = taken = cropped = dropped = 0
    for c in CASES:
        p, boxes, *_ = sample_case(c)
        pre = R.crop_pixels(R.expand_pixels(R.photometric(c["img"], p), p, np.asarray(p.fill, dtype=np.float32)), p)
        wrapped = max(wrapped, ((pre < 0) | (pre >= 256)).mean())
        taken += p.expand is not None
        cropped += p.crop is not None
        dropped += len(boxes) < len(c["boxes"])
    assert wrapped > 0.01 and taken and cropped and dropped


def test_a_frame_without_boxes_skips_the_crop_and_draws_nothing_for_it():
    aug = EA.ExtraAugmentation(random_crop=dict())
    rs = np.random.RandomState(5)
    before = rs.get_state()[1].copy()
    p, boxes, labels, ids, segms = aug.sample(24, 40, np.zeros((0, 4), np.float32), np.zeros(0, np.int64), [], [], rng=rs)
    assert p.crop is None and boxes.shape == (0, 4) and ids == [] and np.array_equal(rs.get_state()[1], before)


# ---- the options ----------------------------------------------------------------------------------------------------------------------------
def test_crop_boxes_aligned_leaves_the_clipped_boxes_where_the_image_is():
    seen = 0
    for c in CASES:
        p, ref_boxes, _, ids, _ = sample_case(c)
        q, boxes, _, ids2, _ = sample_case(c, crop_boxes="aligned")
        assert repr(p) == repr(q) and ids == ids2
        if p.crop is None:
            assert np.array_equal(boxes, ref_boxes)
            continue
        seen += 1
        x0, y0, x1, y1 = p.crop
        assert (boxes[:, 0] >= x0).all() and (boxes[:, 1] >= y0).all() and (boxes[:, 2] <= x1).all() and (boxes[:, 3] <= y1).all()
        assert np.array_equal((boxes - np.tile([x0, y0], 2)).astype(np.float32), ref_boxes)
        assert x0 + y0 > 0 and not np.array_equal(boxes, ref_boxes)
    assert seen >= 2


def test_cast_clip_saturates_where_the_reference_wraps():
    differs = 0
    for c in CASES:
        p = sample_case(c, cast="clip")[0]
        assert p.cast == "clip"
        pre = R.crop_pixels(R.expand_pixels(R.photometric(c["img"], p), p, np.asarray(p.fill, dtype=np.float32)), p)
        got = R.augmented_source(c["img"], p)
        assert np.array_equal(got, np.clip(pre, 0, 255).astype(np.uint8))
        differs += not np.array_equal(got, c["out_img"])
    assert differs
    with pytest.raises(ValueError, match="cast="):
        EA.ExtraAugmentation(cast="round")
    with pytest.raises(ValueError, match="crop_boxes="):
        EA.ExtraAugmentation(crop_boxes="moved")
    with pytest.raises(TypeError, match="unexpected keywords"):
        EA.ExtraAugmentation(expand=dict(ratio=2))


def test_constructor_takes_the_reference_keywords_and_defaults():
    a = EA.ExtraAugmentation()
    assert a.photo is None and a.expand is None and a.crop is None
    a = EA.ExtraAugmentation(photo_metric_distortion={}, expand={}, random_crop={})
    assert a.photo == dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
    assert a.expand["ratio_range"] == (1, 4) and a.expand["fill"] == (0, 0, 0) and a.crop["modes"] == (1, 0.1, 0.3, 0.5, 0.7, 0.9, 0)
    assert EA.ExtraAugmentation(expand=dict(mean=(1, 2, 3), to_rgb=True)).expand["fill"] == (3, 2, 1)
    assert EA.ExtraAugmentation(expand=dict(mean=(1, 2, 3), to_rgb=False)).expand["fill"] == (1, 2, 3)


# ---- the dataset's draw order --------------------------------------------------------------------------------------------------------------------
def dataset(**kw):
    return datasets.YTVISTrainSet(C.annotations(), frame_reader=C.frame_reader(), img_scale=C.SIZE, **kw)


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_both_augmentations_are_drawn_before_the_flip(seed):
    ds = dataset(extra_aug=ALL_ON)
    for i in range(len(ds)):
        seed_all(seed)
        rec = ds[i]
        tail = np.random.random_sample()
        # the reference's order: the pair (Python's random), frame 0's augmentation, frame 1's, then the flip
        seed_all(seed)
        vid, frame_id = ds.img_ids[i]
        clip = sorted(ds.sample_ref((vid, frame_id)) + [frame_id])
        assert clip == rec["frame_ids"]
        aug = EA.ExtraAugmentation(**ALL_ON)
        for t, f in enumerate(clip):
            a = ds.get_ann_info(vid, f)
            H0, W0 = rec["frames"][t].shape[:2]
            p, boxes, labels, ids, segms = aug.sample(H0, W0, a["bboxes"], a["labels"], a["obj_ids"], a["segms"])
            assert repr(p) == repr(rec["aug"][t])
            assert np.array_equal(boxes, rec["bboxes"][t]) and np.array_equal(labels, rec["labels"][t])
            assert ids == rec["obj_ids"][t] and segms == rec["segms"][t] and len(segms) == len(boxes)
        assert bool(np.random.rand() < ds.flip_ratio) == rec["flip"] == rec["img_meta"]["flip"]
        assert np.random.random_sample() == tail


def test_extra_aug_none_draws_and_yields_what_it_did_without_the_argument():
    plain, none = dataset(), dataset(extra_aug=None)
    for i in range(len(plain)):
        seed_all(7)
        a = plain[i]
        tail_a = (np.random.random_sample(), random.random())
        seed_all(7)
        b = none[i]
        assert (np.random.random_sample(), random.random()) == tail_a
        seed_all(7)
        plain.sample_ref(plain.img_ids[i])
        flip = bool(np.random.rand() < 0.5)                       # the one numpy draw of a record
        assert (np.random.random_sample(), random.random()) == tail_a and flip == a["flip"]
        assert sorted(a) == sorted(b) == ["bboxes", "flip", "frame_ids", "frames", "img_meta", "img_scale", "labels", "mean", "obj_ids", "segms",
                                          "size", "size_divisor", "std", "to_rgb", "video_id"]
        assert a["flip"] == b["flip"] and a["frame_ids"] == b["frame_ids"] and a["segms"] == b["segms"] and a["obj_ids"] == b["obj_ids"]
        assert all(np.array_equal(x, y) for k in ("frames", "bboxes", "labels") for x, y in zip(a[k], b[k]))


def test_the_dataset_does_not_change_its_annotations():
    ds = dataset(extra_aug=ALL_ON)
    before = [ds.get_ann_info(*idx)["bboxes"].copy() for idx in ds.img_ids]
    seed_all(0)
    for i in range(len(ds)):
        ds[i]
    assert all(np.array_equal(b, ds.get_ann_info(*idx)["bboxes"]) for b, idx in zip(before, ds.img_ids))


# ---- the private binding ----------------------------------------------------------------------------------------------------------------------
def test_descriptor_mirror_has_the_headers_fields_and_size():
    fields = abi_header.struct_field_names("extra_aug.h", "stm_aug_desc")
    assert fields == [f[0] for f in _lib.AugDesc._fields_]
    size = ctypes.CDLL(_lib.LIB_PATH).stm_aug_struct_bytes
    size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int]
    assert size(0) == ctypes.sizeof(_lib.AugDesc) == 112 and size(1) == 0


# ---- refusals: decided from the arguments and the host descriptors, before any launch ----------------------------------------------------------
FAKE = 0x1000   # never dereferenced: every case below is refused first
EINVAL, ENULL = -1, -2


def host_desc(**kw):
    d = (_lib.AugDesc * 1)()
    v = dict(ptr=FAKE, row_stride_bytes=120, H0=24, W0=40, Hc=24, Wc=40, top=0, left=0, x0=0, y0=0, x1=40, y1=24)
    v.update(kw)
    for k, x in v.items():
        setattr(d[0], k, x)
    d[0].perm[:] = kw.get("perm_", [0, 1, 2])
    return d


def frames_args(**kw):
    m3 = (ctypes.c_double * 3)(1, 1, 1)
    a = dict(host=host_desc(), dev=ctypes.c_void_p(FAKE), n=1, out=ctypes.c_void_p(FAKE), h=24, w=40, Hp=32, Wp=64, mean=m3, std=m3, to_rgb=1,
             stream=None)
    a.update(kw)
    return [a[k] for k in ("host", "dev", "n", "out", "h", "w", "Hp", "Wp", "mean", "std", "to_rgb", "stream")]


FRAME_REFUSALS = [
    (dict(host=None), ENULL, "must be non-NULL"),
    (dict(dev=None), ENULL, "must be non-NULL"),
    (dict(out=None), ENULL, "must be non-NULL"),
    (dict(mean=None), ENULL, "must be non-NULL"),
    (dict(n=-1), EINVAL, "bad sizes"),
    (dict(Hp=16), EINVAL, "bad sizes"),
    (dict(host=host_desc(ptr=None)), ENULL, "frame 0 has a NULL pointer"),
    (dict(host=host_desc(row_stride_bytes=119)), EINVAL, "bad source size 24x40 (row stride 119 bytes)"),
    (dict(host=host_desc(H0=0)), EINVAL, "bad source size"),
    (dict(host=host_desc(Hc=30, top=7)), EINVAL, "the canvas 30x40 does not hold the 24x40 source at (7, 0)"),
    (dict(host=host_desc(Wc=39)), EINVAL, "the canvas"),
    (dict(host=host_desc(left=-1)), EINVAL, "the canvas"),
    (dict(host=host_desc(x1=41)), EINVAL, "the patch (0, 0, 41, 24) is not inside"),
    (dict(host=host_desc(y0=5, y1=4)), EINVAL, "the patch"),
    (dict(host=host_desc(perm_=[0, 1, 3])), EINVAL, "perm[2]=3"),
]


@pytest.mark.parametrize("change,code,text", FRAME_REFUSALS, ids=[f"{i}-{t[2][:24].replace(' ', '_')}" for i, t in enumerate(FRAME_REFUSALS)])
def test_frames_refusals(change, code, text):
    with pytest.raises(StmError) as e:
        _lib.private_call("stm_aug_frames_u8_f32", *frames_args(**change))
    assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_source_and_masks_refusals():
    p = ctypes.c_void_p(FAKE)
    for args, code, text in [((None, p, p, None), ENULL, "must be non-NULL"), ((host_desc(), None, p, None), ENULL, "must be non-NULL"),
                             ((host_desc(), p, None, None), ENULL, "must be non-NULL"),
                             ((host_desc(ptr=None), p, p, None), ENULL, "frame 0 has a NULL pointer"),
                             ((host_desc(x0=-1), p, p, None), EINVAL, "the patch")]:
        with pytest.raises(StmError) as e:
            _lib.private_call("stm_aug_source_u8", *args)
        assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)
    base = dict(starts=p, off=p, n_runs=p, n_lists=1, mdesc=p, frame_of=p, adesc=p, n_frames=1, n=1, total=4, out=p, h=24, w=40, Hp=32, Wp=64, stream=None)
    for change, code, text in [(dict(frame_of=None), ENULL, "NULL argument"), (dict(adesc=None), ENULL, "NULL argument"),
                               (dict(out=None), ENULL, "NULL argument"), (dict(n_frames=0), EINVAL, "bad sizes"),
                               (dict(Wp=62), EINVAL, "must be a multiple of 4"), (dict(out=ctypes.c_void_p(FAKE + 2)), EINVAL, "4-byte aligned")]:
        with pytest.raises(StmError) as e:
            _lib.private_call("stm_aug_masks_u8", *{**base, **change}.values())
        assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)
    with pytest.raises(StmError, match="takes 4 arguments, got 3"):
        _lib.private_call("stm_aug_source_u8", None, None, None)


# ---- the kernels' resources --------------------------------------------------------------------------------------------------------------------
def test_aug_kernels_use_no_scratch_and_no_lds():
    seen = []
    for name, r in kernel_resources("extra_aug.hip").items():
        if any(k in name for k in ("aug_frames_kernel", "aug_masks_kernel", "aug_source_kernel")):
            seen.append(name)
            assert r.scratch == 0 and r.lds == 0, (name, r.scratch, r.lds)
    assert len(seen) == 3, seen
