"""ExtraAugmentation (datasets/extra_aug.py: PhotoMetricDistortion, Expand, RandomCrop) split the way the rest of the training data is: the host
draws the parameters -- scalar work over a handful of boxes, with the reference's numpy calls in the reference's order, so a seeded run draws
what the reference draws -- and the device does the per-pixel work inside the batch kernels (csrc/extra_aug.hip; datasets.py is the caller).
Nothing at source resolution is written on the way to the batch.  INTEGRATION.md section 22 is the contract, with the six findings about the
reference this module reproduces:
  1. the augmented image is assigned back into a uint8 array, a C cast that truncates toward zero and keeps the low 8 bits (300.7 -> 44,
     -5.5 -> 251): cast="reference"; cast="clip" saturates instead;
  2. RandomCrop zeroes everything outside the patch in an image of unchanged size but shifts the boxes by the patch origin:
     crop_boxes="reference"; crop_boxes="aligned" leaves the (clipped) boxes where the image is;
  3. the patch origin is uniform(low=w - new_w, high=1.0);
  4. every frame of a pair draws its own augmentation, the clip's one flip is drawn after both (YTVISTrainSet does that);
  5. RandomCrop on a frame without boxes raises in the reference; here such a frame skips RandomCrop and draws nothing for it;
  6. Expand fills with mean[::-1] in the image's BGR order, after the photometric step, and moves the boxes through
     rint((b + (left, top, left, top)) / ratio) in float64, back to float32.
"""
import numpy as np

PHOTO_DEFAULTS = dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18)
EXPAND_DEFAULTS = dict(mean=(0, 0, 0), to_rgb=True, ratio_range=(1, 4))
CROP_DEFAULTS = dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3)


class AugParams:
    """What one frame's augmentation drew.  Identity values where a step was not taken, so the device applies every step unconditionally.
        photo           the BGR -> HSV -> BGR round trip runs (PhotoMetricDistortion is configured; the round trip itself changes bytes)
        delta           brightness delta (0.0: not drawn)
        contrast_mode   the reference's `mode`: 1 multiplies by alpha before the round trip, 0 after it
        alpha           contrast factor (1.0: not drawn)
        saturation      factor on S (1.0: not drawn)
        hue             delta on H in degrees (0.0: not drawn)
        perm            output channel c is channel perm[c] ((0, 1, 2): not drawn)
        expand          None or (ratio, left, top); canvas = (int(H0 * ratio), int(W0 * ratio))
        fill            Expand's fill per BGR channel
        crop            None or the patch (x0, y0, x1, y1), ends exclusive
        cast            "reference" | "clip"
    """
    __slots__ = ("H0", "W0", "photo", "delta", "contrast_mode", "alpha", "saturation", "hue", "perm", "expand", "canvas", "fill", "crop", "cast")

    def __init__(self, H0, W0, cast="reference"):
        self.H0, self.W0, self.cast = int(H0), int(W0), cast
        self.photo, self.delta, self.contrast_mode, self.alpha, self.saturation, self.hue, self.perm = False, 0.0, 0, 1.0, 1.0, 0.0, (0, 1, 2)
        self.expand, self.canvas, self.fill, self.crop = None, None, (0.0, 0.0, 0.0), None

    def __repr__(self):
        return "AugParams(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


def identity_params(H0, W0):
    return AugParams(H0, W0)


def box_overlaps(patch, boxes):
    """IoU of one box with float32 [k, 4] boxes in float32, ends inclusive (+1), in datasets/bbox_overlaps.py's operation order."""
    a = np.asarray(patch, dtype=np.float32).reshape(4)
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    area_a = (a[2] - a[0] + 1) * (a[3] - a[1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    xs, ys = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    xe, ye = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.maximum(xe - xs + 1, 0) * np.maximum(ye - ys + 1, 0)
    return (inter / (area_a + area_b - inter)).astype(np.float32)


class ExtraAugmentation:
    """The reference's constructor: each of photo_metric_distortion / expand / random_crop is None (off) or the dict of that transform's own
    keywords (an empty dict takes its defaults).  crop_boxes and cast: see the module."""

    def __init__(self, photo_metric_distortion=None, expand=None, random_crop=None, crop_boxes="reference", cast="reference"):
        if crop_boxes not in ("reference", "aligned"):
            raise ValueError(f"ExtraAugmentation: crop_boxes={crop_boxes!r}")
        if cast not in ("reference", "clip"):
            raise ValueError(f"ExtraAugmentation: cast={cast!r}")
        self.crop_boxes, self.cast = crop_boxes, cast
        self.photo = self.expand = self.crop = None
        for name, given, defaults in (("photo", photo_metric_distortion, PHOTO_DEFAULTS), ("expand", expand, EXPAND_DEFAULTS),
                                      ("crop", random_crop, CROP_DEFAULTS)):
            if given is None:
                continue
            unknown = set(given) - set(defaults)
            if unknown:
                raise TypeError(f"ExtraAugmentation: {name} got unexpected keywords {sorted(unknown)}")
            setattr(self, name, {**defaults, **given})
        if self.expand is not None:
            mean = tuple(self.expand["mean"])
            self.expand["fill"] = mean[::-1] if self.expand["to_rgb"] else mean
        if self.crop is not None:
            self.crop["modes"] = (1, *self.crop["min_ious"], 0)

    def sample(self, H0, W0, boxes, labels, obj_ids, segms, rng=None):
        """Draws one frame's augmentation: -> (AugParams, boxes float32 [G', 4], labels [G'], obj_ids list, segms list) as the reference leaves
        them.  rng: a numpy.random.RandomState; None draws from numpy's global stream, as the reference does.
        A frame without boxes skips RandomCrop without drawing anything for it (the reference raises there: overlaps.min() of nothing)."""
        R = np.random if rng is None else rng
        p = AugParams(H0, W0, self.cast)
        boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
        labels, obj_ids, segms = np.asarray(labels), list(obj_ids), list(segms)
        h, w = int(H0), int(W0)
        if self.photo is not None:
            c = self.photo
            p.photo = True
            if R.randint(2):
                p.delta = float(R.uniform(-c["brightness_delta"], c["brightness_delta"]))
            p.contrast_mode = int(R.randint(2))
            if p.contrast_mode == 1 and R.randint(2):
                p.alpha = float(R.uniform(*c["contrast_range"]))
            if R.randint(2):
                p.saturation = float(R.uniform(*c["saturation_range"]))
            if R.randint(2):
                p.hue = float(R.uniform(-c["hue_delta"], c["hue_delta"]))
            if p.contrast_mode == 0 and R.randint(2):
                p.alpha = float(R.uniform(*c["contrast_range"]))
            if R.randint(2):
                p.perm = tuple(int(v) for v in R.permutation(3))
        if self.expand is not None:
            c = self.expand
            p.fill = tuple(float(v) for v in c["fill"])
            if not R.randint(2):
                ratio = R.uniform(*c["ratio_range"])
                left = int(R.uniform(0, w * ratio - w))
                top = int(R.uniform(0, h * ratio - h))
                p.expand, p.canvas = (float(ratio), left, top), (int(h * ratio), int(w * ratio))
                boxes = np.rint((boxes + np.tile((left, top), 2)) / ratio).astype(boxes.dtype)
        if self.crop is not None and len(boxes):
            c = self.crop
            while p.crop is None:
                mode = R.choice(c["modes"])
                if mode == 1:
                    break
                for _ in range(50):
                    new_w = R.uniform(c["min_crop_size"] * w, w)
                    new_h = R.uniform(c["min_crop_size"] * h, h)
                    if new_h / new_w < 0.5 or new_h / new_w > 2:
                        continue
                    left = R.uniform(w - new_w)              # low = w - new_w, high = 1.0
                    top = R.uniform(h - new_h)
                    patch = np.array((int(left), int(top), int(left + new_w), int(top + new_h)))
                    if box_overlaps(patch, boxes).min() < mode:
                        continue
                    center = (boxes[:, :2] + boxes[:, 2:]) / 2
                    keep = (center[:, 0] > patch[0]) * (center[:, 1] > patch[1]) * (center[:, 0] < patch[2]) * (center[:, 1] < patch[3])
                    if not keep.any():
                        continue
                    boxes, labels = boxes[keep], labels[keep]
                    obj_ids = [v for v, k in zip(obj_ids, keep) if k]
                    segms = [v for v, k in zip(segms, keep) if k]
                    boxes[:, 2:] = boxes[:, 2:].clip(max=patch[2:])
                    boxes[:, :2] = boxes[:, :2].clip(min=patch[:2])
                    if self.crop_boxes == "reference":
                        boxes -= np.tile(patch[:2], 2)
                    p.crop = tuple(int(v) for v in patch)
                    break
        return p, boxes, labels, obj_ids, segms


def from_config(extra_aug, crop_boxes="reference", cast="reference"):
    """None, an ExtraAugmentation, or the reference's dict(photo_metric_distortion=..., expand=..., random_crop=...)."""
    if extra_aug is None or isinstance(extra_aug, ExtraAugmentation):
        return extra_aug
    return ExtraAugmentation(**extra_aug, crop_boxes=crop_boxes, cast=cast)


def config_from_names(names, mean, to_rgb=True):
    """'photo,expand,crop' (any subset, a string or a list) -> the reference's extra_aug dict with, for each, the settings its training configs
    carry (datasets/config.py: expand=dict(mean=..., to_rgb=True, ratio_range=(1, 3)), random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9),
    min_crop_size=0.3)); photo takes PhotoMetricDistortion's own defaults.  Nothing named: None."""
    if isinstance(names, str):
        names = [n.strip() for n in names.split(",") if n.strip()]
    unknown = set(names) - {"photo", "expand", "crop"}
    if unknown:
        raise ValueError(f"extra_aug: {sorted(unknown)} is not one of photo, expand, crop")
    cfg = {}
    if "photo" in names:
        cfg["photo_metric_distortion"] = dict(PHOTO_DEFAULTS)
    if "expand" in names:
        cfg["expand"] = dict(mean=tuple(mean), to_rgb=bool(to_rgb), ratio_range=(1, 3))
    if "crop" in names:
        cfg["random_crop"] = dict(CROP_DEFAULTS)
    return cfg or None
