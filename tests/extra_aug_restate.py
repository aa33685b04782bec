"""The yardstick of the ExtraAugmentation tests, in numpy: the colour rule (cv2.cvtColor BGR <-> HSV on float32, restated from OpenCV's scalar
path -- cv2 was not available to re-capture it), the uint8 cast of `imgs[i] = extra_aug(...)`, the pixel work of the three transforms as whole
arrays at source resolution (the path the device code never takes), and their composition with train_data_restate's frame_target / mask_target.
Every float operation is a float32 array operation with float32 scalars: one rounding each, as the kernel's.
Not a test module: imported by the ExtraAugmentation tests and by tests/golden/gen_extra_aug.py (whose mmcv stand-in these functions are)."""
import numpy as np

import train_data_restate as T

F = np.float32
EPS = F(np.finfo(np.float32).eps)
HSCALE = F(6.0) / F(360.0)


def bgr2hsv(img):
    """float32 [..., 3] BGR -> H in [0, 360], S, V."""
    img = np.asarray(img, dtype=np.float32)
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    d = v - vmin
    s = d / (np.abs(v) + EPS)
    k = (60.0 / (d + EPS).astype(np.float64)).astype(np.float32)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + F(120), (r - g) * k + F(240)))
    h = np.where(h < 0, h + F(360), h)
    out = np.stack([h, s, v], axis=-1)
    assert out.dtype == np.float32
    return out


_TAB = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv2bgr(img):
    img = np.asarray(img, dtype=np.float32)
    h, s, v = img[..., 0] * HSCALE, img[..., 1], img[..., 2]
    neg = h < 0                                  # if (h < 0) do h += 6 while (h < 0); else if (h >= 6) do h -= 6 while (h >= 6);
    big = h >= 6                                 # (a negative h that rounds up to 6.0 stays 6.0: sector 6 is caught below)
    m = neg
    while m.any():
        h = np.where(m, h + F(6), h)
        m = neg & (h < 0)
    m = big
    while m.any():
        h = np.where(m, h - F(6), h)
        m = big & (h >= 6)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(np.float32)
    bad = (sector < 0) | (sector > 5)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, F(0), h)
    one = F(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    idx = _TAB[sector]                                                  # [..., 3]
    out = np.take_along_axis(tab, idx, axis=-1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    assert out.dtype == np.float32
    return out


def cast_reference(x):
    """numpy's float -> uint8 assignment for the values an augmentation produces: truncate toward zero, keep the low 8 bits."""
    return (np.trunc(np.asarray(x, dtype=np.float64)).astype(np.int64) & 255).astype(np.uint8)


def cast_clip(x):
    return np.trunc(np.clip(np.asarray(x, dtype=np.float64), 0, 255)).astype(np.uint8)


def cast(x, how):
    return cast_reference(x) if how == "reference" else cast_clip(x)


def imresize_nearest(img, size):
    """cv2.resize(img, (w, h), interpolation=INTER_NEAREST) for [H, W] or [H, W, C]."""
    w, h = size
    return img[T.nearest_index(h, img.shape[0])][:, T.nearest_index(w, img.shape[1])]


def photometric(img, p):
    """PhotoMetricDistortion's pixel work on a float32 [H, W, 3] image with the drawn values of `p`."""
    x = np.asarray(img, dtype=np.float32).copy()
    if not p.photo:
        return x
    if p.delta != 0.0:
        x = x + F(p.delta)
    if p.contrast_mode == 1 and p.alpha != 1.0:
        x = x * F(p.alpha)
    x = bgr2hsv(x)
    if p.saturation != 1.0:
        x[..., 1] = x[..., 1] * F(p.saturation)
    if p.hue != 0.0:
        hh = x[..., 0] + F(p.hue)
        hh = np.where(hh > 360, hh - F(360), hh)
        hh = np.where(hh < 0, hh + F(360), hh)
        x[..., 0] = hh
    x = hsv2bgr(x)
    if p.contrast_mode == 0 and p.alpha != 1.0:
        x = x * F(p.alpha)
    return x[..., list(p.perm)]


def expand_pixels(img, p, fill):
    """Expand's pixel work on [H, W] or [H, W, 3]: the canvas filled with `fill`, the image pasted at (top, left), nearest resize back."""
    if p.expand is None:
        return img
    _, left, top = p.expand
    H0, W0 = img.shape[:2]
    canvas = np.empty((p.canvas[0], p.canvas[1]) + img.shape[2:], dtype=img.dtype)
    canvas[...] = np.asarray(fill).astype(img.dtype)
    canvas[top:top + H0, left:left + W0] = img
    return imresize_nearest(canvas, (W0, H0))


def crop_pixels(img, p):
    if p.crop is None:
        return img
    x0, y0, x1, y1 = p.crop
    out = np.zeros(img.shape, dtype=np.float64)
    out[y0:y1, x0:x1] = img[y0:y1, x0:x1]
    return out


def augmented_source(img, p):
    """uint8 [H0, W0, 3] -> the uint8 image the reference's `imgs[i] = extra_aug(imgs[i], ...)` leaves."""
    x = photometric(img, p)
    x = expand_pixels(x, p, np.asarray(p.fill, dtype=np.float64).astype(np.float32))
    x = crop_pixels(x, p)
    return cast(x, p.cast)


def augmented_mask(mask, p):
    """uint8 [H0, W0] dense mask -> the mask after Expand and RandomCrop, uint8."""
    m = expand_pixels(np.asarray(mask, dtype=np.uint8), p, 0)
    return np.asarray(crop_pixels(m, p)).astype(np.uint8)


def frame_target(img, p, size, divisor, flip, to_rgb, mean, std):
    return T.frame_target(augmented_source(img, p), size, divisor, flip, to_rgb, mean, std)


def mask_target(mask, p, size, divisor, flip):
    return T.mask_target(augmented_mask(mask, p), size, divisor, flip)
