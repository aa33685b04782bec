"""Inputs of the display fixtures (tests/golden/display_*.npz), rebuilt bit for bit from integers on any machine.

gen_display_golden.py feeds them to the reference's eval.prep_display; the tests feed the same inputs to stmask_amd.display.
Frames come from np.random.default_rng(seed).integers (a stream numpy keeps stable); the network input of reference mode is
((u - MEANS) / STD) in float64 rounded once to fp32; soft masks are uint8 k with value k / 256 (exact in fp32, 128 = 0.5).
Masks and detections are stored in the fixture, frames are not.
"""
import numpy as np

MEANS = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)

# name -> (mode, ori (H0, W0), img (h, w), pad (hp, wp), n rows, seed, full output stored)
CASES = {
    "src_empty_333x500": ("source", (333, 500), (360, 640), (384, 640), 0, 1, False),
    "src_one_480x854": ("source", (480, 854), (360, 640), (384, 640), 1, 2, False),
    "src_many_720x1280": ("source", (720, 1280), (360, 640), (384, 640), 28, 3, False),
    "src_crowd_333x500": ("source", (333, 500), (360, 640), (384, 640), 44, 4, False),
    "src_small_72x128": ("source", (72, 128), (90, 160), (96, 160), 7, 5, True),
    "ref_empty_360x640": ("reference", (720, 1280), (360, 640), (384, 640), 0, 6, False),
    "ref_one_360x640": ("reference", (480, 854), (360, 640), (384, 640), 1, 7, False),
    "ref_many_360x640": ("reference", (720, 1280), (360, 640), (384, 640), 28, 8, False),
    "ref_small_90x160": ("reference", (72, 128), (90, 160), (96, 160), 9, 9, True),
}


def meta(spec):
    _, ori, img, pad = spec[:4]
    return {"ori_shape": (ori[0], ori[1], 3), "img_shape": (img[0], img[1], 3), "pad_shape": (pad[0], pad[1], 3)}


def source_frame(spec):
    """uint8 [H0, W0, 3] (BGR, as preprocess.py takes its inputs)."""
    H0, W0 = spec[1]
    return np.random.default_rng(1000 + spec[5]).integers(0, 256, (H0, W0, 3), dtype=np.uint8)


def network_input(spec):
    """fp32 [3, hp, wp]: a frame of img size, normalised per channel, zero in the padding."""
    h, w = spec[2]
    hp, wp = spec[3]
    u = np.random.default_rng(2000 + spec[5]).integers(0, 256, (h, w, 3), dtype=np.uint8).astype(np.float64)
    x = np.zeros((3, hp, wp), dtype=np.float32)
    for c in range(3):
        x[c, :h, :w] = ((u[:, :, c] - MEANS[c]) / STD[c]).astype(np.float32)
    return x


def detections(spec):
    """Rows of one frame as the tracker leaves them: normalised boxes [n, 4] (relative to the padded input), scores, classes,
    box_ids (repeats included) and uint8 masks k [n, mh, mw] (value k / 256) at a quarter of the padded input.  Rows with a low
    score, rows whose box centre lies in the padding, masks touching the crop edge and plateaus of exactly 0.5 all occur."""
    n, seed = spec[4], spec[5]
    hp, wp = spec[3]
    mh, mw = hp // 4, wp // 4
    h, w = spec[2]
    s_h, s_w = h / hp, w / wp
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:mh, 0:mw].astype(np.int64)
    masks = np.zeros((n, mh, mw), dtype=np.uint8)
    boxes = np.zeros((n, 4), dtype=np.float32)
    for i in range(n):
        cx, cy = int(rng.integers(0, mw)), int(rng.integers(0, int(mh * s_h) + 2))
        if i % 7 == 3:                                        # touching the crop edge (bottom / right)
            cy, cx = int(mh * s_h) - 1, int(mw * s_w) - 1 - int(rng.integers(0, 4))
        rx, ry = int(rng.integers(3, max(4, mw // 3))), int(rng.integers(3, max(4, mh // 3)))
        d = (xx - cx) ** 2 * ry * ry + (yy - cy) ** 2 * rx * rx      # < (rx*ry)^2 inside the ellipse
        r2 = (rx * ry) ** 2
        k = np.clip(255 - (d * 200) // max(1, r2), 0, 255)
        if i % 5 == 1:
            k = np.where(k > 60, 128, k)                      # a plateau of exactly 0.5: never drawn
        elif i % 5 == 2:
            k = np.where((k > 100) & (k < 160), 128, k)       # a 0.5 ring around a covered core
        masks[i] = k.astype(np.uint8)
        x1, y1 = max(0, cx - rx) / mw, max(0, cy - ry) / mh
        x2, y2 = min(mw, cx + rx) / mw, min(mh, cy + ry) / mh
        if i % 6 == 5:                                        # centre in the bottom padding: dropped by the centre test (source mode)
            y1, y2 = s_h + (1.0 - s_h) * 0.25, 1.0
        boxes[i] = (x1, y1, x2, y2)
    scores = rng.uniform(0.0, 1.0, n).astype(np.float32)
    if n > 1:
        scores[1::9] = rng.uniform(0.0, 0.05, len(scores[1::9])).astype(np.float32)   # below eval_conf_thresh
    classes = rng.integers(1, 41, n).astype(np.int64)
    box_ids = rng.integers(0, max(1, n // 2 + 1), n).astype(np.int64)                # repeated ids
    return {"box": boxes, "score": scores, "class": classes, "box_ids": box_ids, "mask_u8": masks}
