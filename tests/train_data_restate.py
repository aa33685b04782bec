"""The yardstick of the training-batch tests: the reference's host chain (datasets/transforms.py ImageTransform, MaskTransform, BboxTransform
with keep_ratio=False) restated in numpy.  Masks: every RLE is decoded to a dense column-major mask at SOURCE size, resized by cv2's nearest rule
(restated from resizeNN: sx = min(floor(x * (1.0 / (w / W0))), W0 - 1)), flipped, padded -- the path the device code never takes.  Frames:
oracle.preprocess_frames (the committed cv2-linear yardstick), then the channel reversal with permuted constants, the flip of [..., :w], the pad.
Boxes: numpy float32.  Not a test module (no test_ prefix): imported by the training-batch tests."""
import math

import numpy as np
import torch

import oracle


def padded(size, divisor):
    w, h = size
    return h, w, -(-h // divisor) * divisor, -(-w // divisor) * divisor


def dense(counts, H0, W0):
    """uint8 [H0, W0] of a list of run lengths (column-major, starting with a run of zeros)."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.sum() != H0 * W0 or (counts < 0).any():
        raise ValueError("the runs do not sum to h * w")
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return flat.reshape(W0, H0).T.copy()


def nearest_index(dst, src):
    """cv2 resizeNN: the source index of every destination index on an axis resized from src to dst."""
    inv = float(dst) / src
    ifx = 1.0 / inv
    return np.array([min(int(math.floor(d * ifx)), src - 1) for d in range(dst)], dtype=np.int64)


def resize_nearest(mask, size):
    w, h = size
    H0, W0 = mask.shape
    return mask[nearest_index(h, H0)][:, nearest_index(w, W0)]


def mask_target(mask, size, divisor, flip):
    """MaskTransform for one dense [H0, W0] mask -> uint8 [Hp, Wp]."""
    h, w, Hp, Wp = padded(size, divisor)
    m = resize_nearest(mask, size)
    if flip:
        m = m[:, ::-1]
    out = np.zeros((Hp, Wp), dtype=np.uint8)
    out[:h, :w] = m
    return out


def frame_target(img, size, divisor, flip, to_rgb, mean, std):
    """ImageTransform for one uint8 [H0, W0, 3] BGR frame -> fp32 [3, Hp, Wp]; mean / std in the output's channel order."""
    h, w, Hp, Wp = padded(size, divisor)
    m, s = (tuple(mean)[::-1], tuple(std)[::-1]) if to_rgb else (tuple(mean), tuple(std))      # by source channel
    out = oracle.preprocess_frames(torch.from_numpy(np.ascontiguousarray(img))[None], size=size, divisor=divisor, mean=m, std=s, mode=1)[0].numpy()
    assert out.shape == (3, Hp, Wp)
    if to_rgb:
        out = out[::-1]
    out = out.copy()
    if flip:
        out[:, :h, :w] = out[:, :h, :w][:, :, ::-1].copy()
    return out


def boxes_target(boxes, H0, W0, size, divisor, flip):
    """BboxTransform for float32 [G, 4] boxes of a [H0, W0] frame, in numpy float32 with the reference's operation order."""
    h, w, Hp, Wp = padded(size, divisor)
    scale = np.array([w / W0, h / H0, w / W0, h / H0], dtype=np.float32)
    g = np.asarray(boxes, dtype=np.float32).reshape(-1, 4) * scale
    if flip:
        f = g.copy()
        f[:, 0] = w - g[:, 2] - 1
        f[:, 2] = w - g[:, 0] - 1
        g = f
    g[:, 0::2] = np.clip(g[:, 0::2], 0, w) / Wp
    g[:, 1::2] = np.clip(g[:, 1::2], 0, h) / Hp
    assert g.dtype == np.float32
    return g
