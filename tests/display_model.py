"""Display fixtures and an fp32 torch restatement of prep_display's compositing, for tests/test_display_cpu.py and test_gpu_display.py.

The restatement works on whole frames in the documented operation order: every row enters with
inv_j = m_j * (-a) + 1 and mc_j = (m_j * c_j) * a, m_j in {0, 1}; P is the sequential product; the terms mc_j * cp_{j-1} (j >= 1) are summed
in ATen's CPU grouping (blocks of 16 summed from zero and added to a running total, the remainder summed alone and added last); S = mc_0 + T;
out = (uint8)((img * P + S) * 255).
"""
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import display_cases  # noqa: E402

from stmask_amd import display  # noqa: E402

CASES = display_cases.CASES


def load():
    return dict(np.load(os.path.join(HERE, "golden", "display_cases.npz"), allow_pickle=False))


def case_inputs(z, name, device="cpu"):
    """-> (det dict, base tensor, img_meta, mode) of one fixture case."""
    spec = CASES[name]
    det = {"box": torch.from_numpy(z[f"{name}/box"]), "score": torch.from_numpy(z[f"{name}/score"]),
           "class": torch.from_numpy(z[f"{name}/class"]), "box_ids": torch.from_numpy(z[f"{name}/box_ids"]),
           "mask": torch.from_numpy(z[f"{name}/mask_u8"]).float() / 256.0}
    det = {k: v.to(device) for k, v in det.items()}
    if spec[0] == "source":
        base = torch.from_numpy(display_cases.source_frame(spec)).to(device)
    else:
        base = torch.from_numpy(display_cases.network_input(spec)).to(device)
    return det, base, display_cases.meta(spec), spec[0]


def row_crcs(img):
    a = np.ascontiguousarray(img)
    return np.array([zlib.crc32(a[y].tobytes()) for y in range(a.shape[0])], dtype=np.uint32)


def check_against_golden(z, name, out):
    """out: uint8 [H, W, 3] numpy.  Raises AssertionError naming the first differing row."""
    shape = tuple(int(v) for v in z[f"{name}/shape"])
    assert out.shape == shape, (name, out.shape, shape)
    if f"{name}/out" in z:
        ref = z[f"{name}/out"]
        bad = np.argwhere((out != ref).any(2))
        assert bad.size == 0, f"{name}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {out[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
        return
    yx = z[f"{name}/sample_yx"]
    px = out[yx[:, 0], yx[:, 1]]
    bad = np.nonzero((px != z[f"{name}/sample_px"]).any(1))[0]
    crc = row_crcs(out)
    rows = np.nonzero(crc != z[f"{name}/row_crc"])[0]
    assert rows.size == 0 and bad.size == 0, (f"{name}: {rows.size} rows differ (first {rows[:8].tolist()}), {bad.size} sampled pixels differ"
                                              + (f", first at {tuple(yx[bad[0]])}" if bad.size else ""))


def base_image(base, meta, mode):
    """fp32 [H, W, 3] base of prep_display: source frame / 255, or undo_image_transformation of the network input (float64, as written)."""
    if mode == "source":
        return base.cpu() / 255.0
    img_h, img_w = meta["img_shape"][:2]
    pad_h, pad_w = meta["pad_shape"][:2]
    x = base.cpu()
    x = x[:, :int(img_h / pad_h * x.shape[1]), :int(img_w / pad_w * x.shape[2])]
    x = F.interpolate(x[None], (img_h, img_w), mode="bilinear", align_corners=False)[0]
    a = x.permute(1, 2, 0).numpy()[:, :, (2, 1, 0)]
    a = (a * np.array(display_cases.STD) + np.array(display_cases.MEANS)) / 255.0
    a = np.clip(a[:, :, (2, 1, 0)], 0, 1)
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def coverage(masks, crop_h, crop_w, out_h, out_w):
    return F.interpolate(masks[None, :, :crop_h, :crop_w].float().cpu(), (out_h, out_w), mode="bilinear", align_corners=False)[0] > 0.5


def composite(img, cov, colors, alpha=0.45):
    """img fp32 [H, W, 3], cov bool [n, H, W], colors fp32 [n, 3] -> uint8 [H, W, 3] in the documented order."""
    n = cov.shape[0]
    if n == 0:
        return (img * 255).byte()
    a = torch.tensor(alpha, dtype=torch.float32)
    m = cov.float()[..., None]                                # [n, H, W, 1]
    inv = m * (-a) + 1
    mc = (m * colors.view(n, 1, 1, 3)) * a
    P = inv[0].clone()
    for j in range(1, n):
        P = P * inv[j]
    S_terms = n - 1
    full = 16 * (S_terms // 16)
    acc0 = torch.zeros_like(mc[0].expand_as(img)).clone()
    acc1 = torch.zeros_like(acc0)
    cp = inv[0].clone()
    for k in range(S_terms):                                  # term k = mc_{k+1} * cp_k
        if k < full and k % 16 == 0 and k > 0:
            acc1, acc0 = acc1 + acc0, torch.zeros_like(acc0)
        if k == full and full > 0:
            acc1, acc0 = acc1 + acc0, torch.zeros_like(acc0)
        acc0 = acc0 + mc[k + 1] * cp
        cp = cp * inv[k + 1]
    if full > 0 and full == S_terms:
        acc1, acc0 = acc1 + acc0, torch.zeros_like(acc0)
    S = mc[0] + (acc0 + acc1)
    return ((img * P + S) * 255).byte()


def restate(det, base, meta, mode, palette, alpha=0.45):
    """The whole of prep_display (masks, boxes off) in torch on the host."""
    m, ids, _, crop_h, crop_w, out_h, out_w = display.select(det, meta, mode)
    img = base_image(base, meta, mode)
    if m is None:
        return (img * 255).byte()
    cov = coverage(m, crop_h, crop_w, out_h, out_w)
    return composite(img, cov, display.palette_colors(ids.cpu(), palette, bgr=mode == "source"), alpha)
