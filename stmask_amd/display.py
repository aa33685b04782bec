"""Display mode: tracked instances drawn onto their frames on the device (reference eval.py:143-318, ``prep_display``).

``render`` draws one frame, ``render_batch`` many frames of different sizes in one ``stm_render_overlay_u8`` launch per 64 frames.  The
result is a uint8 [H, W, 3] tensor on the device.  Per frame the rows are chosen as prep_display chooses them: postprocess_ytbvis's score
threshold (``conf_thresh``, cfg.eval_conf_thresh) and, in source mode, its box-centre test (``output_utils.select_rows``), then the first
``top_k`` rows, cut at the first row scoring below ``score_threshold``.  The kernel draws each row's soft mask bilinearly resized and
thresholded at 0.5, exactly the pixels the results json encodes, in palette colour ``(box_ids * 5) % len(palette)``, alpha-blended in
the reference's fp32 operation order.  Row 0 ends on top.

Two base images:
  * ``mode="source"``: the uint8 source frame [ori_h, ori_w, 3], taken as BGR as preprocess.py takes its inputs (the palette colour is
    reversed to match), output at ori_shape.  What a serving user wants: their own frames annotated at full resolution.
  * ``mode="reference"``: what ``eval.py --display`` draws on, the network input fp32 [3, pad_h, pad_w] un-padded and de-normalised
    (reference output_utils.py:136-165 ``undo_image_transformation``, reproduced as it computes: its two channel swaps around
    ``* STD + MEANS`` pair output channel c with STD[2 - c] and MEANS[2 - c]), output at img_shape; colours in palette order.

Box outlines (``boxes=True``) are this project's rule, not cv2's: the reference draws them with cv2.rectangle(thickness=2), which is not
reproduced.  Coordinates are clamped as the reference clamps them (x to [2, max_w], y to [2, max_h], max = ori size in source mode and
the padded size in reference mode), and the 3-pixel band centred on each edge is painted opaque in the row's colour, clipped to the
frame, after the masks, row 0 on top.  Text labels and the fps banner (Hershey fonts rasterised by cv2) are not drawn.

PALETTE is the package's own: 20 colours at golden-ratio hue steps (saturation 0.75, value 0.95), RGB.  ``palette=`` takes any [K, 3]
RGB list, e.g. the reference's cfg.COLORS.
"""
import colorsys
import ctypes

import torch

from . import _lib, output_utils
from .preprocess import MEANS, STD

PALETTE = tuple(tuple(int(round(255 * v)) for v in colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, 0.75, 0.95)) for i in range(20))


def palette_colors(box_ids, palette=None, bgr=False):
    """fp32 [n, 3] colours / 255 of rows with these box ids, on box_ids' device, computed as the reference computes them (get_color:
    palette entry (id * 5) % K divided by 255 in fp32 on the host -- a device division by a scalar multiplies by its reciprocal), channels
    reversed when `bgr`.  No host synchronisation: the K-entry table is divided on the host and indexed on the device."""
    table = torch.tensor(PALETTE if palette is None else palette, dtype=torch.float32).view(-1, 3) / 255.0
    if bgr:
        table = table.flip(1)
    table = table.contiguous().to(box_ids.device)
    return table[(box_ids.long() * 5) % table.shape[0]]


def clamp_boxes(boxes, max_w, max_h):
    """Integer pixel boxes [n, 4] -> int32 [n, 4] clamped as prep_display clamps them before drawing (x to [2, max_w], y to [2, max_h])."""
    b = boxes.long().clone()
    b[:, 0::2] = b[:, 0::2].clamp(2, max_w)
    b[:, 1::2] = b[:, 1::2].clamp(2, max_h)
    return b.int()


def select(det, img_meta, mode="source", conf_thresh=0.05, top_k=100, score_threshold=0.0):
    """Rows prep_display draws -> (masks [n, mh, mw] soft, box_ids [n], pixel boxes [n, 4] long, crop_h, crop_w, out_h, out_w)."""
    preserve = _check_mode(mode)
    if det is None or not det or det["box"].nelement() == 0:
        img_h, img_w = img_meta["img_shape"][:2]
        out_h, out_w = img_meta["ori_shape"][:2] if preserve else (img_h, img_w)
        return None, None, None, 0, 0, out_h, out_w
    rows, crop_h, crop_w, out_h, out_w = output_utils.select_rows(det, img_meta, conf_thresh, preserve)
    n = min(top_k, int(rows["score"].shape[0]))
    if n and score_threshold > 0:
        below = torch.nonzero(rows["score"][:n] < score_threshold).view(-1)
        if below.numel():
            n = int(below[0])
    if n == 0:
        return None, None, None, crop_h, crop_w, out_h, out_w
    pix = output_utils.pixel_boxes(rows["box"][:n], img_meta, preserve)
    return rows["mask"][:n], rows["box_ids"][:n], pix, crop_h, crop_w, out_h, out_w


def _check_mode(mode):
    if mode not in ("source", "reference"):
        raise ValueError(f"display mode {mode!r}: 'source' or 'reference'")
    return mode == "source"


def render(det, base, img_meta, mode="source", palette=None, alpha=0.45, boxes=True, out=None, **select_kw):
    """One frame -> uint8 [H, W, 3] on the device (module docstring).  det: the frame's detection dict (box, score, mask, box_ids; None
    or empty for no rows); base: uint8 [ori_h, ori_w, 3] (source) or the fp32 network input [3, pad_h, pad_w] (reference)."""
    return render_batch([det], [base], [img_meta], mode=mode, palette=palette, alpha=alpha, boxes=boxes,
                        outs=None if out is None else [out], **select_kw)[0]


def render_batch(dets, bases, metas, mode="source", palette=None, alpha=0.45, boxes=True, outs=None, **select_kw):
    """Many frames (sizes may differ) -> list of uint8 [H_i, W_i, 3] on the device, one kernel launch per 64 frames."""
    preserve = _check_mode(mode)
    dets, bases, metas = list(dets), list(bases), list(metas)
    if not (len(dets) == len(bases) == len(metas)) or (outs is not None and len(outs) != len(dets)):
        raise ValueError("render_batch: dets, bases, metas (and outs) must have one entry per frame")
    if not dets:
        return []
    dev = bases[0].device
    if dev.type != "cuda":
        raise ValueError("render_batch: the base images must be on the GPU")
    masks, colors, bxs, frames, results = [], [], [], [], []
    mask_hw, n_rows = None, 0
    for i, (det, base, meta) in enumerate(zip(dets, bases, metas)):
        m, ids, pix, crop_h, crop_w, out_h, out_w = select(det, meta, mode, **select_kw)
        f = _lib.RenderFrame()
        if base.device != dev:
            raise ValueError("render_batch: every base image must be on the same device")
        if preserve:
            if base.dtype != torch.uint8 or base.dim() != 3 or tuple(base.shape) != (out_h, out_w, 3) or base.stride(1) != 3 or base.stride(2) != 1:
                raise ValueError(f"render_batch: frame {i}: source mode needs a uint8 [{out_h}, {out_w}, 3] frame with packed pixels, "
                                 f"got {base.dtype} {tuple(base.shape)}")
            f.base_fmt, f.base_h, f.base_w, f.base_row_stride = 0, out_h, out_w, base.stride(0)
        else:
            if base.dtype != torch.float32 or base.dim() != 3 or base.shape[0] != 3 or not base.is_contiguous():
                raise ValueError(f"render_batch: frame {i}: reference mode needs the contiguous fp32 [3, H, W] network input")
            img_h, img_w = meta["img_shape"][:2]
            pad_h, pad_w = meta["pad_shape"][:2]
            f.base_fmt, f.base_h, f.base_w = 1, base.shape[1], base.shape[2]
            f.base_crop_h, f.base_crop_w = int(img_h / pad_h * base.shape[1]), int(img_w / pad_w * base.shape[2])
            for c in range(3):                                   # undo_image_transformation's swaps: channel c meets STD[2 - c], MEANS[2 - c]
                f.mean[c], f.stdv[c] = MEANS[2 - c], STD[2 - c]
        o = outs[i] if outs is not None else torch.empty(out_h, out_w, 3, dtype=torch.uint8, device=dev)
        if o.dtype != torch.uint8 or tuple(o.shape) != (out_h, out_w, 3) or o.stride(1) != 3 or o.stride(2) != 1 or o.device != dev:
            raise ValueError(f"render_batch: frame {i}: out must be uint8 [{out_h}, {out_w}, 3] with packed pixels on {dev}")
        f.base, f.out, f.out_row_stride, f.out_h, f.out_w = base.data_ptr(), o.data_ptr(), o.stride(0), out_h, out_w
        if m is not None:
            if mask_hw is None:
                mask_hw = tuple(m.shape[1:])
            elif tuple(m.shape[1:]) != mask_hw:
                raise ValueError("render_batch: every frame's masks must have one prototype size")
            max_w, max_h = (meta["ori_shape"][1], meta["ori_shape"][0]) if preserve else (meta["pad_shape"][1], meta["pad_shape"][0])
            masks.append(m)
            colors.append(palette_colors(ids, palette, bgr=preserve))
            bxs.append(clamp_boxes(pix, max_w, max_h))
            f.inst_begin, f.n_inst, f.crop_h, f.crop_w = n_rows, m.shape[0], crop_h, crop_w
            n_rows += m.shape[0]
        frames.append(f)
        results.append(o)
    if n_rows:
        mask_t = torch.cat([m.to(dev, torch.float32) for m in masks]).contiguous()
        color_t = torch.cat(colors).to(dev)
        box_t = torch.cat(bxs).to(dev) if boxes else None
    else:
        mask_t = color_t = box_t = None
    mh, mw = mask_hw if mask_hw else (0, 0)
    ws = torch.empty(_lib.lib().stm_render_workspace_bytes(n_rows), dtype=torch.uint8, device=dev)
    arr = (_lib.RenderFrame * len(frames))(*frames)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    _lib.call("stm_render_overlay_u8", arr, len(frames), ptr(mask_t), n_rows, mh, mw, ptr(color_t), ptr(box_t), alpha, ptr(ws), ws.numel(),
              ctypes.c_void_p(stream))
    return results
