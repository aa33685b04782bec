"""Training batches from a YouTube-VIS / OVIS annotation file: everything between the JSON and
`criterion(net, net(images), gt_bboxes, gt_labels, gt_masks, gt_ids)`.  The reference does this per sample on the host, in DataLoader workers
(datasets/ytvos.py prepare_train_img, datasets/transforms.py, detection_collate, train.py prepare_data): every instance's RLE decoded to a mask at
source resolution, each resized with cv2, flipped, padded and stacked, both frames resized and normalised in numpy, then `G x Hp x Wp` mask bytes
and the float images uploaded.  Here the host only samples and parses (`YTVISTrainSet`: a record of arrays, run lists as the JSON gave them,
boxes, labels, ids and the flip flag) and `collate_device` uploads the uint8 frames and the run lists and renders the batch on the MI355X
(csrc/train_data.hip, include/stmask_hip_data.h): frames resized / normalised / flipped / padded by the kernel of the inference pre-processing,
masks drawn straight from their run lengths at the target size, boxes transformed in fp32.  No mask at source resolution exists anywhere.
INTEGRATION.md section 20 is the contract.  There is no CPU fallback for the device part.

Scope: the reference's training configs -- img_scale=[(640, 360)], resize_keep_ratio=False, size_divisor=32, flip_ratio=0.5, to_rgb=True,
with_track=True, clip_frames=1, and extra_aug=None or the reference's dict: ExtraAugmentation's parameters are drawn on the host (extra_aug.py)
and its pixel work is done inside the frame and mask kernels (csrc/extra_aug.hip).  Not built: aug_ref_bbox_param,
proposals, keep_ratio=True, more than one img_scale.  One rank's share of a batch in a data-parallel run: TrainLoader(shard=...).

YTVISValSet / LazyVideo at the end of the file are the test-mode half: the videos of a validation split in the form
serve.VideoBatcher.run takes, every frame read when the batcher asks for it.

decode="device" (YTVISTrainSet, YTVISValSet; the default is "host") leaves the frames in their files' bytes (jpeg.CompressedFrame) and has the
MI355X decode them: collate_device through jpeg.decode_batch in the place of upload_frames, the batcher through jpeg.compressed_prep
(INTEGRATION.md section 26).  Records, random draws and every other launch are those of "host".
"""
import ctypes
import os
import random

import numpy as np
import torch

from . import _lib, vis_eval
from . import extra_aug as _extra_aug
from . import jpeg as _jpeg
from ._lib import StmError, c_p, call, private_call
from .extra_aug import AugParams, ExtraAugmentation  # noqa: F401  (part of this module's interface)
from .preprocess import MEANS, STD

# launches of the stm_data_* / stm_vis_rle_decode entry points and bytes copied to the device since the last reset_counters()
# (scripts/bench_train_data.py reports them); "uploads" counts the host -> device copies
COUNTERS = {"launches": 0, "uploads": 0, "h2d_bytes": 0}


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0


def _launch(name, launches, *args):
    COUNTERS["launches"] += launches
    call(name, *args)


def _launch_private(name, launches, *args):
    COUNTERS["launches"] += launches
    private_call(name, *args)


def _p(t):
    return c_p(t.data_ptr()) if t is not None and t.numel() else c_p(0)


def _stream():
    return c_p(torch.cuda.current_stream().cuda_stream)


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise StmError("datasets: the batch is rendered on the MI355X; there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise StmError(f"datasets: collate_device needs a GPU device, got {device}; there is no CPU fallback")
    return device


def _up(x, device):
    """One host -> device copy through pinned memory, queued on the current stream (no host wait)."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if t.numel() == 0:
        return torch.empty(t.shape, dtype=t.dtype, device=device)
    COUNTERS["uploads"] += 1
    COUNTERS["h2d_bytes"] += t.numel() * t.element_size()
    return t.pin_memory().to(device, non_blocking=True)


def padded_size(size, divisor):
    """(h, w, Hp, Wp) of img_scale `size` = (w, h) padded to a multiple of `divisor` (mmcv.impad_to_multiple)."""
    w, h = int(size[0]), int(size[1])
    d = int(divisor) if divisor else 1
    return h, w, -(-h // d) * d, -(-w // d) * d


# ------------------------------------------------------------------------------------------------------------------ device stages
def upload_frames(arrays, device=None):
    """uint8 [H_i, W_i, 3] host arrays -> device views of ONE buffer, staged in pinned memory and copied once."""
    device = _device(device)
    sizes = []
    for i, a in enumerate(arrays):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"frame {i}: expected a uint8 [H, W, 3] array, got {type(a).__name__} "
                             f"{getattr(a, 'dtype', '')} {getattr(a, 'shape', '')}")
        sizes.append(a.size)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    stage = torch.empty(int(off[-1]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    for a, o in zip(arrays, off[:-1]):
        host[o:o + a.size] = a.reshape(-1)
    COUNTERS["uploads"] += 1
    COUNTERS["h2d_bytes"] += int(off[-1])
    buf = stage.to(device, non_blocking=True)
    return [buf[o:o + a.size].view(a.shape) for a, o in zip(arrays, off[:-1])]


class AugBlock:
    """The augmentation descriptors of a batch: `host`, a ctypes array of n _lib.AugDesc the entry points check before they launch, and `buf`,
    the one device buffer the kernels read: the same n descriptors, then frame_of int32 [n_masks] (which descriptor augments mask i)."""

    def __init__(self, host, buf, n, n_masks, keep):
        self.host, self.buf, self.n, self.n_masks, self.keep = host, buf, n, n_masks, keep

    @property
    def desc_ptr(self):
        return c_p(self.buf.data_ptr())

    @property
    def frame_of_ptr(self):
        return c_p(self.buf.data_ptr() + self.n * ctypes.sizeof(_lib.AugDesc)) if self.n_masks else c_p(0)


def _rows_ok(f):
    return f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1]


def upload_aug(frames, flips, params, frame_of=(), device=None):
    """One upload for a batch's augmentation: params = one extra_aug.AugParams per frame, frames = the uint8 [H0, W0, 3] device tensors they
    augment (None entries: descriptors for masks only, no pointer), flips = one flag per frame, frame_of = for every mask the index of its
    frame.  -> AugBlock."""
    n = len(params)
    if len(frames) != n or len(flips) != n:
        raise StmError(f"upload_aug: {len(frames)} frames, {len(flips)} flip flags, {n} parameter records")
    if n == 0:
        raise StmError("upload_aug: no frames")
    frame_of = np.asarray(frame_of, dtype=np.int32).reshape(-1)
    if frame_of.size and (frame_of.min() < 0 or frame_of.max() >= n):
        raise StmError(f"upload_aug: frame_of names a frame outside [0, {n})")
    host = (_lib.AugDesc * n)()
    keep = []
    for i, (f, p) in enumerate(zip(frames, params)):
        d = host[i]
        if f is not None:
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3 or f.device.type != "cuda":
                raise StmError(f"upload_aug: frame {i}: expected uint8 [H,W,3] on the GPU, got {f.dtype} {tuple(f.shape)} on {f.device}")
            if (int(f.shape[0]), int(f.shape[1])) != (p.H0, p.W0):
                raise StmError(f"upload_aug: frame {i} is {tuple(f.shape[:2])}, its augmentation was drawn for {(p.H0, p.W0)}")
            if not _rows_ok(f):
                f = f.contiguous()
                keep.append(f)
            d.ptr, d.row_stride_bytes = f.data_ptr(), f.stride(0)
            device = f.device
        d.H0, d.W0, d.flip, d.photo = p.H0, p.W0, int(bool(flips[i])), int(bool(p.photo))
        d.delta, d.saturation, d.hue = p.delta, p.saturation, p.hue
        d.alpha_pre, d.alpha_post = (p.alpha, 1.0) if p.contrast_mode == 1 else (1.0, p.alpha)
        d.perm[:] = [int(v) for v in p.perm]
        (d.Hc, d.Wc), (d.left, d.top) = (p.canvas, p.expand[1:]) if p.expand is not None else ((p.H0, p.W0), (0, 0))
        d.fill[:] = [float(v) for v in p.fill]
        x0, y0, x1, y1 = p.crop if p.crop is not None else (0, 0, p.W0, p.H0)
        d.x0, d.x1 = (min(max(int(v), 0), p.W0) for v in (x0, x1))
        d.y0, d.y1 = (min(max(int(v), 0), p.H0) for v in (y0, y1))
        d.cast_clip = int(p.cast == "clip")
    raw = np.concatenate([np.frombuffer(host, dtype=np.uint8), frame_of.view(np.uint8)])
    return AugBlock(host, _up(raw, _device(device)), n, int(frame_of.size), keep)


def augmented_source(frame, params):
    """stm_aug_source_u8: the augmented image itself -- uint8 [H0, W0, 3] device tensor (BGR; rows may be strided) and the AugParams that
    ExtraAugmentation.sample drew for it -> uint8 [H0, W0, 3]: what the reference's `imgs[i] = extra_aug(imgs[i], ...)` leaves, byte for byte.
    The batch kernels never write this image; this is the tool for looking at what an augmentation did."""
    block = upload_aug([frame], [False], [params])
    out = torch.empty(params.H0, params.W0, 3, dtype=torch.uint8, device=frame.device)
    with torch.cuda.device(frame.device):
        _launch_private("stm_aug_source_u8", 1, block.host, block.desc_ptr, _p(out), _stream())
    return out


def train_frames(frames, flips, size=(640, 360), divisor=32, mean=MEANS, std=STD, to_rgb=True, out=None, aug=None):
    """stm_data_frames_u8_f32: frames = uint8 [H_i, W_i, 3] device tensors (BGR; rows may be strided, pixels and channels contiguous), flips = one
    flag per frame -> fp32 [n, 3, Hp, Wp]: ImageTransform.__call__ with keep_ratio=False.  mean / std in the output's channel order.  With flip
    off and to_rgb=False image i is bit-identical to ops.preprocess_frames_multi.
    aug: one AugParams per frame, or the AugBlock upload_aug made of them (its flips are the ones used) -> stm_aug_frames_u8_f32: the same
    resize over the augmented image, whose bytes are computed at every tap instead of read; identity parameters give the bits of aug=None."""
    frames = list(frames)
    h, w, Hp, Wp = padded_size(size, divisor)
    n = len(frames)
    if len(flips) != n:
        raise StmError(f"train_frames: {n} frames, {len(flips)} flip flags")
    if n == 0:
        raise StmError("train_frames: no frames")
    dev = frames[0].device
    _device(dev)
    if aug is not None:
        block = aug if isinstance(aug, AugBlock) else upload_aug(frames, flips, list(aug))
        if block.n != n:
            raise StmError(f"train_frames: {n} frames, {block.n} augmentation descriptors")
        if out is None:
            out = torch.empty(n, 3, Hp, Wp, device=dev, dtype=torch.float32)
        elif out.dtype != torch.float32 or tuple(out.shape) != (n, 3, Hp, Wp) or not out.is_contiguous() or out.device != dev:
            raise StmError(f"train_frames: out must be contiguous fp32 {(n, 3, Hp, Wp)} on {dev}, got {out.dtype} {tuple(out.shape)}")
        m3, s3 = (ctypes.c_double * 3)(*mean), (ctypes.c_double * 3)(*std)
        with torch.cuda.device(dev):
            _launch_private("stm_aug_frames_u8_f32", -(-n // _lib.AUG_FRAMES_PER_LAUNCH), block.host, block.desc_ptr, n, _p(out), h, w, Hp, Wp, m3, s3,
                            int(bool(to_rgb)), _stream())
        return out
    desc = (_lib.DataFrameDesc * n)()
    keep = []                                       # contiguous copies made here live until the launch is enqueued (same stream)
    for i, f in enumerate(frames):
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3 or f.device != dev:
            raise StmError(f"train_frames: frame {i}: expected uint8 [H,W,3] on {dev}, got {f.dtype} {tuple(f.shape)} on {f.device}")
        if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]:
            f = f.contiguous()
            keep.append(f)
        desc[i].ptr, desc[i].H0, desc[i].W0, desc[i].row_stride_bytes, desc[i].flip = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0), int(bool(flips[i]))
    if out is None:
        out = torch.empty(n, 3, Hp, Wp, device=dev, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, 3, Hp, Wp) or not out.is_contiguous() or out.device != dev:
        raise StmError(f"train_frames: out must be contiguous fp32 {(n, 3, Hp, Wp)} on {dev}, got {out.dtype} {tuple(out.shape)}")
    m3, s3 = (ctypes.c_double * 3)(*mean), (ctypes.c_double * 3)(*std)
    with torch.cuda.device(dev):
        _launch("stm_data_frames_u8_f32", -(-n // 64), desc, n, _p(out), h, w, Hp, Wp, m3, s3, int(bool(to_rgb)), _stream())
    return out


class BatchStatus:
    """The status words of a batch's masks on their way to the host: a copy into pinned memory queued behind the kernels, and an event.
    `raise_if_bad()` waits for the event (already passed a step later) and raises ValueError naming the first flagged record."""

    def __init__(self, status, pos, who):
        self.pos, self.who = pos, who
        self.host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True) if status.numel() else None
        self.event = None
        if self.host is not None:
            self.host.copy_(status, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()

    def raise_if_bad(self):
        if self.host is None:
            return
        self.event.synchronize()
        vis_eval.raise_for_status(self.host.numpy(), self.pos, self.who)


class JoinedStatus:
    """The statuses of one batch (the frames' decode, the masks) behind one raise_if_bad(), looked at in the order given."""

    def __init__(self, *parts):
        self.parts = parts

    def raise_if_bad(self):
        for p in self.parts:
            p.raise_if_bad()


class GroundTruth:
    """render_ground_truth's result.  masks uint8 [n, Hp, Wp], boxes fp32 [n, 4] (None without boxes), extra int64 [k, n] (the rows handed in),
    area int64 [n] and n_runs int32 [n] in the lists' order (list of mask i: pos[i]), status: a BatchStatus; uploaded: the buffers the launches
    read (launch_ground_truth(gt.uploaded) repeats them)."""

    def __init__(self, masks, boxes, extra, area, n_runs, status, pos):
        self.masks, self.boxes, self.extra, self.area, self.n_runs, self.status, self.pos = masks, boxes, extra, area, n_runs, status, pos
        self.uploaded = None


def render_ground_truth(rles, sizes, flips, boxes=None, extra=(), size=(640, 360), divisor=32, device=None, who=None, aug=None):
    """The ground truth of a batch on the device.  rles: n COCO RLE dicts {'size': [H0, W0], 'counts': list of run lengths | compressed string};
    flips: n flags; boxes: float32 [n, 4] in source pixels or None; extra: rows of n integers to travel with the descriptors (labels, ids).
    Uploads: the run lists, the characters of the compressed strings if there are any, one descriptor block, the boxes.  Launches: stm_vis_rle_decode
    when a string is present, stm_data_rle_starts, stm_data_masks_u8, stm_data_boxes_f32.  No host wait: the status is read through the
    BatchStatus returned.
    aug: (one AugParams per mask) or an AugBlock whose frame_of covers the n masks -> stm_aug_masks_u8 instead of stm_data_masks_u8: Expand's
    and RandomCrop's pixel work between the target pixel and the run-list lookup.  The boxes are expected as ExtraAugmentation.sample left them."""
    device = _device(device)
    h, w, Hp, Wp = padded_size(size, divisor)
    n = len(rles)
    name = who or (lambda i: f"mask {i}")
    if len(flips) != n or (boxes is not None and len(boxes) != n) or any(len(e) != n for e in extra):
        raise StmError("render_ground_truth: the masks, flips, boxes and extra rows differ in length")
    masks = torch.empty(n, Hp, Wp, dtype=torch.uint8, device=device)
    if aug is not None and n and not isinstance(aug, AugBlock):
        aug = list(aug)
        if len(aug) != n:
            raise StmError("render_ground_truth: the masks and their augmentation parameters differ in length")
        for i, p in enumerate(aug):
            if (p.H0, p.W0) != (int(sizes[i][0]), int(sizes[i][1])):
                raise StmError(f"render_ground_truth: mask {i} is {tuple(sizes[i])}, its augmentation was drawn for {(p.H0, p.W0)}")
        with torch.cuda.device(device):
            aug = upload_aug([None] * n, flips, aug, np.arange(n), device)
    if aug is not None and n and aug.n_masks != n:
        raise StmError(f"render_ground_truth: {n} masks, the augmentation block names the frames of {aug.n_masks}")
    if n == 0:
        return GroundTruth(masks, None if boxes is None else torch.empty(0, 4, device=device), torch.empty(len(extra), 0, dtype=torch.int64, device=device),
                           torch.empty(0, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int32, device=device),
                           BatchStatus(torch.empty(0, dtype=torch.int32, device=device), np.zeros(0, np.int64), name), np.zeros(0, np.int64))
    for i, r in enumerate(rles):
        if not isinstance(r, dict) or "counts" not in r or "size" not in r:
            raise ValueError(f"{name(i)}: the segmentation is not an RLE dict with 'size' and 'counts' (polygons are not built)")
        if [int(v) for v in r["size"]] != [int(v) for v in sizes[i]]:
            raise ValueError(f"{name(i)}: the RLE's size {list(r['size'])} is not the frame's {list(sizes[i])}")
    hm = vis_eval.flatten_masks(rles, name)           # string masks first; checks h * w < 2^32 and every run length on the host
    ns, total_c, total_l = hm.ns, int(hm.s_off[-1]), int(hm.l_off[-1])
    total = total_c + total_l
    k = len(extra)
    # one descriptor block: int64 offsets [n + 1] | hw [n] | extra [k, n] | int32 n_runs [n] | status [n] | stm_data_mask_desc [n]
    meta = np.zeros((2 + k) * n + 1 + 3 * n, dtype=np.int64)
    meta[:ns] = hm.s_off[:-1]
    meta[ns:n + 1] = total_c + hm.l_off
    meta[n + 1:2 * n + 1] = hm.hw
    for j, e in enumerate(extra):
        meta[(2 + j) * n + 1:(3 + j) * n + 1] = np.asarray(e, dtype=np.int64)
    i32 = meta[(2 + k) * n + 1:].view(np.int32)
    i32[ns:n] = np.diff(hm.l_off)                     # the lists' run counts; stm_vis_rle_decode writes the strings'
    desc = i32[2 * n:].reshape(n, 4)
    desc[:, 0] = [s[0] for s in sizes]
    desc[:, 1] = [s[1] for s in sizes]
    desc[:, 2] = [1 if f else 0 for f in flips]
    desc[:, 3] = hm.pos
    with torch.cuda.device(device):
        up = {"n": n, "ns": ns, "total_c": total_c, "total": total, "k": k, "dims": (h, w, Hp, Wp), "masks": masks, "aug": aug}
        up["meta"] = _up(meta, device)
        up["runs"] = torch.empty(total, dtype=torch.int32, device=device)
        if total_l:
            COUNTERS["uploads"] += 1
            COUNTERS["h2d_bytes"] += 4 * total_l
            up["runs"][total_c:].copy_(torch.from_numpy(hm.flat.view(np.int32)).pin_memory(), non_blocking=True)
        up["chars"] = _up(hm.chars, device) if total_c else None
        up["boxes"] = None if boxes is None else _up(np.asarray(boxes, dtype=np.float32).reshape(n, 4), device)
        boxes_d, extra_d, area, n_runs, status = launch_ground_truth(up)
        st = BatchStatus(status, hm.pos, name)
    gt = GroundTruth(masks, boxes_d, extra_d, area, n_runs, st, hm.pos)
    gt.uploaded = up
    return gt


def launch_ground_truth(up):
    """The device part of render_ground_truth over its uploaded buffers: at most four launches, nothing copied, nothing read.  (A function of its
    own so that scripts/bench_train_data.py can time the launches alone.)"""
    n, ns, total_c, total, k = up["n"], up["ns"], up["total_c"], up["total"], up["k"]
    h, w, Hp, Wp = up["dims"]
    meta_d, runs, device = up["meta"], up["runs"], up["meta"].device
    off_d, hw_d = meta_d[:n + 1], meta_d[n + 1:2 * n + 1]
    extra_d = meta_d[2 * n + 1:(2 + k) * n + 1].view(k, n)
    i32_d = meta_d[(2 + k) * n + 1:].view(torch.int32)
    n_runs, status, desc_d = i32_d[:n], i32_d[n:2 * n], i32_d[2 * n:]
    starts = torch.empty(total, dtype=torch.int32, device=device)
    area = torch.empty(n, dtype=torch.int64, device=device)
    if ns:
        _launch("stm_vis_rle_decode", 1, _p(up["chars"]), _p(off_d), _p(hw_d), ns, total_c, _p(runs), _p(n_runs), _p(area), _p(status), _stream())
    _launch("stm_data_rle_starts", 1, _p(runs), _p(off_d), _p(n_runs), _p(status), _p(hw_d), n, total, _p(starts), _p(n_runs), _p(area), _p(status),
            _stream())
    block = up.get("aug")
    if block is None:
        _launch("stm_data_masks_u8", 1, _p(starts), _p(off_d), _p(n_runs), n, _p(desc_d), n, total, _p(up["masks"]), h, w, Hp, Wp, _stream())
    else:
        _launch_private("stm_aug_masks_u8", 1, _p(starts), _p(off_d), _p(n_runs), n, _p(desc_d), block.frame_of_ptr, block.desc_ptr, block.n, n, total,
                        _p(up["masks"]), h, w, Hp, Wp, _stream())
    boxes_d = None
    if up["boxes"] is not None:
        boxes_d = torch.empty(n, 4, dtype=torch.float32, device=device)
        _launch("stm_data_boxes_f32", 1, _p(up["boxes"]), _p(desc_d), n, _p(boxes_d), h, w, Hp, Wp, _stream())
    return boxes_d, extra_d, area, n_runs, status


# ------------------------------------------------------------------------------------------------------------------ the dataset
def read_frame(path):
    """The default frame_reader: the file decoded with PIL, channels reversed to cv2's BGR.  The decoder is not cv2.imread's: JPEG decoders differ
    in the last bit of some pixels, which is outside the contract."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


class YTVISTrainSet:
    """YTVOSDataset (datasets/ytvos.py) for test_mode=False, as far as the reference's training configs use it.  `ann`: a path or the loaded dict.
    Item i is the frame pair of img_ids[i] as a host record (no pixel work):
        frames [2] uint8 [H0, W0, 3] BGR arrays (frame_reader's), size (H0, W0), flip, video_id, frame_ids [2] (sorted),
        bboxes [2] float32 [G, 4], labels [2] int64 [G], obj_ids [2] lists (the annotation ids), segms [2] lists of RLE dicts as the JSON holds them,
        img_meta (the reference's dict; frame_id is the LAST frame of the sorted pair, its quirk), and the transform's settings.
    Departure: the reference appends a crowd annotation's mask but not its box, which misaligns gt_masks and gt_bboxes for the criterion; here a
    crowd annotation contributes neither.
    extra_aug: None, or the reference's dict(photo_metric_distortion=..., expand=..., random_crop=...) (or an ExtraAugmentation).  With None every
    record and every random draw is what it is without the argument.  With a dict the frames are read first, frame 0's augmentation is drawn,
    then frame 1's, THEN the clip's one flip (datasets/ytvos.py:243-248); the record gains aug = [AugParams, AugParams] and its bboxes / labels /
    obj_ids / segms are what the augmentation left.  The pixels are augmented on the device by collate_device.
    decode: "host" (frame_reader returns pixels; read_frame by default) or "device": frame_reader returns jpeg.CompressedFrames
    (jpeg.read_compressed by default), `frames` holds them, the sizes come from their headers and collate_device has the device decode them
    (decode_split: jpeg.decode_batch's split, None | "auto" | "all", which the records carry to collate_device); every
    other field of the record and every random draw is that of "host"."""

    def __init__(self, ann, img_prefix=None, frame_reader=None, img_scale=(640, 360), size_divisor=32, flip_ratio=0.5, clip_frames=1, to_rgb=True,
                 mean=MEANS, std=STD, extra_aug=None, crop_boxes="reference", cast="reference", decode="host", decode_split=None):
        if decode not in ("host", "device"):
            raise ValueError(f"YTVISTrainSet: decode={decode!r}")
        if decode_split not in (None, "auto", "all") or (decode_split is not None and decode != "device"):
            raise ValueError(f"YTVISTrainSet: decode_split={decode_split!r} with decode={decode!r}")
        self.decode, self.decode_split = decode, decode_split
        if frame_reader is None and decode == "device":
            frame_reader = _jpeg.read_compressed
        data = vis_eval._load(ann)
        self.extra_aug = _extra_aug.from_config(extra_aug, crop_boxes, cast)
        if isinstance(img_scale, list):
            if len(img_scale) != 1:
                raise ValueError("YTVISTrainSet: more than one img_scale is not built")
            img_scale = img_scale[0]
        if not 0 <= flip_ratio <= 1:
            raise ValueError(f"YTVISTrainSet: flip_ratio={flip_ratio}")
        self.img_prefix, self.frame_reader = img_prefix, frame_reader or read_frame
        self.img_scale, self.size_divisor, self.flip_ratio, self.clip_frames = (int(img_scale[0]), int(img_scale[1])), size_divisor, flip_ratio, clip_frames
        self.to_rgb, self.mean, self.std = bool(to_rgb), tuple(mean), tuple(std)
        self.cat_ids = [c["id"] for c in data["categories"]]
        self.cat2label = {cat_id: i + 1 for i, cat_id in enumerate(self.cat_ids)}
        self.vid_ids = [v["id"] for v in data["videos"]]
        self.vid_infos = {v["id"]: v for v in data["videos"]}
        self.vid_anns = {v: [] for v in self.vid_ids}
        for a in data.get("annotations") or []:
            self.vid_anns[a["video_id"]].append(a)
        self.img_ids = [(v, f) for v in self.vid_ids for f in range(len(self.vid_infos[v]["file_names"]))
                        if len(self.get_ann_info(v, f)["bboxes"])]
        self._valid = set(self.img_ids)

    def __len__(self):
        return len(self.img_ids)

    def get_ann_info(self, vid_id, frame_id):
        """_parse_ann_info for one frame: skip bbox None, area <= 0, w < 1, h < 1 (and crowd annotations: see the class)."""
        bboxes, labels, obj_ids, segms = [], [], [], []
        for ann in self.vid_anns[vid_id]:
            bbox = ann["bboxes"][frame_id]
            if bbox is None:
                continue
            area = ann["areas"][frame_id]
            x1, y1, w, h = bbox
            if area <= 0 or w < 1 or h < 1:
                continue
            if ann.get("iscrowd"):
                continue
            bboxes.append([x1, y1, x1 + w - 1, y1 + h - 1])
            labels.append(self.cat2label[ann["category_id"]])
            obj_ids.append(ann["id"])
            segms.append(ann["segmentations"][frame_id])
        return {"bboxes": np.array(bboxes, dtype=np.float32) if bboxes else np.zeros((0, 4), dtype=np.float32),
                "labels": np.array(labels, dtype=np.int64), "obj_ids": obj_ids, "segms": segms}

    def sample_ref(self, idx):
        """Another frame of the video within +-2 * clip_frames that is itself in img_ids, drawn with Python's random; the frame itself if none."""
        vid, frame_id = idx
        valid = [frame_id + i for i in range(-2 * self.clip_frames, 2 * self.clip_frames + 1) if i != 0 and (vid, frame_id + i) in self._valid]
        return random.sample(valid, 1) if valid else [frame_id]

    def __getitem__(self, i):
        vid, frame_id = self.img_ids[i]
        info = self.vid_infos[vid]
        clip = sorted(self.sample_ref((vid, frame_id)) + [frame_id])
        flip = bool(np.random.rand() < self.flip_ratio) if self.extra_aug is None else None
        frames = []
        for f in clip:
            name = info["file_names"][f]
            frames.append(self.frame_reader(name if self.img_prefix is None else os.path.join(self.img_prefix, name)))
            if (self.decode == "device") != isinstance(frames[-1], _jpeg.CompressedFrame):
                raise ValueError(f"YTVISTrainSet: decode={self.decode!r}, the frame_reader returned a {type(frames[-1]).__name__} for {name}")
        H0, W0 = int(frames[0].shape[0]), int(frames[0].shape[1])
        anns = [self.get_ann_info(vid, f) for f in clip]
        aug = None
        if self.extra_aug is not None:
            aug = []
            for t, a in enumerate(anns):
                p, a["bboxes"], a["labels"], a["obj_ids"], a["segms"] = self.extra_aug.sample(frames[t].shape[0], frames[t].shape[1], a["bboxes"],
                                                                                            a["labels"], a["obj_ids"], a["segms"])
                aug.append(p)
            flip = bool(np.random.rand() < self.flip_ratio)
        h, w, Hp, Wp = padded_size(self.img_scale, self.size_divisor)
        last = clip[-1]
        meta = dict(ori_shape=(info["height"], info["width"], 3), img_shape=(h, w, 3), pad_shape=(Hp, Wp, 3), video_id=vid, frame_id=last,
                    is_first=(last == 0), scale_factor=np.array([w / W0, h / H0, w / W0, h / H0], dtype=np.float32), flip=flip)
        rec = dict(frames=frames, size=(H0, W0), flip=flip, video_id=vid, frame_ids=clip, bboxes=[a["bboxes"] for a in anns],
                   labels=[a["labels"] for a in anns], obj_ids=[a["obj_ids"] for a in anns],
                   segms=[a["segms"] for a in anns], img_meta=meta, img_scale=self.img_scale, size_divisor=self.size_divisor, to_rgb=self.to_rgb,
                   mean=self.mean, std=self.std)
        if aug is not None:
            rec["aug"] = aug
        if self.decode_split is not None:
            rec["decode_split"] = self.decode_split
        return rec


def collate_device(records, device=None, max_gt=None, check="raise", decode_split=None):
    """Records of YTVISTrainSet -> (images [bs, 2, 3, Hp, Wp] fp32, gt_bboxes, gt_labels, gt_masks, gt_ids, img_meta) on the device, ready for
    train.train_step, in the nesting synthetic.synthetic_train_batch documents: the four ground-truth entries are lists over the clips of
    [frame 0, frame 1] tensors (boxes [G, 4] fp32 relative to the padded image, labels int64 [G], masks uint8 [G, Hp, Wp], ids int64 [G]), each a
    view into one buffer per kind.  max_gt keeps the first max_gt objects of a frame.  One upload each for the frames (pinned staging), the run
    lists, the descriptors (labels and ids ride along) and the boxes; at most 64 frames take 4 launches, plus one when a mask arrives as a
    compressed string.  Records that carry aug (YTVISTrainSet(extra_aug=...)) are augmented inside those same launches: one more upload (the
    descriptors), no more launches; records with and without aug may not be mixed.  Records of YTVISTrainSet(decode="device") carry
    jpeg.CompressedFrames: jpeg.decode_batch (one upload, at most three launches) takes the place of the frames' upload, its status joins the
    batch's, and nothing else changes (decode_split, or else what the first record carries from YTVISTrainSet(decode_split=...), is its
    `split`); compressed and decoded frames may not be mixed.  A flagged mask raises ValueError naming the video id, annotation id and frame: check="raise" waits for the status words
    here; check="deferred" appends a BatchStatus to the tuple whose .raise_if_bad() the caller invokes a step later, so the call itself never
    waits for the device."""
    if check not in ("raise", "deferred"):
        raise ValueError(f"collate_device: check={check!r}")
    device = _device(device)
    records = list(records)
    if not records:
        raise StmError("collate_device: no records")
    r0 = records[0]
    for r in records:
        if any(r[k] != r0[k] for k in ("img_scale", "size_divisor", "to_rgb", "mean", "std")):
            raise StmError("collate_device: the records come from datasets with different transforms")
    augmented = "aug" in r0
    if any(("aug" in r) != augmented for r in records):
        raise StmError("collate_device: records with and without aug in one batch")
    params, frame_of = [], []
    frames, f_flips, rles, sizes, flips, names, counts = [], [], [], [], [], [], []
    boxes, labels, ids = [], [], []
    for r in records:
        for t, f in enumerate(r["frames"]):
            if augmented:
                params.append(r["aug"][t])
            frames.append(f)
            f_flips.append(r["flip"])
            g = len(r["segms"][t]) if max_gt is None else min(len(r["segms"][t]), int(max_gt))
            counts.append(g)
            size = (int(f.shape[0]), int(f.shape[1]))
            for j in range(g):
                rles.append(r["segms"][t][j])
                frame_of.append(len(frames) - 1)
                sizes.append(size)
                flips.append(r["flip"])
                names.append((r["video_id"], r["obj_ids"][t][j], r["frame_ids"][t]))
            boxes.append(r["bboxes"][t][:g])
            labels.append(r["labels"][t][:g])
            ids.append(np.asarray(r["obj_ids"][t][:g], dtype=np.int64))
    who = lambda i: "video %s, annotation %s, frame %s" % names[i]      # noqa: E731
    compressed = isinstance(frames[0], _jpeg.CompressedFrame)
    if any(isinstance(f, _jpeg.CompressedFrame) != compressed for f in frames):
        raise StmError("collate_device: compressed and decoded frames in one batch")
    decode_status = None
    with torch.cuda.device(device):
        if compressed:
            f_names = ["video %s, frame %s%s" % (r["video_id"], r["frame_ids"][t], f" ({f.name})" if f.name else "")
                       for r in records for t, f in enumerate(r["frames"])]
            dev_frames, decode_status = _jpeg.decode_batch(frames, device, order="bgr", names=f_names, check="deferred",
                                                           split=decode_split if decode_split is not None else r0.get("decode_split"))
        else:
            dev_frames = upload_frames(frames, device)
        block = upload_aug(dev_frames, f_flips, params, frame_of, device) if augmented else None
        images = train_frames(dev_frames, f_flips, r0["img_scale"], r0["size_divisor"], r0["mean"], r0["std"], r0["to_rgb"], aug=block)
        gt = render_ground_truth(rles, sizes, flips, np.concatenate(boxes).reshape(-1, 4), (np.concatenate(labels), np.concatenate(ids)),
                                 r0["img_scale"], r0["size_divisor"], device, who, aug=block)
    edges = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    per = lambda t: [[t[edges[2 * c + k]:edges[2 * c + k + 1]] for k in range(2)] for c in range(len(records))]   # noqa: E731
    out = (images.view(len(records), 2, *images.shape[1:]), per(gt.boxes), per(gt.extra[0]), per(gt.masks), per(gt.extra[1]),
           [r["img_meta"] for r in records])
    status = gt.status if decode_status is None else JoinedStatus(decode_status, gt.status)
    if check == "deferred":
        return out + (status,)
    status.raise_if_bad()
    return out


class TrainLoader:
    """An epoch of batches: torch.randperm with a seeded generator (seed + epoch), the last short batch dropped (len(dataset) // batch_size, the
    reference's epoch_size).  No threads and no worker processes: next() reads and collates batch k + 1 on the host while the device still runs
    the step the caller queued for batch k.  Batches are collated with check="deferred"; the status of batch k is looked at when batch k + 1 is
    asked for (and that of the last batch when the epoch ends), so a loop with max_pos=K never waits for the device here.
    state() is where the run stands -- seed, epoch, batches of that epoch already handed out -- and the next __iter__ after load_state(state)
    continues there: the order is a pure function of seed + epoch, and the records of the batches passed over are neither read nor collated.
    shard=(rank, world) or shard=(rank, batch_alloc) is one rank of a data-parallel run (stmask_amd.parallel): batch_size stays the GLOBAL
    batch, and the order, len(), state() and load_state() are those of the unsharded loader (one sidecar resumes every rank); the rank reads and
    collates only its contiguous share of each global batch -- the equal split, or the slice batch_alloc = (a, b, ...) gives it (the reference's
    --batch_alloc; the entries sum to batch_size).  share is that slice of a batch as (begin, end)."""

    def __init__(self, dataset, batch_size, shuffle=True, seed=0, device=None, max_gt=None, shard=None):
        if batch_size < 1:
            raise ValueError(f"TrainLoader: batch_size={batch_size}")
        self.dataset, self.batch_size, self.shuffle, self.seed, self.device, self.max_gt = dataset, int(batch_size), shuffle, seed, device, max_gt
        self.shard, self.share = shard, (0, self.batch_size)
        if shard is not None:
            rank, second = shard
            if isinstance(second, int):
                if second < 1 or self.batch_size % second:
                    raise ValueError(f"TrainLoader: batch_size={batch_size} does not split evenly over {second} ranks (give a batch_alloc)")
                alloc = [self.batch_size // second] * second
            else:
                alloc = [int(a) for a in second]
                if not alloc or min(alloc) < 1 or sum(alloc) != self.batch_size:
                    raise ValueError(f"TrainLoader: batch_alloc={tuple(second)} must be positive and sum to batch_size={batch_size}")
            if not 0 <= rank < len(alloc):
                raise ValueError(f"TrainLoader: rank={rank} of {len(alloc)}")
            self.share = (sum(alloc[:rank]), sum(alloc[:rank + 1]))
        self.epoch = 0
        self.batch = 0          # batches of the running epoch (self.epoch - 1) handed out so far
        self._resume = None     # (epoch, batch) load_state asked the next __iter__ to continue at

    def state(self):
        """Inside an epoch: that epoch and the batches handed out.  After its last batch (or before the first epoch): the next epoch, batch 0."""
        if self._resume is not None:
            epoch, batch = self._resume
        elif self.epoch > 0 and self.batch < len(self):
            epoch, batch = self.epoch - 1, self.batch
        else:
            epoch, batch = self.epoch, 0
        return {"seed": self.seed, "epoch": epoch, "batch": batch}

    def load_state(self, state):
        epoch, batch = int(state["epoch"]), int(state["batch"])
        if epoch < 0 or not 0 <= batch <= len(self):
            raise ValueError(f"TrainLoader.load_state: epoch={epoch} batch={batch}, an epoch has {len(self)} batches")
        self.seed = state["seed"]
        self.epoch, self.batch, self._resume = epoch, 0, (epoch, batch)

    def __len__(self):
        return len(self.dataset) // self.batch_size

    def order(self, epoch):
        n = len(self.dataset)
        if not self.shuffle:
            return list(range(n))
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seed + epoch)
        return torch.randperm(n, generator=g).tolist()

    def indices(self, order, k):
        """The dataset indices this loader reads for batch k of an epoch's `order`: the whole batch, or the rank's share of it."""
        return order[k * self.batch_size + self.share[0]:k * self.batch_size + self.share[1]]

    def __iter__(self):
        first = 0
        if self._resume is not None:
            (self.epoch, first), self._resume = self._resume, None
        order = self.order(self.epoch)
        self.epoch += 1
        self.batch = first
        pending = None
        for k in range(first, len(self)):
            self.batch = k + 1
            records = [self.dataset[i] for i in self.indices(order, k)]
            *batch, status = collate_device(records, self.device, self.max_gt, check="deferred")
            if pending is not None:
                pending.raise_if_bad()
            pending = status
            yield tuple(batch)
        if pending is not None:
            pending.raise_if_bad()


# ------------------------------------------------------------------------------------------------------------------ the validation split
class LazyVideo:
    """One video of a YTVISValSet in the form serve.VideoBatcher.run indexes: .shape is (T, H, W, 3) from the annotation, video[t] is frame t as a
    uint8 [H, W, 3] tensor (pinned when there is a GPU), read when first asked for and dropped once `keep` later frames of the video have been
    asked for (a frame asked for again after that is read again).  With a pool, asking for frame t also starts the reads of the next
    `read_ahead` frames, in the video's own order.  A frame_reader that returns a jpeg.CompressedFrame (YTVISValSet(decode="device")) has
    video[t] return it as it is: its size is checked from the header, no pixel work is done here, and the batcher's prep decodes it
    (jpeg.compressed_prep)."""

    def __init__(self, names, height, width, frame_reader, keep=2, pool=None, read_ahead=0):
        self.names, self.shape = list(names), (len(names), int(height), int(width), 3)
        self.frame_reader, self.keep, self.pool, self.read_ahead = frame_reader, int(keep), pool, int(read_ahead)
        self._held = {}        # frame index -> tensor, or the future of its read
        self._asked = []       # distinct frame indices in the order they were first asked for, the held ones only

    def __len__(self):
        return self.shape[0]

    def _read(self, t):
        a = self.frame_reader(self.names[t])
        if isinstance(a, _jpeg.CompressedFrame):
            if tuple(a.shape) != self.shape[1:]:
                raise ValueError(f"{self.names[t]}: its header says {tuple(a.shape)}, the annotation says {self.shape[1:]}")
            return a
        if tuple(a.shape) != self.shape[1:]:
            raise ValueError(f"{self.names[t]}: decoded to {tuple(a.shape)}, the annotation says {self.shape[1:]}")
        f = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))
        return f.pin_memory() if torch.cuda.is_available() else f

    def __getitem__(self, t):
        t = int(t)
        if not 0 <= t < self.shape[0]:
            raise IndexError(f"frame {t} of a video of {self.shape[0]}")
        if self.pool is not None:
            for u in range(t + 1, min(t + 1 + self.read_ahead, self.shape[0])):
                if u not in self._held:
                    self._held[u] = self.pool.submit(self._read, u)
        got = self._held.get(t)
        if got is None:
            got = self._read(t)
        elif not isinstance(got, (torch.Tensor, _jpeg.CompressedFrame)):
            got = got.result()
        self._held[t] = got
        if t not in self._asked:
            self._asked.append(t)
            while len(self._asked) > self.keep:         # `keep` later frames have been asked for: the oldest goes
                self._held.pop(self._asked.pop(0), None)
        return got


class YTVISValSet:
    """YTVOSDataset (datasets/ytvos.py) for test_mode=True, as far as the reference's validation uses it: the videos of an annotation file in
    file order, each with id, filenames, height, width, length, with or without `annotations` (the official valid split has none).  videos() is
    the list of (video_id, LazyVideo) serve.VideoBatcher.run takes: no frame is read before the batcher asks for it, and a video holds at most
    keep + read_ahead frames.  read_ahead=k > 0: a thread pool of min(8, k) threads reads up to k frames ahead in each video's own order.
    decode="device": the frames stay jpeg.CompressedFrames (frame_reader: jpeg.read_compressed by default) and the batcher takes
    prep=jpeg.compressed_prep(...); read_ahead then reads file bytes ahead, not pixels.  decode_split (None | "auto" | "all") is kept for whoever
    makes that prep (validate.validation does): jpeg.compressed_prep(split=dataset.decode_split).
    Not restated: several img_scales, test-time flip (commented out in the reference), proposals, clip_eval_mode."""

    def __init__(self, ann, img_prefix=None, frame_reader=None, read_ahead=0, decode="host", decode_split=None):
        if decode not in ("host", "device"):
            raise ValueError(f"YTVISValSet: decode={decode!r}")
        if decode_split not in (None, "auto", "all") or (decode_split is not None and decode != "device"):
            raise ValueError(f"YTVISValSet: decode_split={decode_split!r} with decode={decode!r}")
        self.decode, self.decode_split = decode, decode_split
        data = vis_eval._load(ann)
        self.img_prefix, self.read_ahead = img_prefix, int(read_ahead)
        self.frame_reader = frame_reader or (_jpeg.read_compressed if decode == "device" else read_frame)
        if self.read_ahead < 0:
            raise ValueError(f"YTVISValSet: read_ahead={read_ahead}")
        self.has_annotations = bool(data.get("annotations"))
        self.videos_info = []
        for v in data["videos"]:
            names = [n if img_prefix is None else os.path.join(img_prefix, n) for n in v["file_names"]]
            if not names:
                raise ValueError(f"YTVISValSet: video {v['id']} has no frames")
            self.videos_info.append(dict(id=v["id"], filenames=names, height=int(v["height"]), width=int(v["width"]), length=len(names)))
        self._pool = None

    def __len__(self):
        return len(self.videos_info)

    def videos(self, keep=2):
        if self.read_ahead > 0 and self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=min(8, self.read_ahead))
        return [(v["id"], LazyVideo(v["filenames"], v["height"], v["width"], self.frame_reader, keep, self._pool, self.read_ahead))
                for v in self.videos_info]

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
