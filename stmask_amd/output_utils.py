"""Output stage on the MI355X -- mirror of the reference's layers/output_utils.py:16-133 (``postprocess_ytbvis``), the
first "next" row after the hot path: score filter, un-pad, bilinear up-sampling of the soft masks to
the original frame size, threshold, COCO run-length encoding, box rescaling.

The reference brings every full-resolution mask to the host (``masks[i].cpu()``) and encodes it with pycocotools; here
resize + threshold + run extraction run on the device (``stm_mask_resize_rle_f32``) and only the run lengths cross PCIe.
The 5-bit string packing of COCO RLE (pycocotools maskApi.c ``rleToString``) is a few hundred bytes per mask and stays
on the host.

``OutputStageBatch`` (below) is the same stage for all frames of a step at once, string packing included, in a fixed number of
launches and one device -> host copy (``stm_output_stage_multi_f32``); ``postprocess_ytbvis`` stays the per-frame form.
"""
import torch

from . import ops
from .layers.box_utils import center_size, sanitize_coordinates

_SKIP = ("proto", "bbox_idx", "priors", "embed_vectors", "box_shift")


def rle_counts_to_string(counts):
    """COCO compressed RLE string of a list of run lengths (maskApi.c rleToString)."""
    out = bytearray()
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1F
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
    return bytes(out)


def encode_masks(masks_soft, crop_h, crop_w, out_h, out_w, thr=0.5, max_runs=4096):
    """[n,mh,mw] soft masks -> list of COCO RLE dicts {'size': [h, w], 'counts': bytes} (device resize + RLE)."""
    n = masks_soft.shape[0]
    counts, n_runs = ops.mask_resize_rle(masks_soft, crop_h, crop_w, out_h, out_w, thr, max_runs)
    nr = n_runs.cpu()
    if n and int(nr.max()) > max_runs:  # a very ragged mask: redo with room for every run
        return encode_masks(masks_soft, crop_h, crop_w, out_h, out_w, thr, int(nr.max()))
    width = int(nr.max()) if n else 0
    if n == 0:
        return []
    host = counts[:, :width].contiguous().cpu()  # the ONLY mask bytes that cross PCIe: run lengths
    strings = rle_strings(host, nr)
    return [{"size": [out_h, out_w], "counts": strings[i]} for i in range(n)]


def rle_strings(counts_host, n_runs_host):
    """COCO RLE strings of the rows of counts_host [n, width] int32 (CPU, contiguous; row i holds n_runs_host[i] runs): the library's host-side
    packer (stm_rle_strings_host) -- the Python form above costs ~0.2 ms per mask, more than the GPU spends on a whole step."""
    import ctypes
    import numpy as np
    from . import _lib
    n, width = counts_host.shape
    c = np.ascontiguousarray(counts_host.numpy().astype(np.uint32, copy=False))
    nr = np.ascontiguousarray(n_runs_host.numpy().astype(np.int32, copy=False))
    out_ld = max(16, 5 * width)                              # a run takes at most 7 characters, typically 1-3; retried below if it does not fit
    while True:
        out = np.empty((n, out_ld), dtype=np.uint8)
        lens = np.empty(n, dtype=np.int32)
        try:
            _lib.call("stm_rle_strings_host", c.ctypes.data_as(ctypes.c_void_p), width, nr.ctypes.data_as(ctypes.c_void_p), n,
                      out.ctypes.data_as(ctypes.c_void_p), out_ld, lens.ctypes.data_as(ctypes.c_void_p))
            break
        except _lib.StmError:
            if int(lens.max()) <= out_ld:
                raise
        out_ld = int(lens.max())
    return [out[i, :lens[i]].tobytes() for i in range(n)]


def select_rows(det, img_meta, score_threshold=0, preserve_aspect_ratio=True):
    """Row selection of postprocess_ytbvis (reference output_utils.py:45-69): the rows with score > score_threshold (when > 0) and, with
    preserve_aspect_ratio, whose box centre lies inside the image.  det: the detection dict (not modified; unselected keys are shared).
    -> (dict of the kept rows, crop_h, crop_w, out_h, out_w): the un-padded mask size and the size the masks are resized to."""
    dets = dict(det)
    ori_h, ori_w = img_meta["ori_shape"][:2]
    img_h, img_w = img_meta["img_shape"][:2]
    pad_h, pad_w = img_meta["pad_shape"][:2]
    s_w, s_h = img_w / pad_w, img_h / pad_h
    out_h, out_w = (ori_h, ori_w) if preserve_aspect_ratio else (img_h, img_w)
    masks = dets.get("mask")
    crop_h, crop_w = (int(s_h * masks.size(1)), int(s_w * masks.size(2))) if masks is not None and masks.dim() == 3 else (0, 0)
    if dets["box"].nelement() == 0:
        return dets, crop_h, crop_w, out_h, out_w

    def keep_rows(keep):
        idx = torch.nonzero(keep).view(-1)
        for k in dets:
            if k not in _SKIP and torch.is_tensor(dets[k]) and dets[k].dim() > 0 and dets[k].shape[0] == keep.shape[0]:
                dets[k] = dets[k].index_select(0, idx)

    if score_threshold > 0:
        keep_rows(dets["score"] > score_threshold)
    if preserve_aspect_ratio and dets["score"].nelement() != 0:
        c = center_size(dets["box"])
        keep_rows(((c[:, 0] > s_w).int() + (c[:, 1] > s_h).int()) < 1)
    return dets, crop_h, crop_w, out_h, out_w


def pixel_boxes(boxes, img_meta, preserve_aspect_ratio=True):
    """Normalised boxes [n, 4] (relative to the padded input) -> integer pixel boxes of the output frame (reference output_utils.py:112-129)."""
    img_h, img_w = img_meta["img_shape"][:2]
    pad_h, pad_w = img_meta["pad_shape"][:2]
    s_w, s_h = img_w / pad_w, img_h / pad_h
    out_h, out_w = img_meta["ori_shape"][:2] if preserve_aspect_ratio else (img_h, img_w)
    boxes = boxes.clone()
    boxes[:, 0::2] = boxes[:, 0::2] / s_w
    boxes[:, 1::2] = boxes[:, 1::2] / s_h
    boxes[:, 0], boxes[:, 2] = sanitize_coordinates(boxes[:, 0], boxes[:, 2], out_w, cast=False)
    boxes[:, 1], boxes[:, 3] = sanitize_coordinates(boxes[:, 1], boxes[:, 3], out_h, cast=False)
    return boxes.long()


def postprocess_ytbvis(det_output, img_meta, interpolation_mode="bilinear", display_mask=False, score_threshold=0,
                       preserve_aspect_ratio=True):
    """Same contract as the reference: returns the detection dict with 'segm' (list of COCO RLE dicts, or the binary
    masks on the device when display_mask) and integer pixel 'box'.  `preserve_aspect_ratio` is what eval.py sets on the
    global cfg before calling (eval.py:639)."""
    if interpolation_mode != "bilinear":
        raise NotImplementedError("the reference only ever calls this with bilinear interpolation")
    dets = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in det_output["detection"].items()}
    if dets["box"].nelement() == 0:
        dets["segm"] = []
        return dets
    dets, crop_h, crop_w, out_h, out_w = select_rows(dets, img_meta, score_threshold, preserve_aspect_ratio)
    if dets["score"].size(0) == 0:
        dets["segm"] = []
        return dets

    masks = dets["mask"]
    if display_mask:
        up = torch.nn.functional.interpolate(masks[None, :, :crop_h, :crop_w], (out_h, out_w), mode="bilinear",
                                             align_corners=False)[0]
        dets["segm"] = up.gt_(0.5)
    else:
        dets["segm"] = encode_masks(masks, crop_h, crop_w, out_h, out_w)
    dets["box"] = pixel_boxes(dets["box"], img_meta, preserve_aspect_ratio)
    return dets


# ---- the batched output stage: every frame of a step at once (ops.output_stage_multi, include/stmask_hip_output.h) ----

def frame_geometry(img_meta, mask_h, mask_w, preserve_aspect_ratio=True):
    """(crop_h, crop_w, out_h, out_w, s_w, s_h) of one frame, as select_rows / pixel_boxes form them from its img_meta."""
    ori_h, ori_w = img_meta["ori_shape"][:2]
    img_h, img_w = img_meta["img_shape"][:2]
    pad_h, pad_w = img_meta["pad_shape"][:2]
    s_w, s_h = img_w / pad_w, img_h / pad_h
    out_h, out_w = (ori_h, ori_w) if preserve_aspect_ratio else (img_h, img_w)
    return int(s_h * mask_h), int(s_w * mask_w), out_h, out_w, s_w, s_h


def unpack_step_buffer(buf, metas, classes, reencode=None):
    """The host half of the batched output stage, a pure function of the copied bytes.  buf: uint8 numpy array, stm_output_header | records |
    arena (the arena at least header.total_bytes long, unless a row says arena overflow).  metas: per frame its img_meta (with video_id and
    frame_id), or None for a frame that is not there (an idle slot).  -> per frame the dict bbox2result_with_id(postprocess_ytbvis(...)) gives
    (same keys in the same order, same value types), None for a None meta.  A kept row whose record carries the run-overflow bit has no string
    on the device: reencode(row, frame) -> its RLE dict.  Raises StmError for a record no caller should see (arena overflow, a frame index
    outside metas): OutputStageBatch resubmits the former before it unpacks."""
    import ctypes
    import numpy as np
    from . import _lib
    hb, rb = ctypes.sizeof(_lib.OutputHeader), ctypes.sizeof(_lib.OutputRow)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    n = int(buf[:hb].view(np.int32)[0]) if buf.size >= hb else 0
    records = [None if m is None else {"video_id": m["video_id"], "frame_id": m["frame_id"]} for m in metas]
    if n == 0:
        return records
    if buf.size < hb + n * rb:
        raise _lib.StmError(f"unpack_step_buffer: {buf.size} bytes cannot hold {n} records")
    table = buf[hb:hb + n * rb].view(np.int32).reshape(n, rb // 4)
    arena = buf[hb + n * rb:]
    frame, status, str_off, str_len, cls, box_id = (table[:, c] for c in (0, 1, 3, 4, 5, 6))
    scores = np.ascontiguousarray(table[:, 7]).view(np.float32)
    boxes = table[:, 8:12].astype(np.int64)
    if np.any(status & _lib.ROW_BAD_FRAME) or np.any(status & _lib.ROW_ARENA_OVERFLOW):
        raise _lib.StmError("unpack_step_buffer: a record carries the bad-frame or the arena-overflow bit")
    labels = cls.astype(np.int64)
    ids = box_id.astype(np.int64)
    for r in np.flatnonzero(((status & _lib.ROW_KEPT) != 0) & (ids >= 0)):     # row order: a frame's objects in the order of its rows
        f = int(frame[r])
        if not 0 <= f < len(metas) or metas[f] is None:
            raise _lib.StmError(f"unpack_step_buffer: row {r} belongs to frame {f}, which has no img_meta")
        if status[r] & _lib.ROW_RUN_OVERFLOW:
            if reencode is None:
                raise _lib.StmError(f"unpack_step_buffer: row {r} has more runs than the device buffer held and no reencode hook was given")
            segm = reencode(int(r), f)
        else:
            o, l = int(str_off[r]), int(str_len[r])
            if o + l > arena.size:
                raise _lib.StmError(f"unpack_step_buffer: row {r}'s string ends at byte {o + l} of an arena of {arena.size}")
            segm = {"size": [metas[f]["ori_shape"][0], metas[f]["ori_shape"][1]], "counts": arena[o:o + l].tobytes()}
        entry = {"bbox": boxes[r], "score": scores[r], "segm": segm, "label": labels[r], "category": classes[labels[r] - 1]}
        records[f][ids[r]] = entry
    return records


class OutputStageBatch:
    """Soft masks -> finished per-frame records for all frames of a step, the host one step behind the device.

    ticket = submit(rows, metas): rows = what BatchedClipPipeline.tracked_rows() returns (dict of flat device tensors: mask, box, score, class,
    frame, box_id, keep; or None for no rows), metas = per frame its img_meta with video_id / frame_id (None: idle).  Enqueues the kernels on
    the current stream and one copy of header + records + a prefix of the arena into pinned memory on a side stream; does not wait.
    collect(ticket) waits for that copy and returns per frame what postprocess_ytbvis -> bbox2result_with_id return (unpack_step_buffer).
    Two device buffers and two pinned buffers alternate: at most two tickets may be outstanding."""

    def __init__(self, classes, score_threshold=0, max_runs=4096, arena_bytes=1 << 20, prefix_bytes=1 << 16, thr=0.5):
        self.classes, self.score_threshold, self.max_runs, self.thr = classes, score_threshold, int(max_runs), thr
        self.arena_bytes, self.prefix_bytes = int(arena_bytes), int(prefix_bytes)
        self.largest_total = 0           # the largest header.total_bytes seen: the copied arena prefix is sized from it
        self._dev = [None, None]
        self._pin = [None, None]
        self._side = None
        self._n_submitted = 0
        self.bytes_copied = 0            # device -> host bytes of all collects so far
        self.resubmits = 0               # steps run again with a larger arena
        self.tail_copies = 0             # collects whose strings ran past the copied prefix
        self.reencoded_rows = 0

    def _buffers(self, slot, n, device):
        need = ops.output_stage_bytes(n, self.arena_bytes)
        room = ops.output_stage_bytes(n + n // 2, self.arena_bytes)         # (the tracked set grows from step to step: grow in strides)
        if self._dev[slot] is None or self._dev[slot].numel() < need or self._dev[slot].device != device:
            self._dev[slot] = torch.empty(room, dtype=torch.uint8, device=device)
        if self._pin[slot] is None or self._pin[slot].numel() < need:
            self._pin[slot] = torch.empty(room, dtype=torch.uint8).pin_memory()
        return self._dev[slot][:need], self._pin[slot]

    def _launch(self, t):
        rows, n = t["rows"], t["n"]
        dev_buf, pin = self._buffers(t["slot"], n, rows["mask"].device)
        ops.output_stage_multi(rows["mask"], rows["frame"], rows["score"], rows["class"], rows["box_id"], rows["box"], t["frames"],
                               row_keep=rows.get("keep"), score_threshold=self.score_threshold, thr=self.thr, max_runs=self.max_runs, out=dev_buf)
        head = ops.output_stage_bytes(n, 0)
        prefix = min(self.arena_bytes, max(self.prefix_bytes, self.largest_total + self.largest_total // 2))
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev_buf.device)
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            pin[:head + prefix].copy_(dev_buf[:head + prefix], non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        t.update(dev=dev_buf, pin=pin, head=head, copied=head + prefix, done=done)

    def submit(self, rows, metas):
        metas = list(metas)
        n = 0 if rows is None else int(rows["mask"].shape[0])
        t = {"slot": self._n_submitted % 2, "n": n, "metas": metas, "rows": rows}
        self._n_submitted += 1
        if n:
            mh, mw = rows["mask"].shape[1:]
            geo = [(1, 1, 1, 1, 1.0, 1.0) if m is None else frame_geometry(m, mh, mw) for m in metas]   # (no row may name an idle frame)
            t["frames"] = ops.output_frames(geo)
            t["geo"] = geo
            self._launch(t)
        return t

    def collect(self, t):
        import ctypes
        from . import _lib
        if t["n"] == 0:
            return [None if m is None else {"video_id": m["video_id"], "frame_id": m["frame_id"]} for m in t["metas"]]
        while True:
            t["done"].synchronize()
            host = t["pin"].numpy()
            self.bytes_copied += t["copied"]
            hdr = _lib.OutputHeader.from_buffer_copy(host[:ctypes.sizeof(_lib.OutputHeader)].tobytes())
            self.largest_total = max(self.largest_total, hdr.total_bytes)
            if hdr.total_bytes <= hdr.arena_bytes:
                break
            # the strings of this step do not fit the device arena: grow it and run the step's output stage again
            self.arena_bytes = max(2 * self.arena_bytes, 2 * hdr.total_bytes)
            self.resubmits += 1
            self._launch(t)
        end = t["head"] + hdr.total_bytes
        if end > t["copied"]:                                    # the strings ran past the copied prefix: fetch the rest
            t["pin"][t["copied"]:end].copy_(t["dev"][t["copied"]:end])
            self.bytes_copied += end - t["copied"]
            self.tail_copies += 1
        rows, geo = t["rows"], t["geo"]

        def reencode(r, f):
            self.reencoded_rows += 1
            crop_h, crop_w, out_h, out_w = geo[f][:4]
            return encode_masks(rows["mask"][r:r + 1], crop_h, crop_w, out_h, out_w, self.thr, self.max_runs)[0]

        return unpack_step_buffer(host[:end], t["metas"], self.classes, reencode)
