"""Baseline JPEG frames decoded on the MI355X (csrc/jpeg.h, csrc/jpeg_decode.hip): an opt-in path in front of the frame, mask, augmentation and
pre-processing kernels.  The host reads the file's bytes and parses its markers (`parse`: pure Python and numpy, no pixel is touched);
`decode_batch` packs the descriptors, the tables and every entropy-coded segment of a batch into ONE pinned blob, copies it once, and at most
three launches turn it into uint8 [H, W, 3] frames on the device, bit for bit what PIL (libjpeg, its default settings) decodes.  INTEGRATION.md
section 26 is the contract.

On the device: 8-bit baseline sequential DCT (SOF0), Huffman coding, one interleaved scan, 8-bit quantisation tables, up to two DC and two AC
tables, optional restart intervals, 1 component or 3 (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, width and height 1..8192.
Everything else -- progressive, arithmetic, 12-bit, multi-scan, 4 components, other sampling factors, an Adobe marker with a non-YCbCr
transform, DNL, a file that is no JPEG -- is `Unsupported`: decode_batch decodes such a file on the host with PIL, its pixels ride in the same
copy, and COUNTERS["host_fallback"] counts it.  A file whose markers contradict themselves is `Malformed` (a ValueError).  Not built: PNG, EXIF
orientation (PIL ignores it too), encoding.

A file without restart markers is one segment and, by default, one wavefront's serial work.  split="all" | "auto" (pack_batch, decode_batch,
launch_batch's batch, compressed_prep) decodes such a segment at many places at once instead (csrc/jpeg_split.hip: self-synchronising
sub-sequences of JPEG_SUB_BYTES bytes, SPLIT_LAUNCHES launches in place of the first one); a segment that does not converge, or is damaged, is
decoded by the serial kernel after all, with the serial path's pixels and status word plus the bit _lib.JPEG_REDONE (DecodeStatus.redone()).

The library's default stays the host decoder (datasets.read_frame); this path is chosen with decode="device".
"""
import ctypes
import io

import numpy as np
import torch

from . import _lib
from ._lib import StmError, c_p, private_call

# launches of stm_jpeg_decode_u8's kernels, host -> device copies and their bytes, and files decoded on the host since the last reset_counters()
COUNTERS = {"launches": 0, "uploads": 0, "h2d_bytes": 0, "host_fallback": 0}
# images that were split since the last reset_counters(), and the segments of such images a caller of DecodeStatus.redone() has seen redone
SPLIT_COUNTERS = {"images": 0, "redone": 0}
SPLIT_LAUNCHES = _lib.JPEG_SPLIT_LAUNCHES      # what the entropy launch becomes for a batch with a split image: sync rounds 0..R, scan, write, serial
# split="auto" splits a segment of at least this many bytes: one group's.  Measured (profiles/bench_jpeg_split.txt, part 6: one noise file alone,
# the slowest content to synchronise): the split launches lose to the serial kernel at 3.7 KB and win from 8.3 KB on.
SPLIT_MIN_BYTES = _lib.JPEG_SUB_BYTES * _lib.JPEG_SUB_GROUP

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
STATUS_TEXT = {_lib.JPEG_ENOCODE: "no Huffman code within 16 bits", _lib.JPEG_EINDEX: "a coefficient index past 63",
               _lib.JPEG_ESIZE: "a size category out of range", _lib.JPEG_ETRUNCATED: "the entropy-coded data ends before its blocks are done"}
_GUARD = 16        # zero bytes behind every segment in the blob


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0
    for k in SPLIT_COUNTERS:
        SPLIT_COUNTERS[k] = 0


class Unsupported(ValueError):
    """A file the device path does not decode; .reason says why.  decode_batch hands it to PIL."""

    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


class Malformed(ValueError):
    """A file whose markers contradict themselves (a restart count that does not fit, a table that is no prefix code, a selector without table)."""


class Header:
    """What parse() found.  width, height, ncomp; hs, vs: luma sampling (chroma 1x1); mcu_w, mcu_h; dri: MCUs per restart interval (0: none);
    quant uint16 [4, 64] in natural order (tables the file does not define are zero); huff: [DC 0, DC 1, AC 0, AC 1] as (counts [16], values) or
    None; tq, td, ta: per component; ecs: (begin, end) of the entropy-coded data in the file; segments int64 [n, 4]: byte begin, byte end (in the
    file, markers excluded), first MCU, MCU count of every restart interval; tables: the stm_jpeg_tables bytes the kernels read."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def shape(self):
        return (self.height, self.width, 3)


def huff_struct(counts, values):
    """One Huffman table (counts of codes per length 1..16, symbols in code order) -> _lib.JpegHuff: the first-level lookup of JPEG_LOOK_BITS
    bits and the canonical maxcode / valoff of the longer codes."""
    counts = [int(c) for c in counts]
    values = [int(v) for v in values]
    if len(counts) != 16 or sum(counts) != len(values) or len(values) > 256:
        raise Malformed("a Huffman table whose counts and values disagree")
    t = _lib.JpegHuff()
    look = np.zeros(1 << _lib.JPEG_LOOK_BITS, dtype=np.uint16)
    code, k = 0, 0
    for length in range(1, 17):
        n = counts[length - 1]
        t.maxcode[length], t.valoff[length] = -1, 0
        if n:
            if code + n > (1 << length):
                raise Malformed("a Huffman table that is no prefix code")
            t.valoff[length] = k - code
            t.maxcode[length] = code + n - 1
            if length <= _lib.JPEG_LOOK_BITS:
                sh = _lib.JPEG_LOOK_BITS - length
                for i in range(n):
                    look[(code + i) << sh:(code + i + 1) << sh] = (length << 8) | values[k + i]
            k += n
            code += n
        code <<= 1
    t.maxcode[0] = t.maxcode[17] = -1
    ctypes.memmove(t.look, look.ctypes.data, look.nbytes)
    for i, v in enumerate(values):
        t.huffval[i] = v
    return t


def _u16(d, i):
    return (d[i] << 8) | d[i + 1]


def parse(data):
    """The markers of a JPEG file (bytes) -> Header, or raises Unsupported(reason) / Malformed.  No pixel work."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Unsupported("not a JPEG file")
    quant = np.zeros((4, 64), dtype=np.uint16)
    have_q = [False] * 4
    huff = [None] * 4
    dri, sof, adobe, jfif = 0, None, None, False
    i = 2
    while True:
        if i + 4 > n:
            raise Unsupported("no scan before the end of the file")
        if d[i] != 0xFF:
            raise Unsupported("not a JPEG file: bytes between its markers")
        m = d[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m == 0xD9:
            raise Unsupported("no scan before the end of the file")
        length = _u16(d, i + 2)
        if length < 2 or i + 2 + length > n:
            raise Unsupported("a marker segment that runs past the end of the file")
        s = d[i + 4:i + 2 + length]
        if m == 0xC0:
            if sof is not None:
                raise Unsupported("more than one frame")
            if len(s) < 6 or len(s) != 6 + 3 * s[5]:
                raise Malformed("a frame header of the wrong length")
            sof = s
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7):
            raise Unsupported({0xC1: "extended sequential DCT", 0xC2: "progressive DCT"}.get(m, "lossless or hierarchical coding"))
        elif 0xC9 <= m <= 0xCF:
            raise Unsupported("arithmetic coding")
        elif m == 0xDB:
            j = 0
            while j < len(s):
                if s[j] >> 4:
                    raise Unsupported("a 16-bit quantisation table")
                t = s[j] & 15
                if t > 3 or j + 65 > len(s):
                    raise Malformed("a quantisation table segment of the wrong length")
                quant[t, ZIGZAG] = np.frombuffer(s, dtype=np.uint8, count=64, offset=j + 1)
                have_q[t] = True
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(s):
                if j + 17 > len(s):
                    raise Malformed("a Huffman table segment of the wrong length")
                tc, th = s[j] >> 4, s[j] & 15
                counts = list(s[j + 1:j + 17])
                k = sum(counts)
                if tc > 1 or j + 17 + k > len(s):
                    raise Malformed("a Huffman table segment of the wrong length")
                if th > 1:
                    raise Unsupported("more than two Huffman tables of a class")
                huff[2 * tc + th] = (counts, list(s[j + 17:j + 17 + k]))
                j += 17 + k
        elif m == 0xDD:
            if len(s) != 2:
                raise Malformed("a restart interval segment of the wrong length")
            dri = _u16(s, 0)
        elif m == 0xDC:
            raise Unsupported("a DNL marker")
        elif m == 0xEE and len(s) >= 12 and s[:5] == b"Adobe":
            adobe = s[11]
        elif m == 0xE0 and s[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xDA:
            break
        i += 2 + length
    if sof is None:
        raise Unsupported("a scan without a baseline frame header")
    if sof[0] != 8:
        raise Unsupported(f"{sof[0]}-bit samples")
    height, width, ncomp = _u16(sof, 1), _u16(sof, 3), sof[5]
    if height == 0:
        raise Unsupported("a DNL marker")
    if ncomp not in (1, 3):
        raise Unsupported(f"{ncomp} components")
    if not (1 <= width <= _lib.JPEG_MAX_DIM and 1 <= height <= _lib.JPEG_MAX_DIM):
        raise Unsupported(f"a size of {width} x {height}, outside 1..{_lib.JPEG_MAX_DIM}")
    comps = [(sof[6 + 3 * c], sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15, sof[8 + 3 * c]) for c in range(ncomp)]
    if ncomp == 3:
        if adobe is not None and adobe != 1:
            raise Unsupported("an Adobe marker with a non-YCbCr transform")
        if adobe is None and not jfif and [c[0] for c in comps] == [82, 71, 66]:
            raise Unsupported("RGB components")
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise Unsupported("sampling factors " + ",".join(f"{c[1]}x{c[2]}" for c in comps))
        hs, vs = comps[0][1], comps[0][2]
    else:
        if not (1 <= comps[0][1] <= 4 and 1 <= comps[0][2] <= 4):
            raise Malformed("sampling factors outside 1..4")
        hs = vs = 1                 # one component: its scan is not interleaved, an MCU is one block
    if any(c[3] > 3 for c in comps):
        raise Malformed("a quantisation table selector out of range")
    # the scan header
    if len(s) < 1 or len(s) != 4 + 2 * s[0]:
        raise Malformed("a scan header of the wrong length")
    if s[0] != ncomp:
        raise Unsupported("more than one scan")
    if [s[1 + 2 * c] for c in range(ncomp)] != [c[0] for c in comps]:
        raise Unsupported("a scan whose components are not in the frame's order")
    if (s[1 + 2 * ncomp], s[2 + 2 * ncomp], s[3 + 2 * ncomp]) != (0, 63, 0):
        raise Unsupported("a scan with spectral selection or successive approximation")
    td = [s[2 + 2 * c] >> 4 for c in range(ncomp)]
    ta = [s[2 + 2 * c] & 15 for c in range(ncomp)]
    tq = [c[3] for c in comps]
    if any(t > 1 for t in td + ta):
        raise Unsupported("more than two Huffman tables of a class")
    if any(huff[t] is None for t in td) or any(huff[2 + t] is None for t in ta) or any(not have_q[t] for t in tq):
        raise Malformed("a scan that names a table the file does not define")
    begin = i + 2 + length
    # the end of the entropy-coded data: the first FF followed by anything but 00, a restart marker or another FF
    a = np.frombuffer(d, dtype=np.uint8)
    ff = np.flatnonzero(a[begin:n - 1] == 0xFF) + begin
    nxt = a[ff + 1]
    stop = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    end = int(stop[0]) if stop.size else n
    if stop.size and a[end + 1] != 0xD9:         # (fill bytes in front of a marker stay with the data: the reader stops at an FF without 00)
        m = int(a[end + 1])
        raise Unsupported("a DNL marker" if m == 0xDC else "more than one scan" if m in (0xDA, 0xC4, 0xDB, 0xDD) else f"marker FF{m:02X} behind the scan")
    mcu_w, mcu_h = -(-width // (8 * hs)), -(-height // (8 * vs))
    n_mcu = mcu_w * mcu_h
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7) & (ff < end)]
    expected = -(-n_mcu // dri) - 1 if dri else 0
    if rst.size != expected:
        raise Malformed(f"{rst.size} restart markers for {n_mcu} MCUs at a restart interval of {dri}: {expected} expected")
    if rst.size and not np.array_equal(a[rst + 1] - 0xD0, np.arange(rst.size) % 8):
        raise Malformed("restart markers that do not count D0, D1, ... D7 in order")
    starts = np.concatenate([[begin], rst + 2]).astype(np.int64)
    ends = np.concatenate([rst, [end]]).astype(np.int64)
    step = dri if dri else n_mcu
    first = np.arange(starts.size, dtype=np.int64) * step
    segments = np.stack([starts, ends, first, np.minimum(step, n_mcu - first)], axis=1)
    tables = _lib.JpegTables()
    ctypes.memmove(tables.quant, quant.ctypes.data, quant.nbytes)
    for k in range(4):
        if huff[k] is not None:
            tables.huff[k] = huff_struct(*huff[k])
    return Header(width=width, height=height, ncomp=ncomp, hs=hs, vs=vs, mcu_w=mcu_w, mcu_h=mcu_h, dri=dri, quant=quant, huff=huff, tq=tq, td=td, ta=ta,
                  ecs=(begin, end), segments=segments, tables=bytes(tables))


class CompressedFrame:
    """A frame still in its file's bytes: data, header (parse's, or None for a file the device path does not decode: PIL reads its size) and a
    name for messages.  .shape is (H, W, 3), what the decoded frame will have."""

    def __init__(self, data, header=None, name=None):
        self.data, self.name = bytes(data), name
        if header is None:
            try:
                header = parse(self.data)
            except Unsupported:
                header = None
        self.header = header
        if header is not None:
            self.shape = header.shape
        else:
            from PIL import Image
            with Image.open(io.BytesIO(self.data)) as im:
                self.shape = (im.size[1], im.size[0], 3)


def read_compressed(path):
    """A frame_reader for decode="device": the file's bytes and its parsed header, no pixel work."""
    with open(path, "rb") as f:
        return CompressedFrame(f.read(), name=str(path))


def _host_decode(data, order):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        a = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(a[:, :, ::-1] if order == "bgr" else a)


def _pad16(v):
    return (int(v) + 15) & ~15


class Batch:
    """The blob of a batch and the host copies of its descriptors (pack_batch).  fill(buffer) writes the blob into a uint8 numpy view of
    blob_bytes bytes: the image descriptors, the segment descriptors, the table sets (one per distinct set), the segments, the raw pixels."""

    def __init__(self, images, segments, n_images, n_segments, images_off, segments_off, blob_bytes, out_bytes, pieces, shapes, seg_image, fallbacks,
                 names, split_images=(), total_groups=0):
        self.names = names                 # one per file: what a message about it says
        self.split_images, self.total_groups = list(split_images), total_groups     # the files decoded at many places at once; their groups
        self.images, self.segments, self.n_images, self.n_segments = images, segments, n_images, n_segments
        self.images_off, self.segments_off, self.blob_bytes, self.out_bytes = images_off, segments_off, blob_bytes, out_bytes
        self.pieces, self.shapes, self.seg_image, self.fallbacks = pieces, shapes, seg_image, fallbacks
        self.total_blocks = int(images[n_images - 1].blk_first + _blocks(images[n_images - 1])) if n_images else 0

    @property
    def workspace_bytes(self):
        return 192 * self.total_blocks

    def fill(self, host):
        host[:self.blob_bytes] = 0
        if self.n_images:
            host[self.images_off:self.images_off + ctypes.sizeof(self.images)] = np.frombuffer(self.images, dtype=np.uint8)
        if self.n_segments:
            host[self.segments_off:self.segments_off + ctypes.sizeof(self.segments)] = np.frombuffer(self.segments, dtype=np.uint8)
        for off, piece in self.pieces:
            flat = piece.reshape(-1) if isinstance(piece, np.ndarray) else np.frombuffer(piece, dtype=np.uint8)
            host[off:off + flat.size] = flat


def _blocks(im):
    return im.mcu_w * im.mcu_h * (im.hs * im.vs + im.ncomp - 1) if im.kind == _lib.JPEG_DECODE else 0


def split_fits(nbytes, blocks):
    """csrc/jpeg_core.h jpeg_split_fits: a segment of nbytes has two sub-sequences or more, and their records (32 bytes each) fit in the plane
    region of an image of `blocks` blocks (64 bytes each)."""
    subs = -(-nbytes // _lib.JPEG_SUB_BYTES)
    return _lib.JPEG_SUB_BYTES < nbytes <= _lib.JPEG_SPLIT_MAX_BYTES and 32 * subs <= 64 * blocks


def pack_batch(datas, order="bgr", names=None, split=None):
    """Parse every file and lay the batch out (no device work): -> Batch.  A file parse() refuses as Unsupported is decoded here with PIL and
    rides as pixels; Malformed raises ValueError naming the file.  datas: bytes objects or CompressedFrames.  split: None -- every segment is one
    wavefront's work; "all" -- every image of one segment whose sub-sequence records fit (split_fits) is split; "auto" -- those of them whose
    segment has SPLIT_MIN_BYTES or more."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"jpeg: order={order!r}")
    if split not in (None, "auto", "all"):
        raise ValueError(f"jpeg: split={split!r}")
    n = len(datas)
    names = list(names) if names is not None else [getattr(x, "name", None) or f"frame {i}" for i, x in enumerate(datas)]
    if len(names) != n:
        raise ValueError(f"jpeg: {n} files, {len(names)} names")
    headers, raws = [], []
    for i, x in enumerate(datas):
        if isinstance(x, CompressedFrame):
            h, data = x.header, x.data
        else:
            data = bytes(x)
            try:
                h = parse(data)
            except Unsupported:
                h = None
            except Malformed as e:
                raise ValueError(f"{names[i]}: {e}") from None
        headers.append((h, data))
    images = (_lib.JpegImage * max(n, 1))()
    n_seg = sum(len(h.segments) for h, _ in headers if h is not None)
    segments = (_lib.JpegSegment * max(n_seg, 1))()
    images_off = 0
    segments_off = _pad16(n * ctypes.sizeof(_lib.JpegImage))
    cur = _pad16(segments_off + n_seg * ctypes.sizeof(_lib.JpegSegment))
    pieces, table_at, shapes, seg_image = [], {}, [], []
    out, blk, quad, k, fallbacks = 0, 0, 0, 0, 0
    grp, split_images = 0, []
    for h, _ in headers:                       # the table sets first, so that they share cache lines
        if h is not None and h.tables not in table_at:
            table_at[h.tables] = cur
            pieces.append((cur, h.tables))
            cur += _pad16(len(h.tables))
    for i, (h, data) in enumerate(headers):
        im = images[i]
        if h is None:
            try:
                px = _host_decode(data, order)
            except Exception as e:
                raise ValueError(f"{names[i]}: the device path does not decode it and PIL fails: {e}") from None
            fallbacks += 1
            im.kind, im.width, im.height, im.ncomp, im.hs, im.vs = _lib.JPEG_RAW, px.shape[1], px.shape[0], 3, 1, 1
            im.mcu_w, im.mcu_h = -(-px.shape[1] // 8), -(-px.shape[0] // 8)
            im.src_off = cur
            pieces.append((cur, px))
            cur += _pad16(12 * ((px.shape[0] * px.shape[1] + 3) // 4))
            shape = px.shape
        else:
            im.kind, im.width, im.height, im.ncomp, im.hs, im.vs, im.mcu_w, im.mcu_h = _lib.JPEG_DECODE, h.width, h.height, h.ncomp, h.hs, h.vs, h.mcu_w, h.mcu_h
            for c in range(h.ncomp):
                im.tq[c], im.td[c], im.ta[c] = h.tq[c], h.td[c], h.ta[c]
            im.src_off = table_at[h.tables]
            for b, e, first, count in h.segments.tolist():
                sg = segments[k]
                sg.byte_off, sg.nbytes, sg.image, sg.mcu_first, sg.mcu_count = cur, e - b, i, first, count
                pieces.append((cur, data[b:e]))
                cur += _pad16(e - b) + _GUARD
                seg_image.append(i)
                k += 1
            shape = h.shape
        im.out_off, im.blk_first, im.quad_first = out, blk, quad
        if split is not None:
            nb = int(h.segments[0][1] - h.segments[0][0]) if h is not None and len(h.segments) == 1 else 0
            if split_fits(nb, _blocks(im)) and (split == "all" or nb >= SPLIT_MIN_BYTES):
                im.split = 2 * grp + 1
                split_images.append(i)
                grp += -(-(-(-nb // _lib.JPEG_SUB_BYTES)) // _lib.JPEG_SUB_GROUP)
            else:
                im.split = 2 * grp                # (0 while nothing is split: the descriptors of such a batch are what they were)
        q = (shape[0] * shape[1] + 3) // 4
        out += _pad16(12 * q)
        blk += _blocks(im)
        quad += q
        shapes.append(tuple(int(v) for v in shape))
    if blk >= 2 ** 31 or quad >= 2 ** 31 or grp >= 2 ** 30:
        raise StmError("jpeg: 2^31 blocks or 4-pixel groups, or 2^30 sub-sequence groups, in one batch")
    return Batch(images, segments, n, n_seg, images_off, segments_off, _pad16(cur), out, pieces, shapes, np.asarray(seg_image, dtype=np.int64), fallbacks,
                 names, split_images, grp)


class DecodeStatus:
    """The status words of a batch's segments on their way to the host, in the style of datasets.BatchStatus: a copy into pinned memory queued
    behind the kernels, and an event.  raise_if_bad() waits for the event and raises ValueError naming the first damaged file."""

    def __init__(self, status, seg_image, names):
        self.seg_image, self.names = seg_image, names
        self.host, self.event = None, None
        if status is not None and status.numel():
            self.host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
            self.host.copy_(status, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()

    def flagged(self):
        """{index of the file in the batch: status word of its first flagged segment}; waits for the event."""
        if self.host is None:
            return {}
        self.event.synchronize()
        st = self.host.numpy() & ~_lib.JPEG_REDONE
        out = {}
        for s in np.flatnonzero(st):
            out.setdefault(int(self.seg_image[s]), int(st[s]))
        return out

    def redone(self):
        """The indices of the split files whose segment the serial kernel decoded after all (damaged, or not converged); waits for the event."""
        if self.host is None:
            return set()
        self.event.synchronize()
        return {int(self.seg_image[s]) for s in np.flatnonzero(self.host.numpy() & _lib.JPEG_REDONE)}

    def raise_if_bad(self):
        bad = self.flagged()
        if bad:
            i = min(bad)
            raise ValueError(f"{self.names[i]}: the JPEG data is damaged ({STATUS_TEXT.get(bad[i] & ~_lib.JPEG_REDONE, bad[i])})")


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise StmError("jpeg: frames are decoded on the MI355X; use datasets.read_frame for the host decoder")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise StmError(f"jpeg: decode_batch needs a GPU device, got {device}")
    return device


def launch_batch(batch, blob, out, status, workspace, order="bgr", stages=7):
    """The device part of decode_batch over an uploaded blob: at most three launches (SPLIT_LAUNCHES - 1 more when pack_batch split an image),
    nothing copied, nothing read.  (A function of its own so that scripts/bench_jpeg_decode.py can time the launches alone and one at a time.)"""
    launches = ((1 if stages & 1 and batch.n_segments else 0) + (1 if stages & 2 and batch.total_blocks else 0) +
                (1 if stages & 4 and batch.n_images else 0) + (SPLIT_LAUNCHES - 1 if stages & 1 and batch.split_images else 0))
    if stages & 1:
        SPLIT_COUNTERS["images"] += len(batch.split_images)
    COUNTERS["launches"] += launches
    p = lambda t: c_p(t.data_ptr()) if t is not None and t.numel() else c_p(0)     # noqa: E731
    with torch.cuda.device(blob.device):
        private_call("stm_jpeg_decode_u8", batch.images, batch.n_images, batch.segments, batch.n_segments, p(blob), batch.blob_bytes, batch.images_off,
                     batch.segments_off, p(out), batch.out_bytes, p(status), p(workspace), batch.workspace_bytes, int(order == "bgr"), stages,
                     c_p(torch.cuda.current_stream().cuda_stream))


def decode_batch(datas, device=None, order="bgr", names=None, check="raise", split=None):
    """JPEG files (bytes or CompressedFrames) -> their frames as uint8 [H_i, W_i, 3] device views of ONE buffer, channels in `order`.  One pinned
    staging blob, one host -> device copy, at most three launches, whatever the batch's size and mix of sizes.  A damaged file raises ValueError
    naming it: check="raise" waits for the status words here; check="deferred" returns (frames, DecodeStatus) and never waits for the device.
    split: pack_batch's; a batch with a split image takes SPLIT_LAUNCHES + 2 launches, whatever its size."""
    if check not in ("raise", "deferred"):
        raise ValueError(f"decode_batch: check={check!r}")
    device = _device(device)
    batch = pack_batch(datas, order, names, split)
    names = batch.names
    COUNTERS["host_fallback"] += batch.fallbacks
    if batch.n_images == 0:
        st = DecodeStatus(None, batch.seg_image, names)
        return ([], st) if check == "deferred" else []
    stage = torch.empty(batch.blob_bytes, dtype=torch.uint8, pin_memory=True)
    batch.fill(stage.numpy())
    COUNTERS["uploads"] += 1
    COUNTERS["h2d_bytes"] += batch.blob_bytes
    with torch.cuda.device(device):
        blob = stage.to(device, non_blocking=True)
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=device)
        status = torch.empty(batch.n_segments, dtype=torch.int32, device=device)
        workspace = torch.empty(batch.workspace_bytes, dtype=torch.uint8, device=device)
        launch_batch(batch, blob, out, status, workspace, order)
        st = DecodeStatus(status, batch.seg_image, names)
    frames = []
    for i, (h, w, _) in enumerate(batch.shapes):
        o = int(batch.images[i].out_off)
        frames.append(out[o:o + h * w * 3].view(h, w, 3))
    if check == "deferred":
        return frames, st
    st.raise_if_bad()
    return frames


def compressed_prep(size=(640, 360), channels_last=True, split=None):
    """A `prep` for serve.VideoBatcher over videos whose frames are CompressedFrames (datasets.YTVISValSet(decode="device")): the busy slots'
    frames of a step are decoded in ONE decode_batch (split: its argument) and handed to serve.device_prep as device frames.  A damaged
    file raises at the step that decodes it (check="raise")."""
    from . import serve

    def prep(frames, frame_ids):
        busy = [i for i, f in enumerate(frames) if f is not None]
        if busy:
            if not all(isinstance(frames[i], CompressedFrame) for i in busy):
                raise StmError("jpeg.compressed_prep: the videos' frames must be CompressedFrames (YTVISValSet(decode=\"device\"))")
            decoded = decode_batch([frames[i] for i in busy], order="bgr", split=split)
            frames = list(frames)
            for i, f in zip(busy, decoded):
                frames[i] = f
        return serve.device_prep(frames, frame_ids, size=size, channels_last=channels_last)
    return prep
