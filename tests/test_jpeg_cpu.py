"""The JPEG decoder without a GPU: the marker parse and the batch layout (stmask_amd/jpeg.py), the binding tables, the entry point's refusals,
the records of decode="device", the Python restatement against the fixtures, and the kernels' own arithmetic (csrc/jpeg_core.h) run by a
stand-alone host program under AddressSanitizer and UBSan.  No Python code runs under a sanitizer."""
import ctypes
import io
import random

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restate
from kernel_resources import kernel_resources
import train_data_cases as C
from stmask_amd import _lib, datasets, jpeg

GRID, UNSUPPORTED, DAMAGED = JC.load()


def test_fixture_grid_is_the_one_the_issue_names():
    names = [c.name for c in GRID]
    assert len(names) == 8 * 4 * 4 + 1 and len(set(names)) == len(names)
    for size in ("1x1", "7x5", "8x8", "16x16", "17x9", "33x31", "48x40", "64x50"):
        for s in ("444", "422", "420", "grey"):
            for e in ("q90", "q30opt", "q75rst3", "q100noise"):
                assert f"{size}_{s}_{e}" in names
    assert "96x160_420_rstrows1" in names
    assert [c.name for c in UNSUPPORTED] == ["unsupported_progressive", "unsupported_cmyk"]
    assert len(DAMAGED) == 3 * 8


def test_restatement_equals_every_fixture_and_counts_what_the_set_must_hold():
    stats = {}
    for c in GRID:
        assert np.array_equal(jpeg_restate.decode(c.data, stats), c.rgb), c.name
    assert all(stats[k] > 0 for k in jpeg_restate.STAT_KEYS), stats


def test_restatement_equals_a_live_pil_decode():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    for kw in (dict(quality=85, subsampling=2), dict(quality=60, subsampling=1, restart_marker_blocks=2), dict(quality=95, subsampling=0, optimize=True)):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "JPEG", **kw)
        ref = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))
        assert np.array_equal(jpeg_restate.decode(bio.getvalue()), ref), kw
    for c in GRID[::9]:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB")), c.rgb), c.name


# ---------------------------------------------------------------------------------------------------------------- parse
def test_parse_fields():
    h = jpeg.parse(JC.by_name("33x31_420_q90").data)
    assert (h.width, h.height, h.ncomp, h.hs, h.vs, h.mcu_w, h.mcu_h, h.dri) == (33, 31, 3, 2, 2, 3, 2, 0)
    assert h.shape == (31, 33, 3) and h.tq == [0, 1, 1] and h.td == [0, 1, 1] and h.ta == [0, 1, 1]
    assert h.segments.tolist() == [[h.ecs[0], h.ecs[1], 0, 6]]
    h = jpeg.parse(JC.by_name("17x9_422_q90").data)
    assert (h.hs, h.vs, h.mcu_w, h.mcu_h) == (2, 1, 2, 2)
    h = jpeg.parse(JC.by_name("17x9_grey_q90").data)
    assert (h.ncomp, h.hs, h.vs, h.mcu_w, h.mcu_h) == (1, 1, 1, 3, 2)
    h = jpeg.parse(JC.by_name("64x50_444_q90").data)
    assert (h.hs, h.vs, h.mcu_w, h.mcu_h) == (1, 1, 8, 7)


def test_parse_tables_against_the_restatement():
    for name in ("48x40_420_q90", "48x40_444_q30opt", "16x16_grey_q100noise"):
        data = JC.by_name(name).data
        h = jpeg.parse(data)
        _, _, comps, q, ht, _, _, _ = jpeg_restate.parse(data)
        t = _lib.JpegTables.from_buffer_copy(h.tables)
        for tq, tab in q.items():
            assert np.array_equal(np.ctypeslib.as_array(t.quant[tq]), tab) and np.array_equal(h.quant[tq], tab)
        for key, codes in ht.items():
            hf = t.huff[2 * (key >> 4) + (key & 15)]
            for (length, code), sym in codes.items():
                if length <= _lib.JPEG_LOOK_BITS:          # every stream prefix that starts with the code finds it in the first level
                    sh = _lib.JPEG_LOOK_BITS - length
                    assert all(hf.look[i] == ((length << 8) | sym) for i in range(code << sh, (code + 1) << sh))
                else:
                    assert hf.look[code >> (length - _lib.JPEG_LOOK_BITS)] == 0
                assert code <= hf.maxcode[length] and hf.huffval[code + hf.valoff[length]] == sym
            lengths = {length for length, _ in codes}
            assert all(hf.maxcode[length] == -1 for length in range(1, 17) if length not in lengths)


def test_parse_restart_segments():
    c = JC.by_name("48x40_420_q75rst3")
    h = jpeg.parse(c.data)
    assert h.dri == 3 and (h.mcu_w, h.mcu_h) == (3, 3) and len(h.segments) == 3
    c = JC.by_name("64x50_444_q75rst3")
    h = jpeg.parse(c.data)
    n_mcu = h.mcu_w * h.mcu_h
    assert h.dri == 3 and h.dri % h.mcu_w and len(h.segments) == -(-n_mcu // 3)
    assert h.segments[:, 2].tolist() == list(range(0, n_mcu, 3)) and int(h.segments[:, 3].sum()) == n_mcu and h.segments[-1, 3] == n_mcu - 3 * (len(h.segments) - 1)
    for k, (b, e, _, _) in enumerate(h.segments.tolist()):
        assert h.ecs[0] <= b <= e <= h.ecs[1]
        if k:                                                  # between two segments: exactly one restart marker, counted modulo 8
            assert c.data[b - 2] == 0xFF and c.data[b - 1] == 0xD0 + (k - 1) % 8 and h.segments[k - 1, 1] == b - 2
    assert c.data[h.ecs[1]:h.ecs[1] + 2] == b"\xff\xd9"
    h = jpeg.parse(JC.by_name("96x160_420_rstrows1").data)
    assert h.dri == h.mcu_w == 6 and len(h.segments) == h.mcu_h == 10


def _with_marker(data, marker, payload, before=0xDA):
    """data with an extra marker segment in front of its first `before` marker"""
    i = data.index(bytes([0xFF, before]))
    return data[:i] + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload + data[i:]


def _patched(data, marker, offset, value):
    i = data.index(bytes([0xFF, marker]))
    d = bytearray(data)
    d[i + 4 + offset] = value
    return bytes(d)


def test_every_unsupported_kind_is_refused_with_its_reason():
    base = JC.by_name("33x31_420_q90").data
    sof, sos = base.index(b"\xff\xc0"), base.index(b"\xff\xda")
    one_component_scan = base[:sos] + b"\xff\xda\x00\x08\x01" + base[sos + 5:sos + 7] + b"\x00\x3f\x00" + base[sos + 2 + base[sos + 3]:]
    cases = {
        "progressive": (UNSUPPORTED[0].data, "progressive"),
        "cmyk": (UNSUPPORTED[1].data, "4 components"),
        "arithmetic": (base[:sof] + b"\xff\xc9" + base[sof + 2:], "arithmetic"),
        "12-bit": (_patched(base, 0xC0, 0, 12), "12-bit"),
        "multi-scan": (one_component_scan, "more than one scan"),
        "sampling": (_patched(base, 0xC0, 7, 0x12), "sampling factors"),
        "chroma sampling": (_patched(base, 0xC0, 10, 0x21), "sampling factors"),
        "adobe rgb": (_with_marker(base, 0xEE, b"Adobe\0\x64\0\0\0\0\0"), "Adobe"),
        "dnl": (_with_marker(base, 0xDC, b"\0\x1f"), "DNL"),
        "height 0": (_patched(_patched(base, 0xC0, 1, 0), 0xC0, 2, 0), "DNL"),
        "16-bit quant": (_patched(base, 0xDB, 0, 0x10), "16-bit quantisation"),
        "successive approximation": (_patched(base, 0xDA, 9, 0x10), "successive approximation"),
        "not jpeg": (b"\x89PNG\r\n\x1a\n" + bytes(32), "not a JPEG"),
        "empty": (b"", "not a JPEG"),
        "no scan": (base[:base.index(b"\xff\xda")], "no scan"),
    }
    for what, (data, reason) in cases.items():
        with pytest.raises(jpeg.Unsupported) as e:
            jpeg.parse(data)
        assert reason in e.value.reason, (what, e.value.reason)
    big = bytearray(base)
    big[sof + 5:sof + 9] = (8193).to_bytes(2, "big") + (33).to_bytes(2, "big")
    with pytest.raises(jpeg.Unsupported, match="8192"):
        jpeg.parse(bytes(big))


def test_a_restart_count_that_does_not_fit_is_malformed():
    c = JC.by_name("48x40_444_q75rst3")
    h = jpeg.parse(c.data)
    b = int(h.segments[3, 0])
    with pytest.raises(jpeg.Malformed, match="restart markers"):
        jpeg.parse(c.data[:b - 2] + c.data[b:])                          # one marker removed
    with pytest.raises(jpeg.Malformed, match="restart markers"):
        jpeg.parse(_patched(c.data, 0xDD, 1, 4))                         # the interval changed under the markers
    with pytest.raises(jpeg.Malformed, match="restart markers"):
        jpeg.parse(_with_marker(JC.by_name("48x40_444_q90").data, 0xDD, b"\0\x03"))
    with pytest.raises(ValueError, match="this one.*restart markers"):
        jpeg.pack_batch([c.data[:b - 2] + c.data[b:]], names=["this one"])


def test_restart_markers_out_of_sequence_are_malformed():
    c = JC.by_name("64x50_444_q75rst3")
    h = jpeg.parse(c.data)
    assert len(h.segments) > 9                                           # the count wraps from D7 to D0 inside this file
    for k in (1, 8, 9, len(h.segments) - 1):
        d = bytearray(c.data)
        b = int(h.segments[k, 0])
        d[b - 1] = 0xD0 + k % 8                                          # marker k - 1 carries the next one's number: the count still fits
        with pytest.raises(jpeg.Malformed, match="in order"):
            jpeg.parse(bytes(d))


def test_malformed_tables_are_refused():
    with pytest.raises(jpeg.Malformed, match="prefix code"):
        jpeg.huff_struct([3] + [0] * 15, [0, 1, 2])
    with pytest.raises(jpeg.Malformed, match="disagree"):
        jpeg.huff_struct([1] + [0] * 15, [0, 1])
    base = JC.by_name("8x8_444_q90").data
    with pytest.raises(jpeg.Malformed, match="does not define"):
        jpeg.parse(_patched(base, 0xC0, 8, 3))                           # component 0 names quantisation table 3


# ---------------------------------------------------------------------------------------------------------------- the batch layout
def test_pack_batch_layout():
    cases = [JC.by_name("33x31_420_q90"), UNSUPPORTED[0], JC.by_name("48x40_444_q75rst3"), JC.by_name("33x31_420_q90"), JC.by_name("1x1_grey_q90")]
    b = jpeg.pack_batch([c.data for c in cases], "rgb")
    assert (b.n_images, b.fallbacks, b.images_off) == (5, 1, 0) and b.blob_bytes % 16 == 0 and b.segments_off % 16 == 0
    assert b.shapes == [c.rgb.shape for c in cases]
    blob = np.full(b.blob_bytes + 8, 0xEE, dtype=np.uint8)
    b.fill(blob)
    assert (blob[b.blob_bytes:] == 0xEE).all()
    im = b.images
    assert [im[i].kind for i in range(5)] == [0, 1, 0, 0, 0]
    assert im[0].src_off == im[3].src_off != im[2].src_off                 # equal table sets are stored once
    blocks = [6 * 6, 0, 6 * 5 * 3, 6 * 6, 1]
    assert [im[i].blk_first for i in range(5)] == [0] + np.cumsum(blocks)[:-1].tolist() and b.total_blocks == sum(blocks)
    quads = [(c.rgb.shape[0] * c.rgb.shape[1] + 3) // 4 for c in cases]
    assert [im[i].quad_first for i in range(5)] == [0] + np.cumsum(quads)[:-1].tolist()
    assert all(im[i].out_off % 16 == 0 and im[i].out_off + 12 * quads[i] <= (im[i + 1].out_off if i < 4 else b.out_bytes) for i in range(5))
    px = UNSUPPORTED[0].rgb
    assert np.array_equal(blob[im[1].src_off:im[1].src_off + px.size].reshape(px.shape), px)           # the host-decoded pixels ride in the blob
    assert b.n_segments == 1 + 10 + 1 + 1 and b.seg_image.tolist() == [0] + [2] * 10 + [3, 4]
    for k in range(b.n_segments):
        s = b.segments[k]
        h = jpeg.parse(cases[s.image].data)
        row = h.segments[[r[2] for r in h.segments.tolist()].index(s.mcu_first)]
        assert s.byte_off % 16 == 0 and s.nbytes == row[1] - row[0] and s.mcu_count == row[3]
        assert bytes(blob[s.byte_off:s.byte_off + s.nbytes]) == cases[s.image].data[row[0]:row[1]]
        guard = blob[s.byte_off + s.nbytes:((s.byte_off + s.nbytes + 15) & ~15) + 16]
        assert guard.size >= 16 and not guard.any()                        # a zero guard behind every segment
    with pytest.raises(ValueError, match="order"):
        jpeg.pack_batch([], "gbr")


def test_compressed_frame():
    c = JC.by_name("17x9_420_q90")
    f = jpeg.CompressedFrame(c.data, name="a.jpg")
    assert f.shape == (9, 17, 3) and f.header is not None and f.name == "a.jpg"
    pytest.importorskip("PIL.Image")
    u = jpeg.CompressedFrame(UNSUPPORTED[0].data)
    assert u.header is None and u.shape == UNSUPPORTED[0].rgb.shape


def test_read_compressed(tmp_path):
    c = JC.by_name("17x9_420_q90")
    p = tmp_path / "f.jpg"
    p.write_bytes(c.data)
    f = jpeg.read_compressed(str(p))
    assert isinstance(f, jpeg.CompressedFrame) and f.data == c.data and f.shape == (9, 17, 3) and f.name == str(p)


# ---------------------------------------------------------------------------------------------------------------- the binding
def _call(batch, **over):
    """stm_jpeg_decode_u8 over a packed batch with fake (never dereferenced) device pointers -> the return code"""
    a = dict(images=batch.images, n_images=batch.n_images, segments=batch.segments, n_segments=batch.n_segments, blob=0x1000, blob_bytes=batch.blob_bytes,
             images_off=batch.images_off, segments_off=batch.segments_off, out=0x2000, out_bytes=batch.out_bytes, status=0x3000, workspace=0x4000,
             workspace_bytes=batch.workspace_bytes, bgr=1, stages=7, stream=None)
    a.update(over)
    return _lib.private_fn("stm_jpeg_decode_u8")(*a.values())


def _copy(batch):
    images = (_lib.JpegImage * batch.n_images)()
    ctypes.memmove(images, batch.images, ctypes.sizeof(images))
    segments = (_lib.JpegSegment * batch.n_segments)()
    ctypes.memmove(segments, batch.segments, ctypes.sizeof(segments))
    return images, segments


def test_entry_point_refuses_bad_arguments_before_any_launch():
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -4, -5
    b = jpeg.pack_batch([JC.by_name("33x31_420_q90").data, JC.by_name("48x40_444_q75rst3").data])
    assert _call(b, n_images=0, n_segments=0) == 0                                  # nothing to do: no launch, no pointer read
    assert _call(b, n_images=-1) == EINVAL and _call(b, n_segments=-1) == EINVAL
    for null in ("images", "blob", "out", "segments", "status", "workspace"):
        assert _call(b, **{null: None}) == EINVAL, null
    assert _call(b, blob=0x1008) == EINVAL and _call(b, out=0x2004) == EINVAL       # alignment
    assert _call(b, workspace_bytes=b.workspace_bytes - 1) == EWORKSPACE
    assert _call(b, out_bytes=b.out_bytes - 16) == EINVAL and _call(b, blob_bytes=b.blob_bytes - 32) == EINVAL
    assert _call(b, images_off=b.blob_bytes) == EINVAL and _call(b, segments_off=b.blob_bytes - 8) == EINVAL
    assert _call(b, n_segments=b.n_segments - 1) == EINVAL                          # the last image's MCUs are not covered

    def broken(field, value, seg=None):
        images, segments = _copy(b)
        setattr(segments[seg] if seg is not None else images[1], field, value)
        return _call(b, images=images, segments=segments)
    for field, value in (("width", 0), ("width", 8193), ("height", 0), ("height", 8193), ("ncomp", 2), ("ncomp", 4), ("hs", 3), ("vs", 2), ("kind", 2),
                         ("mcu_w", 7), ("mcu_h", 4), ("blk_first", 35), ("quad_first", 0), ("out_off", 8), ("out_off", 1 << 40), ("src_off", 1 << 40),
                         ("src_off", -16)):
        assert broken(field, value) == EINVAL, (field, value)
    for field, value in (("mcu_first", 1), ("mcu_count", 0), ("mcu_count", 99), ("nbytes", -1), ("byte_off", 8), ("byte_off", 1 << 40), ("image", 0)):
        assert broken(field, value, seg=2) == EINVAL, (field, value)
    images, segments = _copy(b)
    images[1].tq[2] = 4
    assert _call(b, images=images) == EINVAL
    images[1].tq[2], images[1].ta[0] = 1, 2
    assert _call(b, images=images) == EINVAL
    # a grey image may not be subsampled; 2^31 blocks are refused as unsupported, not as invalid
    g = jpeg.pack_batch([JC.by_name("16x16_grey_q90").data])
    images, _ = _copy(g)
    images[0].hs = 2
    assert _call(g, images=images) == EINVAL
    many = (_lib.JpegImage * 2200)()
    for i in range(2200):
        ctypes.memmove(ctypes.byref(many[i]), ctypes.byref(g.images[0]), ctypes.sizeof(_lib.JpegImage))
        many[i].width = many[i].height = 8192
        many[i].mcu_w = many[i].mcu_h = 1024
        many[i].blk_first, many[i].quad_first, many[i].out_off = (i * 1024 * 1024) & 0x7FFFFFFF, (i * 2048 * 8192) & 0x7FFFFFFF, i * 8192 * 8192 * 3
    assert _call(g, images=many, n_images=2200, n_segments=0, segments=None, status=None, out_bytes=1 << 60) in (EUNSUPPORTED, EINVAL)
    fn = _lib.private_fn("stm_jpeg_workspace_bytes")
    assert fn(b.images, 2) == b.workspace_bytes == 192 * (36 + 90) and fn(None, 2) == 0 and fn(b.images, 0) == 0 and fn(images, 1) == 0
    assert "stm_jpeg_decode_u8" in _lib.lib().stm_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------- the datasets
def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if hasattr(a, "__slots__"):
        return type(a) is type(b) and all(_same(getattr(a, k), getattr(b, k)) for k in a.__slots__)
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("aug", [None, dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18),
                                            expand=dict(mean=C.MEAN, to_rgb=True, ratio_range=(1, 2)),
                                            random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3))], ids=["plain", "extra_aug"])
def test_device_records_equal_host_records_but_for_the_frames(aug):
    ann, host_reader, device_reader, files = JC.sources()
    out = {}
    for mode, reader in (("host", host_reader), ("device", device_reader)):
        ds = datasets.YTVISTrainSet(ann, frame_reader=reader, img_scale=C.SIZE, size_divisor=C.DIVISOR, extra_aug=aug, decode=mode)
        random.seed(11)
        np.random.seed(11)
        recs = [ds[i] for i in range(len(ds))] + [ds[0]]
        out[mode] = (recs, random.getstate(), np.random.get_state())
    (hr, hp, hn), (dr, dp, dn) = out["host"], out["device"]
    assert hp == dp and _same(list(hn), list(dn))                        # both random streams stand at the same place
    assert len(hr) == len(dr) > 5
    for a, b in zip(hr, dr):
        assert a.keys() == b.keys()
        assert all(_same(a[k], b[k]) for k in a if k != "frames"), [k for k in a if k != "frames" and not _same(a[k], b[k])]
        assert all(isinstance(f, jpeg.CompressedFrame) and f.shape == g.shape for f, g in zip(b["frames"], a["frames"]))
        names = ann["videos"][a["video_id"] - 1]["file_names"]
        assert [f.data for f in b["frames"]] == [files[names[t]].data for t in a["frame_ids"]]


def test_decode_option_is_checked():
    ann, host_reader, device_reader, _ = JC.sources()
    with pytest.raises(ValueError, match="decode"):
        datasets.YTVISTrainSet(ann, decode="gpu")
    with pytest.raises(ValueError, match="decode"):
        datasets.YTVISValSet(ann, decode="gpu")
    assert datasets.YTVISTrainSet(ann, decode="device").frame_reader is jpeg.read_compressed
    assert datasets.YTVISValSet(ann, decode="device").frame_reader is jpeg.read_compressed
    assert datasets.YTVISTrainSet(ann).frame_reader is datasets.read_frame and datasets.YTVISValSet(ann).frame_reader is datasets.read_frame
    with pytest.raises(ValueError, match="frame_reader returned"):
        datasets.YTVISTrainSet(ann, frame_reader=host_reader, decode="device")[0]
    with pytest.raises(ValueError, match="frame_reader returned"):
        datasets.YTVISTrainSet(ann, frame_reader=device_reader)[0]


def test_lazy_video_hands_out_compressed_frames_checked_against_the_annotation():
    ann, _, device_reader, files = JC.sources()
    vs = datasets.YTVISValSet(ann, frame_reader=device_reader, decode="device")
    vid, video = vs.videos()[0]
    assert vid == 1 and video.shape == (4, 31, 33, 3)
    f = video[1]
    assert isinstance(f, jpeg.CompressedFrame) and f.data == files["a/1.jpg"].data and video[1] is f
    ann["videos"][1]["height"] += 1
    wrong = datasets.YTVISValSet(ann, frame_reader=device_reader, decode="device").videos()[1][1]
    with pytest.raises(ValueError, match="header says"):
        wrong[0]
    ahead = datasets.YTVISValSet(JC.sources()[0], frame_reader=device_reader, decode="device", read_ahead=2)
    v = ahead.videos()[0][1]
    assert [v[t].data for t in range(4)] == [files[f"a/{t}.jpg"].data for t in range(4)]
    ahead.close()


def test_validation_passes_the_decode_option_on():
    from stmask_amd import validate

    class Twin:
        def refresh(self):
            pass

        def batcher(self, n_slots, **kw):
            self.kw = kw
            return self

        def run(self, vb, videos, out_file=None):
            self.ran = (vb, out_file)

    ann, _, device_reader, _ = JC.sources()
    twin = Twin()
    assert validate.validation(twin, datasets.YTVISValSet(ann, frame_reader=device_reader, decode="device"), "o.json", decode="device") is None
    assert callable(twin.kw["prep"]) and twin.ran == (twin, "o.json")
    assert validate.validation(twin, datasets.YTVISValSet(ann, frame_reader=device_reader), "o.json") is None and twin.kw == {}
    with pytest.raises(_lib.StmError, match="decode"):
        validate.validation(twin, datasets.YTVISValSet(ann, frame_reader=device_reader), "o.json", decode="device")


# ---------------------------------------------------------------------------------------------------------------- the kernels' arithmetic on the host
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return JC.build_host_program(tmp_path_factory.mktemp("jpeg_host"), sanitize=True)        # no compiler at all is an error, not a skip


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_host_program_decodes_every_fixture_bit_equal_under_sanitizers(host_program, tmp_path, order):
    cases = list(GRID) + list(UNSUPPORTED)
    batch = JC.write_job(tmp_path / "all.job", cases, [0] * len(cases), order)
    assert batch.fallbacks == 2                                          # the grid needs no host fallback
    rc, lines, text = JC.run_host_program(host_program, tmp_path / "all.job")
    assert rc == 0 and "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert [lines.get(i) for i in range(len(cases))] == ["equal"] * len(cases)


def test_host_program_ends_damaged_files_flagged_or_bit_equal_under_sanitizers(host_program, tmp_path):
    """Three fixtures, each cut at 25 %, 50 % and 99 % of its entropy-coded bytes and with one byte inverted at five seeded positions: every one
    ends flagged, or bit-equal to the oracle's decode of the same damaged bytes (a damaged stream can still be a valid one), and no read leaves
    the segment.  A cut that loses restart markers never reaches the kernels: parse refuses it."""
    names = [c.name for c in DAMAGED]
    for src in ("33x31_420_q90", "48x40_444_q75rst3", "64x50_422_q30opt"):
        assert [n for n in names if n.startswith(src + "_cut")] == [f"{src}_cut{p}" for p in (25, 50, 99)]
        assert len([n for n in names if n.startswith(src + "_flip")]) == 5
        sound = JC.by_name(src).data
        for c in DAMAGED:
            if c.name.startswith(src + "_flip"):
                assert len(c.data) == len(sound) and sum(a != b for a, b in zip(c.data, sound)) == 1
    dev = JC.device_damaged()
    refused = [c for c in DAMAGED if c not in dev]
    assert len(dev) >= 20
    for c in refused:
        assert c.verdict == "refused"
        with pytest.raises(jpeg.Malformed):
            jpeg.parse(c.data)
    beside = [JC.by_name("17x9_422_q90"), JC.by_name("16x16_grey_q30opt")]
    cases = dev[:7] + beside[:1] + dev[7:] + beside[1:]
    lenient = [int(c in dev) for c in cases]
    JC.write_job(tmp_path / "damaged.job", cases, lenient)
    rc, lines, text = JC.run_host_program(host_program, tmp_path / "damaged.job")
    assert rc == 0 and "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    for i, c in enumerate(cases):
        if lenient[i]:
            assert lines[i].startswith("flagged") or (lines[i] == "equal" and c.rgb is not None), (c.name, lines[i])
            assert lines[i] == c.verdict, (c.name, lines[i], c.verdict)      # what the fixtures say of it (tests/test_gpu_jpeg.py relies on that)
        else:
            assert lines[i] == "equal", (c.name, lines[i])
    assert all(lines[cases.index(c)].startswith("flagged") for c in dev if "_cut" in c.name)       # a cut file is always flagged


# ---------------------------------------------------------------------------------------------------------------- the kernels' resources
def test_jpeg_kernels_use_no_scratch():
    """The entropy loop keeps the byte window, four first-level lookups and the block's coefficient in registers and cannot afford a spill; 8 lanes
    a block in the IDCT, and launches 2 and 3 left apart, were chosen from this report."""
    seen = {}
    for name, r in kernel_resources("jpeg_decode.hip").items():
        kernel = next((k for k in ("jpeg_entropy_kernel", "jpeg_idct_kernel", "jpeg_colour_kernel") if k in name), None)
        if kernel is None:
            continue
        assert r.scratch == 0 and r.spills == (0, 0), (kernel, r, r.spills)
        seen[kernel] = (r.vgpr, r.lds)
    assert sorted(seen) == ["jpeg_colour_kernel", "jpeg_entropy_kernel", "jpeg_idct_kernel"], sorted(seen)
    assert seen["jpeg_entropy_kernel"][0] <= 64 and seen["jpeg_entropy_kernel"][1] <= 4096        # 1 KiB window + the tables' canonical part
    assert seen["jpeg_idct_kernel"][1] == 9216 and seen["jpeg_colour_kernel"][1] == 0
