"""The JPEG decoder beyond PIL's encoder, without a GPU: the edge fixtures (tests/golden/jpeg_edge_cases.npz: narrow chroma planes, header
layouts, table selections, magnitudes, the staging window's offsets, the largest sizes) against the restatement, stmask_amd.jpeg.parse and the
kernels' arithmetic run by the stand-alone host program under AddressSanitizer and UBSan; and the test-side writer (tests/jpeg_write.py)
against PIL.  Every comparison is exact equality with PIL's stored pixels.  No Python code runs under a sanitizer."""
import io

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restate
import jpeg_write as JW
from stmask_amd import _lib, jpeg

EDGE = JC.load_edge()
SEGMENT_BYTES = (1, 16, 63, 64, 65, 1023, 1024, 1025, 2048)


def _edge(name):
    return JC.edge_by_name(name)


def test_edge_fixture_set_is_the_one_the_generator_names():
    names = [c.name for c in EDGE]
    assert len(set(names)) == len(names) and {n.split("_")[0] for n in names} == set(JC.EDGE_GROUPS)
    for w in range(1, 7):
        for h in (1, 2, 9, 17):
            assert f"narrow_{w}x{h}_422" in names and f"narrow_{w}x{h}_420" in names
    for n in SEGMENT_BYTES:
        assert f"staging_segment_{n}" in names
    for what in ("stuffed_at_63", "stuffed_at_1023", "stuffed_at_2047", "stuffed_ends_segment", "code_straddles_1024", "value_straddles_1024"):
        assert "staging_" + what in names
    big = _lib.JPEG_MAX_DIM
    assert _edge(f"extent_{big}x8_420").rgb.shape == (8, big, 3) and _edge(f"extent_8x{big}_422").rgb.shape == (big, 8, 3)
    assert _edge(f"extent_8x{big}_grey_rst1").rgb.shape == (big, 8, 3)
    assert all(max(c.rgb.shape) <= big and c.rgb.shape[0] * c.rgb.shape[1] <= 8 * big for c in EDGE)        # nothing larger than 8192 x 8


def test_restatement_equals_every_edge_fixture_and_counts_what_the_set_must_hold():
    stats = {}
    for c in EDGE:
        assert np.array_equal(jpeg_restate.decode(c.data, stats), c.rgb), c.name
    assert all(stats[k] > 0 for k in jpeg_restate.EDGE_STAT_KEYS), stats
    assert stats["excursion"] < 384                # inside libjpeg's range-limit table: PIL's pixels are the one answer
    assert stats["restart_wraps"] >= 127 and stats["dc_size_11"] >= 2 and stats["dense_block"] >= 2
    # the narrow files whose chroma libjpeg replicates where an interpolation would give other samples, two planes each
    only = {}
    for c in EDGE:
        if c.name.startswith("narrow_"):
            jpeg_restate.decode(c.data, only)
    assert only["chroma_replicated"] == 2 * (2 * 4 + 4 * 2)


def test_parse_fields_of_the_layout_cases():
    base = jpeg.parse(JC.by_name("33x31_420_q75rst3").data)
    assert (base.tq, base.td, base.ta, base.dri, len(base.segments)) == ([0, 1, 1], [0, 1, 1], [0, 1, 1], 3, 2)
    same = ("width", "height", "ncomp", "hs", "vs", "mcu_w", "mcu_h", "dri")

    def fields(h):
        return [getattr(h, k) for k in same]
    for c in EDGE:
        if not c.name.startswith("layout_") or "grey_factors" in c.name or "restart_interval" in c.name:
            continue
        h = jpeg.parse(c.data)
        assert fields(h) == fields(base) and h.segments[:, 2:].tolist() == base.segments[:, 2:].tolist(), c.name
        assert c.data[h.ecs[1]:h.ecs[1] + 2] == b"\xff\xd9", c.name
        if c.name == "layout_huffman_ids_swapped":
            assert (h.td, h.ta, h.tq) == ([1, 0, 0], [1, 0, 0], [0, 1, 1])
            assert h.huff[0] == base.huff[1] and h.huff[1] == base.huff[0] and h.huff[2] == base.huff[3] and h.huff[3] == base.huff[2]
        elif c.name == "layout_quant_slots_2_3":
            assert h.tq == [2, 3, 3] and (h.td, h.ta) == (base.td, base.ta)
            assert np.array_equal(h.quant[2:], base.quant[:2]) and not h.quant[:2].any()
        else:
            assert (h.tq, h.td, h.ta) == (base.tq, base.td, base.ta) and h.huff == base.huff and np.array_equal(h.quant, base.quant), c.name
        if "fill" not in c.name:
            assert (np.diff(h.segments[:, :2]) == np.diff(base.segments[:, :2])).all(), c.name
    # fill bytes in front of a restart marker or the end-of-image marker stay with the segment in front: the reader stops at an FF without 00
    for name, restart, end in (("fill_restart", 1, 0), ("fill_end", 0, 3), ("fill_everywhere", 3, 1), ("fill_header", 0, 0)):
        c = _edge("layout_" + name)
        h = jpeg.parse(c.data)
        grow = np.diff(h.segments[:, :2])[:, 0] - np.diff(base.segments[:, :2])[:, 0]
        assert grow.tolist() == [restart] * (len(grow) - 1) + [end], name
        for k, (b, e, _, _) in enumerate(h.segments.tolist()):
            marker = b"\xff\xd9" if k == len(grow) - 1 else bytes([0xFF, 0xD0 + k])
            assert c.data[e:e + 2] == marker and c.data[e - int(grow[k]):e] == b"\xff" * int(grow[k]), name
    assert jpeg.parse(_edge("layout_fill_header").data).ecs[0] == base.ecs[0] + 2 * len(JW.split(JC.by_name("33x31_420_q75rst3").data)[0])
    for f in ("2x2", "4x1", "1x3"):                 # one component: its sampling factors mean nothing, an MCU is one block
        h = jpeg.parse(_edge(f"layout_grey_factors_{f}").data)
        assert (h.ncomp, h.hs, h.vs, h.mcu_w, h.mcu_h) == (1, 1, 1, 3, 2)
    for v in (0, 2, 3, 65535):                      # no restart marker in any of them: one segment of both MCUs
        h = jpeg.parse(_edge(f"layout_restart_interval_{v}").data)
        assert h.dri == v and h.segments[:, 2:].tolist() == [[0, 2]]
    h = jpeg.parse(_edge("layout_restart_interval_1_64x64").data)
    assert h.dri == 1 and h.segments[:, 2].tolist() == list(range(16)) and h.segments[:, 3].tolist() == [1] * 16


def test_parse_fields_of_the_table_and_extent_cases():
    h = jpeg.parse(_edge("tables_three_selections").data)
    assert (h.tq, h.td, h.ta) == ([0, 1, 2], [0, 1, 0], [0, 1, 1]) and h.quant[2].any() and not np.array_equal(h.quant[2], h.quant[1])
    h = jpeg.parse(_edge("tables_luma_on_1").data)
    assert (h.td, h.ta) == ([1, 0, 0], [1, 0, 0])
    h = jpeg.parse(_edge("tables_every_code_length").data)
    assert h.huff[0][0] == [1] * 16 and h.huff[2][0] == [1] * 16 and h.huff[1] is None and h.huff[3] is None
    t = _lib.JpegTables.from_buffer_copy(h.tables)
    for k in (0, 2):                                # the canonical codes 0, 10, 110, ...: the one of length l is 2^l - 2
        assert [t.huff[k].maxcode[length] for length in range(1, 17)] == [(1 << length) - 2 for length in range(1, 17)]
    h = jpeg.parse(_edge("tables_quant_255").data)
    assert h.quant.max() == 255
    h = jpeg.parse(_edge("tables_defined_twice").data)           # the later definition holds
    std = jpeg.parse(JC.by_name("33x31_420_q90").data)
    assert np.array_equal(h.quant, std.quant) and h.huff == std.huff and h.dri == 4 and len(h.segments) == 2
    big = _lib.JPEG_MAX_DIM
    h = jpeg.parse(_edge(f"extent_8x{big}_grey_rst1").data)
    assert h.dri == 1 and len(h.segments) == big // 8 and h.segments[:, 2].tolist() == list(range(big // 8))
    h = jpeg.parse(_edge(f"extent_{big}x8_420").data)
    assert (h.width, h.height, h.mcu_w, h.mcu_h) == (big, 8, big // 16, 1)
    h = jpeg.parse(_edge(f"extent_8x{big}_422").data)
    assert (h.width, h.height, h.mcu_w, h.mcu_h) == (8, big, 1, big // 8)


def test_staging_cases_put_their_bytes_where_their_names_say():
    for n in SEGMENT_BYTES:
        c = _edge(f"staging_segment_{n}")
        h = jpeg.parse(c.data)
        assert len(h.segments) == 2 and h.segments[0, 1] - h.segments[0, 0] == n
    for at in (63, 1023, 2047):
        c = _edge(f"staging_stuffed_at_{at}")
        b, e = jpeg.parse(c.data).segments[0, :2]
        assert c.data[b + at:b + at + 2] == b"\xff\x00" and e - b > at + 2
    c = _edge("staging_stuffed_ends_segment")
    e = int(jpeg.parse(c.data).segments[0, 1])
    assert c.data[e - 2:e + 2] == b"\xff\x00\xff\xd0"
    for kind in ("code", "value"):
        stats = {}
        jpeg_restate.decode(_edge(f"staging_{kind}_straddles_1024").data, stats)
        assert stats[f"{kind}_straddles_1024"] >= 1


# ---------------------------------------------------------------------------------------------------------------- the kernels' arithmetic on the host
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return JC.build_host_program(tmp_path_factory.mktemp("jpeg_edge_host"), sanitize=True)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_host_program_decodes_every_edge_fixture_bit_equal_under_sanitizers(host_program, tmp_path, order):
    batch = JC.write_job(tmp_path / "edge.job", EDGE, [0] * len(EDGE), order)
    assert batch.fallbacks == 0                                          # parse takes every one of them
    rc, lines, text = JC.run_host_program(host_program, tmp_path / "edge.job")
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert [c.name for i, c in enumerate(EDGE) if lines.get(i) != "equal"] == [] and rc == 0


# ---------------------------------------------------------------------------------------------------------------- the writer
def _written():
    """Small files straight from the writer: (name, bytes, reports)"""
    std = jpeg.parse(JC.by_name("33x31_420_q90").data)
    quant = {0: std.quant[0].astype(np.int64), 1: std.quant[1].astype(np.int64)}
    huff = {(0, 0): std.huff[0], (0, 1): std.huff[1], (1, 0): std.huff[2], (1, 1): std.huff[3]}
    rng = np.random.default_rng(3)

    def comps(w, h, fh, fv, sel):
        mw, mh = -(-w // (8 * fh)), -(-h // (8 * fv))
        out = []
        for c, (tq, td, ta) in enumerate(sel):
            a, b = (fh, fv) if c == 0 else (1, 1)
            plane = np.clip(128 + 90 * np.sin(np.arange(8 * a * mw) / 9.0 + c)[None, :] * np.cos(np.arange(8 * b * mh) / 7.0)[:, None] +
                            rng.normal(0, 12, (8 * b * mh, 8 * a * mw)), 0, 255)
            out.append(dict(id=c + 1, h=a, v=b, tq=tq, td=td, ta=ta, blocks=JW.quantise(plane, quant[tq])))
        return out
    plain = [(0, 0, 0), (1, 1, 1), (1, 1, 1)]
    yield "444", *JW.write(21, 13, comps(21, 13, 1, 1, plain), quant, huff)
    yield "422 restart 2", *JW.write(37, 9, comps(37, 9, 2, 1, plain), quant, huff, dri=2)
    yield "420 crossed", *JW.write(35, 27, comps(35, 27, 2, 2, [(1, 1, 0), (0, 0, 1), (1, 0, 0)]), quant, huff, dri=5, layout=dict(
        app="adobe", merged=True, fill={0xDB: 2, 0xC0: 1, 0xDA: 3, "rst": 2, 0xD9: 4}, extra=[(0xFE, b"\xff\xd9 a comment")], trailer=b"behind"))
    yield "grey 2x2 factors", *JW.write(19, 17, [dict(comps(19, 17, 1, 1, plain[:1])[0], h=2, v=2)], quant, huff, dri=1, layout=dict(app=None))
    decoy = dict(quant={0: quant[1]}, huff={(0, 0): huff[(0, 1)], (1, 0): huff[(1, 1)]})
    yield "defined twice", *JW.write(16, 16, comps(16, 16, 2, 2, plain), quant, huff, layout=dict(first=decoy))


def test_writer_round_trips_through_pil_and_reports_its_offsets():
    Image = pytest.importorskip("PIL.Image")
    seen = 0
    for name, data, reports in _written():
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(jpeg_restate.decode(data), ref), name
        h = jpeg.parse(data)
        assert len(reports) == len(h.segments), name
        fill = 2 if "crossed" in name else 0
        for k, (rep, (b, e, _, count)) in enumerate(zip(reports, h.segments.tolist())):
            seg = data[b:e]
            assert rep["length"] == len(seg) - (fill if k < len(reports) - 1 else 4 * bool(fill)), name
            assert rep["stuffed"] == [i for i in range(rep["length"] - 1) if seg[i] == 0xFF and seg[i + 1] == 0], name
            assert len(rep["blocks"]) == count * (1 if h.ncomp == 1 else h.hs * h.vs + 2) and rep["blocks"] == sorted(rep["blocks"]) and rep["blocks"][0] == 0
            assert all(0 <= first <= last < rep["length"] for _, first, last in rep["fields"]) and rep["fields"][0][0] == "code"
            seen += len(rep["stuffed"])
    assert seen > 0


def test_header_rewrites_keep_the_pixels():
    """The rewrites the layout fixtures were made with, on another file: a rewritten file still parses and the restatement decodes the same pixels"""
    c = JC.by_name("48x40_422_q75rst3")
    for data in (JW.with_huffman_ids_swapped(c.data), JW.with_quant_slots(c.data, {0: 3, 1: 2}), JW.with_tables_merged(c.data),
                 JW.with_component_ids(c.data, (9, 8, 7)), JW.with_fill(c.data, header=1, restart=2, end=1),
                 JW.with_segments(JW.without(c.data, 0xE0), [(0xEE, JW.ADOBE_YCC)])):
        assert data != c.data and jpeg.parse(data).shape == c.rgb.shape
        assert np.array_equal(jpeg_restate.decode(data), c.rgb)
    assert JW.join(*JW.split(c.data)) == c.data
