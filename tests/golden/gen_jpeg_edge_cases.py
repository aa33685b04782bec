"""Writes tests/golden/jpeg_edge_cases.npz: JPEG files beyond what PIL's encoder writes and tests/golden/jpeg_cases.npz reaches, each with its
bytes and PIL's decoded RGB (tests/jpeg_cases.py load_edge()).

    python tests/golden/gen_jpeg_edge_cases.py

Six groups; a case's name starts with its group.
  narrow      widths 1..6 x heights 1, 2, 9, 17 x 4:2:2 and 4:2:0, PIL at quality 90 on noise: chroma planes of one, two and three columns
              (libjpeg replicates the first two, interpolates from three on).
  layout      header rewrites (tests/jpeg_write.py) of grid fixtures: Huffman ids swapped, quantisation slots 2 and 3, merged table segments,
              other component ids with and without a JFIF marker, an Adobe marker, long COM / APP1 segments, bytes behind the end-of-image
              marker, sampling factors on a grey frame, restart intervals of 0, the MCU count, more, 65535 and 1, fill bytes.
  tables      written by tests/jpeg_write.py: three components on three different (quantisation, DC, AC) selections, luma on tables 1 and
              chroma on 0, DC and AC tables with one code of every length 1..16 whose 10- to 16-bit codes are used, a quantisation entry of
              255, a table defined twice.
  magnitudes  a DC difference of size 11 (8 x 8 checker, quality 100), an AC value of size 10 at k = 63, a block of 63 coefficients of the
              largest size that fits.  Every case keeps |sample - 128| below 384 behind the IDCT (asserted in the restatement): libjpeg's
              range-limit table is exact only there, and beyond it its C and SIMD transforms disagree, so PIL is no oracle.  For 63
              coefficients that rules size 10 out (the transform is orthonormal: 63 values of 512 or more put the samples' RMS above 508)
              and DENSE_SIZE = 8 is the largest size for which dense_block()'s search finds a block; it found none of size 9.
  staging     restart segments of exactly SEGMENT_BYTES bytes; a stuffed FF at segment offsets 63, 1023 and 2047 (its 00 opens the next
              64-byte group or 1 KiB window of the kernel's reader); a stuffed pair as the last two bytes of a segment; a Huffman code and a
              value field across offset 1024.  Found by seeded search over the writer's output and asserted from the writer's offsets.
  extent      8192 x 8 at 4:2:0, 8 x 8192 at 4:2:2, a grey 8 x 8192 frame with a restart interval of 1 (1024 segments).

For every case the script asserts that PIL decodes it, that stmask_amd.jpeg.parse takes it (no host fallback) and that the restatement
(tests/jpeg_restate.py) equals PIL; it runs the host program (tests/jpeg_host_main.cpp) under AddressSanitizer and UBSan on all of them and
requires "equal"; and it fails when one of jpeg_restate.EDGE_STAT_KEYS was never counted."""
import io
import os
import sys
import tempfile

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_cases as JC  # noqa: E402
import jpeg_restate  # noqa: E402
import jpeg_write as JW  # noqa: E402

from stmask_amd import _lib, jpeg  # noqa: E402

SEGMENT_BYTES = (1, 16, 63, 64, 65, 1023, 1024, 1025, 2048)
DENSE_SIZE = 8
RANGE = 384


def encode(a, **kw):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


def smooth(w, h, c=3):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([127 + 100 * np.sin(xx / (37.0 + 11 * k) + k) * np.cos(yy / (29.0 + 5 * k)) for k in range(c)], -1)
    return np.clip(a, 0, 255).astype(np.uint8)


def standard_tables():
    """The tables PIL writes without optimize (Annex K's Huffman tables, quality 90's quantisation tables), read from a grid fixture."""
    h = jpeg.parse(JC.by_name("33x31_420_q90").data)
    huff = {(0, 0): h.huff[0], (0, 1): h.huff[1], (1, 0): h.huff[2], (1, 1): h.huff[3]}
    return {0: h.quant[0].astype(np.int64), 1: h.quant[1].astype(np.int64)}, huff


def colour_components(rng, w, h, quant, sel, ids=(1, 2, 3)):
    """4:2:0 components over smooth content with some noise; sel: (tq, td, ta) per component."""
    mw, mh = -(-w // 16), -(-h // 16)
    comps = []
    for c, (tq, td, ta) in enumerate(sel):
        f = 2 if c == 0 else 1
        plane = smooth(8 * f * mw, 8 * f * mh, 3)[:, :, c].astype(np.float64) + rng.normal(0, 6, (8 * f * mh, 8 * f * mw))
        comps.append(dict(id=ids[c], h=f, v=f, tq=tq, td=td, ta=ta, blocks=JW.quantise(np.clip(plane, 0, 255), quant[tq])))
    return comps


def grey(blocks, **kw):
    return [dict(dict(id=1, h=1, v=1, tq=0, td=0, ta=0, blocks=blocks), **kw)]


def dense_block(size, seed=0, iters=4000):
    """63 AC coefficients of size category `size` whose samples stay inside RANGE: alternating projections between the two sets."""
    lo, hi = 1 << (size - 1), (1 << size) - 1
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(0.125), 0.5)[:, None]
    x = np.random.default_rng(seed).choice([-1.0, 1.0], (8, 8)) * RANGE * 0.8
    for _ in range(iters):
        f = basis @ x @ basis.T
        dc = f[0, 0]
        f = np.sign(f + 1e-9) * np.clip(np.abs(f), lo + 2, hi - 2)
        f[0, 0] = np.clip(dc, -200, 200)
        fi = np.rint(f).astype(np.int64)
        if np.abs(jpeg_restate.idct_raw(fi.reshape(1, 8, 8))).max() < RANGE:
            return fi.reshape(64)
        x = np.clip(basis.T @ f @ basis, -(RANGE - 15), RANGE - 15)
    return None


# ---------------------------------------------------------------------------------------------------------------- the staging window
class Segment:
    """A restart segment of grey blocks with DC 0 being shaped: each block's bits are its own, so a change re-encodes one block."""

    def __init__(self, n, dc, ac):
        self.blocks, self.dc, self.ac = np.zeros((n, 64), dtype=np.int64), dc, ac
        self.bits = [self._bits(i) for i in range(n)]

    def _bits(self, i):
        return "".join(format(v, f"0{w}b") for _, v, w in JW.block_fields(self.blocks[i], 0, self.dc, self.ac))

    def set(self, i, k, v):
        self.blocks[i, JW.ZZ[k]] = v
        self.bits[i] = self._bits(i)

    def length(self):
        bits = "".join(self.bits)
        bits += "1" * (-len(bits) % 8)
        raw = int(bits, 2).to_bytes(len(bits) // 8, "big")
        return len(raw) + raw.count(b"\xff")


def value(rng):
    """A small coefficient, often all ones in its bits (2^s - 1): those make FF bytes"""
    s = int(rng.integers(1, 5))
    return (1 << s) - 1 if rng.random() < 0.5 else int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))


def segment_of(rng, nbytes, dc, ac):
    """-> blocks [n, 64] of a segment of exactly nbytes bytes (stuffing included): coefficients are added and removed until the length fits."""
    seg = Segment(-(-nbytes // 30), dc, ac)
    n = len(seg.blocks)
    for _ in range(200000):
        got = seg.length()
        if got == nbytes:
            return seg.blocks
        i, k = int(rng.integers(n)), int(rng.integers(1, 64))
        if got < nbytes and np.count_nonzero(seg.blocks[i]) < 60:
            seg.set(i, k, value(rng))
        elif got > nbytes:
            nz = np.flatnonzero(seg.blocks[i])
            if nz.size:
                seg.blocks[i, nz[int(rng.integers(nz.size))]] = 0
                seg.bits[i] = seg._bits(i)
    raise AssertionError(f"no segment of {nbytes} bytes")


def noise_blocks(rng, n, last_at_63=False):
    b = np.zeros((n, 64), dtype=np.int64)
    for i in range(n):
        for k in rng.choice(np.arange(1, 64), int(rng.integers(20, 45)), replace=False):
            b[i, JW.ZZ[k]] = value(rng)
    if last_at_63:
        b[-1, 63] = 15
    return b


def staging_file(first, rng, quant, huff):
    """Two rows of grey blocks, one restart segment a row: `first` is the upper row's blocks; -> (bytes, reports)."""
    n = len(first)
    second = noise_blocks(rng, n) // 2
    return JW.write(8 * n, 16, grey(np.stack([first, second])), {0: quant}, huff, dri=n)


def main():
    print(f"PIL {PIL.__version__}, libjpeg {features.version('jpg')}{' (libjpeg-turbo)' if features.check_feature('libjpeg_turbo') else ''}")
    rng = np.random.default_rng(20241021)
    names, out, stats = [], {}, {}
    cases = []

    def add(name, data):
        assert name.split("_")[0] in JC.EDGE_GROUPS and name not in names, name
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))              # PIL decodes it
        jpeg.parse(data)                                                           # ... parse takes it: no host fallback
        before = stats.get("excursion", 0)
        stats["excursion"] = 0
        got = jpeg_restate.decode(data, stats)
        assert stats["excursion"] < RANGE, (name, stats["excursion"])
        stats["excursion"] = max(stats["excursion"], before)
        assert np.array_equal(got, ref), name                                      # ... and the restatement equals PIL
        out[f"data_{len(names)}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"rgb_{len(names)}"] = ref
        names.append(name)
        cases.append(JC.Case(name, data, ref))

    def counted(key, since):
        assert stats[key] > since.get(key, 0), f"{names[-1]} does not add to {key}"

    # ---- narrow
    for w in range(1, 7):
        for h in (1, 2, 9, 17):
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            for sname, ss in (("422", 1), ("420", 2)):
                add(f"narrow_{w}x{h}_{sname}", encode(a, quality=90, subsampling=ss))
    assert stats["chroma_replicated"] == 2 * (2 * 4 + 4 * 2)       # two planes each: 4:2:2 widths 3, 4 at every height; 4:2:0 widths 1..4, heights 9, 17

    # ---- layout
    base = JC.by_name("33x31_420_q75rst3").data
    own = JC.by_name("1x1_444_q90").data
    marker_like = (b"\xff\xd9\xff\xda\x00\x0c\xff\xc0\xff\xd0\xff\x00\xff\xff\xc4" * 4400)[:65533]
    layout = {
        "huffman_ids_swapped": JW.with_huffman_ids_swapped(base),
        "quant_slots_2_3": JW.with_quant_slots(base, {0: 2, 1: 3}),
        "tables_merged": JW.with_tables_merged(base),
        "ids_0_1_2": JW.with_component_ids(base, (0, 1, 2)),
        "ids_7_9_200": JW.with_component_ids(base, (7, 9, 200)),
        "ids_rgb_under_jfif": JW.with_component_ids(base, (82, 71, 66)),
        "no_jfif_ids_1_2_3": JW.without(base, 0xE0),
        "no_jfif_ids_0_1_2": JW.with_component_ids(JW.without(base, 0xE0), (0, 1, 2)),
        "no_jfif_ids_5_6_7": JW.with_component_ids(JW.without(base, 0xE0), (5, 6, 7)),
        "adobe_transform_1": JW.with_segments(JW.without(base, 0xE0), [(0xEE, JW.ADOBE_YCC)]),
        "com_65k_marker_like": JW.with_segments(base, [(0xFE, marker_like)]),
        "app1_holds_a_jpeg": JW.with_segments(base, [(0xE1, b"Exif\0\0" + base)]),
        "thirty_segments": JW.with_segments(base, [(0xFE, b"segment %d" % k) for k in range(24)]),
        "bytes_behind_eoi": base + b"\xff\xd8\xff\xda\x00\x03" + own + bytes(range(256)),
        "fill_header": JW.with_fill(base, header=2),
        "fill_restart": JW.with_fill(base, restart=1),
        "fill_end": JW.with_fill(base, end=3),
        "fill_everywhere": JW.with_fill(base, header=1, restart=3, end=1),
    }
    g = JC.by_name("17x9_grey_q90").data
    for f in (0x22, 0x41, 0x13):
        layout[f"grey_factors_{f >> 4}x{f & 15}"] = JW.patched(g, 0xC0, 7, f)
    r = JC.by_name("17x9_420_q90").data
    assert jpeg.parse(r).mcu_w * jpeg.parse(r).mcu_h == 2
    for v in (0, 2, 3, 65535):
        layout[f"restart_interval_{v}"] = JW.with_segments(r, [(0xDD, v.to_bytes(2, "big"))], before=0xDA)
    layout["restart_interval_1_64x64"] = encode(smooth(64, 64), quality=90, subsampling=2, restart_marker_blocks=1)
    before = dict(stats)
    for name, data in layout.items():
        add("layout_" + name, data)
    for key in ("header_fill", "restart_fill", "end_fill"):
        counted(key, before)
    assert len(jpeg.parse(layout["restart_interval_1_64x64"]).segments) == 16
    assert len(JW.split(layout["thirty_segments"])[0]) > 19

    # ---- tables
    quant, huff = standard_tables()
    q3 = {0: quant[0], 1: quant[1], 2: np.clip(quant[1][::-1] + 3, 1, 255)}
    before = dict(stats)
    add("tables_three_selections", JW.write(35, 27, colour_components(rng, 35, 27, q3, [(0, 0, 0), (1, 1, 1), (2, 0, 1)]), q3, huff)[0])
    counted("tables_crossed", before)
    crossed = {(0, 0): huff[(0, 1)], (0, 1): huff[(0, 0)], (1, 0): huff[(1, 1)], (1, 1): huff[(1, 0)]}
    add("tables_luma_on_1", JW.write(35, 27, colour_components(rng, 35, 27, quant, [(0, 1, 1), (1, 0, 0), (1, 0, 0)]), quant, crossed)[0])
    counted("luma_on_table_1", before)
    # one code of every length: DC sizes 0..6 and seven AC symbols sit on the 10- to 16-bit codes
    dc16 = ([1] * 16, [15, 14, 13, 12, 11, 10, 9, 8, 7, 0, 1, 2, 3, 4, 5, 6])
    ac16 = ([1] * 16, [0x01, 0x00, 0x02, 0x11, 0x03, 0x21, 0xF0, 0x12, 0x31, 0x04, 0x41, 0x13, 0x22, 0x51, 0x05, 0x61])
    blocks, dc = np.zeros((3, 5, 64), dtype=np.int64), 0
    for i in range(15):
        s = i % 7
        mag = int(rng.integers(1 << (s - 1), 1 << s)) if s else 0
        dc += -mag if dc > 0 else mag
        blocks[i // 5, i % 5, 0] = dc
        k = 1
        for sym in rng.permutation([s for s in ac16[1] if s not in (0x00, 0xF0)])[:int(rng.integers(4, 12))].tolist() + [0xF0, 0x04 + (i % 2)]:
            if sym == 0xF0:
                k += 16
                continue
            k += sym >> 4
            if k > 63:
                break
            s = sym & 15
            blocks[i // 5, i % 5, JW.ZZ[k]] = int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))
            k += 1
    ones = np.ones(64, dtype=np.int64) * 2
    add("tables_every_code_length", JW.write(37, 19, grey(blocks), {0: ones}, {(0, 0): dc16, (1, 0): ac16})[0])
    for kind in ("dc", "ac"):
        for length in range(10, 17):
            counted(f"{kind}_code_{length}", before)
    q255 = {0: quant[0].copy(), 1: quant[1].copy()}
    q255[0][[63, 10]] = 255
    q255[1][9] = 255
    comps = colour_components(rng, 35, 27, q255, [(0, 0, 0), (1, 1, 1), (1, 1, 1)])
    comps[0]["blocks"][1, 2, 63], comps[0]["blocks"][2, 3, 10], comps[1]["blocks"][0, 1, 9] = 1, -1, 1
    add("tables_quant_255", JW.write(35, 27, comps, q255, huff)[0])
    counted("quant_255", before)
    decoy = dict(quant={0: quant[1][::-1].copy(), 1: quant[0]}, huff={(0, 0): huff[(0, 1)], (1, 1): huff[(1, 0)]})
    lay = dict(app="adobe", merged=True, first=decoy, fill={0xDB: 1, 0xC4: 2, 0xC0: 1, "rst": 2, 0xD9: 1}, extra=[(0xFE, b"written twice")], trailer=b"\0\xff")
    data, reports = JW.write(35, 27, colour_components(rng, 35, 27, quant, [(0, 0, 0), (1, 1, 1), (1, 1, 1)], ids=(3, 2, 1)), quant, huff, dri=4, layout=lay)
    add("tables_defined_twice", data)
    h = jpeg.parse(data)
    assert len(reports) == len(h.segments) == 2 and np.array_equal(h.quant[0], quant[0]) and h.huff[0] == (list(huff[(0, 0)][0]), list(huff[(0, 0)][1]))

    # ---- magnitudes
    checker = np.kron(np.indices((2, 4)).sum(0) % 2, np.ones((8, 8))).astype(np.uint8) * 255
    before = dict(stats)
    add("magnitudes_dc_size_11_grey", encode(checker, quality=100))
    counted("dc_size_11", before)
    before = dict(stats)
    add("magnitudes_dc_size_11_444", encode(np.stack([checker, 255 - checker, checker], -1), quality=100, subsampling=0))
    counted("dc_size_11", before)
    one = {0: np.ones(64, dtype=np.int64)}
    blocks = np.zeros((1, 2, 64), dtype=np.int64)
    blocks[0, 0, 63], blocks[0, 1, 63], blocks[0, 1, 0] = 1023, -600, 40
    add("magnitudes_ac_size_10_at_63", JW.write(16, 8, grey(blocks), one, huff)[0])
    counted("ac_size_10_at_63", before)
    assert dense_block(10, iters=50) is None and dense_block(DENSE_SIZE + 1) is None, "a larger dense block exists: raise DENSE_SIZE"
    dense = dense_block(DENSE_SIZE)
    assert (np.abs(dense[1:]) >= 1 << (DENSE_SIZE - 1)).all()
    before = dict(stats)
    add("magnitudes_dense_block", JW.write(16, 8, grey(np.stack([dense, -dense])[None]), one, huff)[0])
    assert stats["dense_block"] == before["dense_block"] + 2

    # ---- staging
    dc, ac = JW.codes_of(*huff[(0, 0)]), JW.codes_of(*huff[(1, 0)])
    for nbytes in SEGMENT_BYTES:
        data, reports = staging_file(segment_of(rng, nbytes, dc, ac), rng, one[0], huff)
        assert reports[0]["length"] == nbytes and np.diff(jpeg.parse(data).segments[0, :2]) == nbytes
        add(f"staging_segment_{nbytes}", data)

    def search(what, nbytes, found, **kw):
        for seed in range(4000):
            r = np.random.default_rng(seed)
            data, reports = staging_file(noise_blocks(r, -(-nbytes // 15), **kw), r, one[0], huff)
            if found(reports[0]):
                before = dict(stats)
                add(f"staging_{what}", data)
                counted(what, before)
                return
        raise AssertionError(f"no file with {what}")
    for at in (63, 1023, 2047):
        search(f"stuffed_at_{at}", at + 120, lambda rep, at=at: at in rep["stuffed"] and rep["length"] > at + 2)
    search("stuffed_ends_segment", 200, lambda rep: rep["stuffed"] and rep["stuffed"][-1] == rep["length"] - 2, last_at_63=True)
    for kind in ("code", "value"):
        search(f"{kind}_straddles_1024", 1200, lambda rep, kind=kind: any(k == kind and b < 1024 <= e for k, b, e in rep["fields"]))

    # ---- extent
    big = _lib.JPEG_MAX_DIM
    before = dict(stats)
    add(f"extent_{big}x8_420", encode(smooth(big, 8), quality=90, subsampling=2))
    add(f"extent_8x{big}_422", encode(smooth(8, big), quality=90, subsampling=1))
    add(f"extent_8x{big}_grey_rst1", encode(smooth(8, big, 1)[:, :, 0], quality=90, restart_marker_blocks=1))
    assert len(jpeg.parse(cases[-1].data).segments) == big // 8 and stats["restart_wraps"] - before["restart_wraps"] >= 127
    counted("dimension_over_160", before)
    counted("segments_over_19", before)

    missing = [k for k in jpeg_restate.EDGE_STAT_KEYS if not stats.get(k)]
    assert not missing, f"the set lacks {missing}: {stats}"

    # the kernels' arithmetic on the CPU under the sanitizers: every case equal
    with tempfile.TemporaryDirectory() as tmp:
        exe = JC.build_host_program(tmp, sanitize=True)
        JC.write_job(os.path.join(tmp, "edge.job"), cases, [0] * len(cases))
        rc, lines, text = JC.run_host_program(exe, os.path.join(tmp, "edge.job"))
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    differ = [c.name for i, c in enumerate(cases) if lines.get(i) != "equal"]
    assert rc == 0 and not differ, differ
    path = os.path.join(HERE, "jpeg_edge_cases.npz")
    np.savez_compressed(path, names=np.array(names), **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"{path}: {len(names)} cases, {size} bytes; {stats}")


if __name__ == "__main__":
    main()
