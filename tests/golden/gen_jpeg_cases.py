"""Writes tests/golden/jpeg_cases.npz: the JPEG fixtures of tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py.  Synthetic images, PIL as encoder
and as oracle: every case holds the file's bytes and PIL's decoded RGB.

    python tests/golden/gen_jpeg_cases.py

The grid: sizes 1x1, 7x5, 8x8, 16x16, 17x9, 33x31, 48x40, 64x50 (width x height) x sampling 4:4:4, 4:2:2, 4:2:0, grey x encodings quality 90;
quality 30 with optimize=True; quality 75 with restart_marker_blocks=3; quality 100 on uniform noise -- plus 96x160 at 4:2:0 with
restart_marker_rows=1, plus two files the device path does not decode (progressive, CMYK) with PIL's pixels, plus damaged files: each of
DAMAGE_SOURCES cut at 25 %, 50 % and 99 % of its entropy-coded bytes (the end-of-image marker put back) and with one of those bytes inverted at
five seeded positions, each with PIL's pixels for the damaged bytes (an empty array where PIL refuses the file) and with the verdict of the
host program (tests/jpeg_host_main.cpp) run here under AddressSanitizer and UBSan: flagged with its status word, equal, or refused by parse.  The script asserts that the
restatement (tests/jpeg_restate.py) equals PIL on every case, that stmask_amd.jpeg.parse takes every grid case (no host fallback), and, by
counting in the restatement, that the set contains what a decoder can get wrong: a stuffed FF 00, a ZRL symbol, a block whose last coefficient
sits at k = 63, a Huffman code longer than the first-level lookup, a pixel clamped at 0 and one at 255, a restart interval that does not divide
the MCUs of a row, a chroma plane one column wide."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_restate  # noqa: E402

from stmask_amd import jpeg  # noqa: E402

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (48, 40), (64, 50)]
SAMPLING = [("444", 0), ("422", 1), ("420", 2), ("grey", None)]
DAMAGE_SOURCES = ("33x31_420_q90", "48x40_444_q75rst3", "64x50_422_q30opt")
ENCODINGS = [("q90", dict(quality=90), False), ("q30opt", dict(quality=30, optimize=True), False),
             ("q75rst3", dict(quality=75, restart_marker_blocks=3), False), ("q100noise", dict(quality=100), True)]


def smooth(rng, w, h):
    """A smooth field with strong edges and some noise: saturated regions (clamping), long zero runs (ZRL) and fine detail alike."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([127 + 140 * np.sin(xx / (5.0 + c)) * np.cos(yy / 7.0) for c in range(3)], -1) + rng.normal(0, 10, (h, w, 3))
    a[(xx + yy) % 23 == 0] = 255
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, **kw):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    rng = np.random.default_rng(20240607)
    names, out, stats = [], {}, {}

    def add(name, data, check=True, may_fail=False):
        try:
            ref = pil_rgb(data)
        except Exception:
            if not may_fail:
                raise
            ref = np.zeros(0, dtype=np.uint8)
        if check:
            jpeg.parse(data)                                        # SOF0, or this raises: no host fallback on the grid
            got = jpeg_restate.decode(data, stats)
            assert np.array_equal(got, ref), name
        out[f"data_{len(names)}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"rgb_{len(names)}"] = ref
        names.append(name)

    for w, h in SIZES:
        images = {False: smooth(rng, w, h), True: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)}
        for sname, ss in SAMPLING:
            for ename, kw, noise in ENCODINGS:
                a = images[noise]
                data = encode(a[:, :, 1], **kw) if ss is None else encode(a, subsampling=ss, **kw)
                add(f"{w}x{h}_{sname}_{ename}", data)
    add("96x160_420_rstrows1", encode(smooth(rng, 96, 160), quality=90, subsampling=2, restart_marker_rows=1))
    n_grid = len(names)
    a = smooth(rng, 33, 31)
    add("unsupported_progressive", encode(a, quality=90, progressive=True), check=False)
    bio = io.BytesIO()
    Image.fromarray(np.dstack([a, 255 - a[:, :, :1]]), "CMYK").save(bio, "JPEG", quality=90)
    add("unsupported_cmyk", bio.getvalue(), check=False)
    for name in names[n_grid:]:
        try:
            jpeg.parse(out[f"data_{names.index(name)}"].tobytes())
        except jpeg.Unsupported:
            continue
        raise AssertionError(f"{name} is not refused")
    n_whole = len(names)
    pos_rng = np.random.default_rng(7)
    for src in DAMAGE_SOURCES:
        data = out[f"data_{names.index(src)}"].tobytes()
        begin, end = jpeg.parse(data).ecs
        for pct in (25, 50, 99):
            add(f"{src}_cut{pct}", data[:begin + (end - begin) * pct // 100] + b"\xff\xd9", check=False, may_fail=True)
        for pos in pos_rng.integers(begin, end, 5).tolist():
            d = bytearray(data)
            d[pos] ^= 0xFF
            add(f"{src}_flip{pos}", bytes(d), check=False, may_fail=True)
    # how the host program ends each damaged file under the sanitizers (tests/jpeg_host_main.cpp; tests/test_jpeg_cpu.py repeats the run and
    # compares): stored, so that the GPU test knows which files the device must flag, and with which status word, without building anything
    import tempfile
    import jpeg_cases
    cases = [jpeg_cases.Case(n, out[f"data_{i}"].tobytes(), out[f"rgb_{i}"] if out[f"rgb_{i}"].size else None) for i, n in enumerate(names)][n_whole:]
    dev = []
    for c in cases:
        try:
            jpeg.parse(c.data)
            dev.append(c)
        except ValueError:
            out[f"verdict_{names.index(c.name)}"] = np.array("refused")
    with tempfile.TemporaryDirectory() as tmp:
        exe = jpeg_cases.build_host_program(tmp, sanitize=True)
        jpeg_cases.write_job(os.path.join(tmp, "damaged.job"), dev, [1] * len(dev))
        rc, lines, text = jpeg_cases.run_host_program(exe, os.path.join(tmp, "damaged.job"))
    assert rc == 0 and "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    for i, c in enumerate(dev):
        assert lines[i].startswith("flagged") or (lines[i] == "equal" and c.rgb is not None), (c.name, lines[i])
        out[f"verdict_{names.index(c.name)}"] = np.array(lines[i])
    missing = [k for k in jpeg_restate.STAT_KEYS if not stats.get(k)]
    assert not missing, f"the set lacks {missing}: {stats}"
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, names=np.array(names), n_grid=np.int64(n_grid), n_whole=np.int64(n_whole), **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"{path}: {len(names)} cases, {size} bytes; {stats}")


if __name__ == "__main__":
    main()
