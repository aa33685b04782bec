"""The files and the host program of the split entropy decode (csrc/jpeg_split.hip, csrc/jpeg_split_core.h), shared by
tests/test_jpeg_split_cpu.py and tests/test_gpu_jpeg_split.py.  Nothing large is stored: the files are made here, at test time, with
tests/jpeg_write.py, and their expected pixels come from tests/jpeg_restate.py; the stored fixtures (tests/jpeg_cases.py) bring the rest.

tests/jpeg_split_host_main.cpp is the model: it runs the lanes' arithmetic with the kernels' grouping and round count in plain loops and says,
per image, whether it was decoded split, left serial, or redone by the serial decode."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np

import jpeg_cases as JC
import jpeg_restate
import jpeg_write as JW
from stmask_amd import _lib, jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
SUB, GROUP, ROUNDS = _lib.JPEG_SUB_BYTES, _lib.JPEG_SUB_GROUP, _lib.JPEG_SPLIT_ROUNDS
GROUP_BYTES = SUB * GROUP

# the standard tables of the JPEG specification's annex K, which every encoder's defaults are
DC_L = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_L = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
        [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42,
         0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35,
         0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67,
         0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98,
         0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
         0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4,
         0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
        [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1,
         0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A,
         0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66,
         0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96,
         0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
         0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4,
         0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
HUFF = {(0, 0): DC_L, (0, 1): DC_C, (1, 0): AC_L, (1, 1): AC_C}
QUANT = {0: [2] * 64, 1: [3] * 64}
MODES = {"grey": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}        # components, luma sampling: 1, 3, 4 and 6 blocks an MCU


def sparse_blocks(rng, rows, cols, density):
    """Quantised blocks [rows, cols, 64] as a noisy picture has them: a DC level that wanders and a few small AC coefficients, mostly early."""
    b = np.zeros((rows, cols, 64), dtype=np.int64)
    b[:, :, 0] = rng.integers(-200, 200, size=(rows, cols))
    weight = density * np.exp(-np.arange(1, 64) / 12.0)
    on = rng.random((rows, cols, 63)) < weight
    mag = rng.integers(1, 24, size=(rows, cols, 63)) * rng.choice([-1, 1], size=(rows, cols, 63))
    zz = np.array(JW.ZZ[1:])
    b[:, :, zz] = np.where(on, mag, 0)
    return b


def components(rng, mode, mcu_w, mcu_h, density=2.0):
    n, hs, vs = MODES[mode]
    comps = [dict(id=1, h=hs, v=vs, tq=0, td=0, ta=0, blocks=sparse_blocks(rng, mcu_h * vs, mcu_w * hs, density))]
    for c in range(1, n):
        comps.append(dict(id=1 + c, h=1, v=1, tq=1, td=1, ta=1, blocks=sparse_blocks(rng, mcu_h, mcu_w, density / 2)))
    return comps, hs, vs


def ecs_of(data):
    """(begin, end) of a file's entropy-coded data"""
    h = jpeg.parse(data)
    return int(h.ecs[0]), int(h.ecs[1])


def make(mode, mcu_w, mcu_h, seed, density=2.0):
    """-> (file bytes, the writer's report of its one segment)"""
    rng = np.random.default_rng(seed)
    comps, hs, vs = components(rng, mode, mcu_w, mcu_h, density)
    data, reports = JW.write(8 * hs * mcu_w, 8 * vs * mcu_h, comps, QUANT, HUFF)
    return data, reports[0]


def repeated_rows(mode, mcu_w, rows, seed, density=2.0):
    """A file of `rows` MCU rows that all hold the same blocks but the first, whose DC levels start from zero predictions: the entropy-coded bits of
    a row whose predecessor ends on the same DC levels are the same, so row 1's bits are packed once and repeated.  (The Python writer is too slow
    for fresh content of this size.)  -> file bytes"""
    rng = np.random.default_rng(seed)
    comps, hs, vs = components(rng, mode, mcu_w, 1, density)
    one, _ = JW.write(8 * hs * mcu_w, 8 * vs, comps, QUANT, HUFF)
    codes = [(JW.codes_of(*HUFF[(0, c["td"])]), JW.codes_of(*HUFF[(1, c["ta"])])) for c in comps]

    def row_bits(pred):
        bits = []
        for mx in range(mcu_w):
            for ci, c in enumerate(comps):
                h, v = (hs, vs) if ci == 0 else (1, 1)
                for by in range(v):
                    for bx in range(h):
                        block = c["blocks"][by][mx * h + bx]
                        bits.extend(format(value, f"0{width}b") for _, value, width in JW.block_fields(block, pred[ci], *codes[ci]))
                        pred[ci] = int(block[0])
        return "".join(bits)
    pred = [0] * len(comps)
    first = row_bits(pred)
    again = row_bits(pred)                                  # from the levels the row ends on: what every later row starts from
    bits = first + again * (rows - 1)
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    segs, _ = JW.split(one)
    for s in segs:
        if s[0] == 0xC0:
            s[1] = s[1][:1] + (8 * vs * rows).to_bytes(2, "big") + s[1][3:]
    return JW.join(segs, raw + b"\xff\xd9")


Case = JC.Case


@functools.lru_cache(maxsize=None)
def expected(data):
    rgb = jpeg_restate.decode(data)
    rgb.setflags(write=False)
    return rgb


def case(name, data):
    return Case(name, data, expected(data))


def _sized(mode, target, seed):
    """The smallest file of `mode`, 8 MCUs wide, whose data has `target` bytes or more."""
    rows = 1
    while True:
        data, rep = make(mode, 8, rows, seed)
        if rep["length"] >= target:
            return data, rep
        rows += max(1, int(rows * (target / rep["length"] - 1)))


@functools.lru_cache(maxsize=None)
def multi_group():
    """Per mode, one file of more than ROUNDS + 2 groups of data (the sizes are checked here): -> [Case]"""
    out = []
    for k, mode in enumerate(MODES):
        data, rep = _sized(mode, (ROUNDS + 2) * GROUP_BYTES + 1, 100 + k)
        assert rep["length"] > (ROUNDS + 2) * GROUP_BYTES and rep["length"] < (ROUNDS + 4) * GROUP_BYTES, (mode, rep["length"])
        out.append(case(f"groups_{mode}", data))
    return out


def _with_length(target, seed, mode="grey"):
    """A file whose data has exactly `target` bytes: blocks are added one MCU column at a time, then the last block's coefficients are thinned or
    thickened until the length is met."""
    rng = np.random.default_rng(seed)
    for mcu_w in range(1, 400):
        comps, hs, vs = components(np.random.default_rng(seed), mode, mcu_w, 1)
        data, reports = JW.write(8 * hs * mcu_w, 8 * vs, comps, QUANT, HUFF)
        if reports[0]["length"] >= target - 8:
            break
    last = comps[0]["blocks"][0][mcu_w - 1]
    for _ in range(4000):
        n = reports[0]["length"]
        if n == target:
            return data, reports[0]
        k = int(rng.integers(1, 64))
        last[JW.ZZ[k]] = 0 if n > target else int(rng.integers(1, 1 << int(rng.integers(1, 10))))
        data, reports = JW.write(8 * hs * mcu_w, 8 * vs, comps, QUANT, HUFF)
    raise AssertionError(f"no file of {target} bytes")


@functools.lru_cache(maxsize=None)
def boundary_lengths():
    """Data of exactly SUB, SUB + 1, 2 SUB - 1 and 2 SUB bytes -> [Case]"""
    out = []
    for k, n in enumerate((SUB, SUB + 1, 2 * SUB - 1, 2 * SUB)):
        data, rep = _with_length(n, 200 + k)
        assert rep["length"] == n
        out.append(case(f"length_{n}", data))
    return out


def _search(want, what, mode="grey", mcu_w=40, rows=1, seeds=range(300, 700), density=2.0):
    for seed in seeds:
        data, rep = make(mode, mcu_w, rows, seed, density)
        if want(rep):
            return data, rep
    raise AssertionError(f"no seed gives {what}")


def _stuffed_at(boundary, seed):
    """A grey file with a stuffed FF in byte boundary - 1 of its data and the 00 in byte `boundary`.  Three blocks of nothing but coefficients of
    255 (eight 1 bits behind a code that begins with nine) lie across the boundary, so nearly every second byte there is an FF; a coefficient of the
    first block is varied until the phase fits."""
    cols = 8
    rng = np.random.default_rng(seed)
    blocks = sparse_blocks(rng, 1, cols * 400, 2.0)
    comps = [dict(id=1, h=1, v=1, tq=0, td=0, ta=0, blocks=blocks.reshape(400, cols, 64))]
    _, reports = JW.write(8 * cols, 8 * 400, comps, QUANT, HUFF)
    starts = reports[0]["blocks"]
    i = max(k for k, b in enumerate(starts) if b <= boundary - 150)
    rows = (i + 3 + cols - 1) // cols + 4
    blocks = blocks[:, :rows * cols].copy()
    blocks[0, i:i + 3, 1:] = 255
    comps[0]["blocks"] = blocks.reshape(rows, cols, 64)
    for t in range(1, 400):
        blocks[0, 0, JW.ZZ[1 + t % 63]] = t
        data, reports = JW.write(8 * cols, 8 * rows, comps, QUANT, HUFF)
        if boundary - 1 in reports[0]["stuffed"] and reports[0]["length"] > boundary + SUB:
            return data
    raise AssertionError(f"no stuffed FF at {boundary - 1}")


@functools.lru_cache(maxsize=None)
def boundary_straddles():
    """A stuffed FF 00 across a sub-sequence boundary both ways (FF | 00 and FF 00 |), a stuffed FF 00 across a group boundary, a value field
    across a sub-sequence boundary, a code across one -> [Case]; each property is asserted from the writer's report."""
    subs = lambda rep: range(SUB, rep["length"] - 1, SUB)                                                                     # noqa: E731
    out = []
    data, _ = _search(lambda r: any(b - 1 in r["stuffed"] for b in subs(r)), "FF | 00 at a sub-sequence boundary")
    out.append(case("stuffed_ff_then_boundary", data))
    data, _ = _search(lambda r: any(b - 2 in r["stuffed"] for b in subs(r)), "FF 00 | at a sub-sequence boundary")
    out.append(case("stuffed_pair_then_boundary", data))
    data, _ = _search(lambda r: any(b in r["stuffed"] for b in subs(r)), "| FF 00 at a sub-sequence boundary")
    out.append(case("boundary_then_stuffed", data))
    data, _ = _search(lambda r: any(k == "value" and a < b <= e for k, a, e in r["fields"] for b in subs(r)), "a value field across a boundary")
    out.append(case("value_across_boundary", data))
    data, _ = _search(lambda r: any(k == "code" and a < b <= e for k, a, e in r["fields"] for b in subs(r)), "a code across a boundary")
    out.append(case("code_across_boundary", data))
    data = _stuffed_at(GROUP_BYTES, 800)
    out.append(case("stuffed_at_group_boundary", data))
    return out


@functools.lru_cache(maxsize=None)
def past_a_scan_tile():
    """The scan works in tiles of 256 sub-sequences with a running carry: a file of more than 2 tiles, made by repeating a packed MCU row."""
    data = repeated_rows("420", 8, 2, 900)
    b, e = ecs_of(data)
    per_row = (e - b) / 2
    rows = int(2.2 * 256 * SUB / per_row) + 1
    data = repeated_rows("420", 8, rows, 900)
    b, e = ecs_of(data)
    assert e - b > 2 * 256 * SUB, e - b
    return case("scan_tiles_420", data)


def damaged_variants(c, seed):
    """c cut at 25 / 50 / 99 % of its entropy-coded bytes and with one byte inverted at five seeded positions -> [Case] (.rgb None)"""
    b, e = ecs_of(c.data)
    out = []
    for pct in (25, 50, 99):
        cut = b + (e - b) * pct // 100
        out.append(Case(f"{c.name}_cut{pct}", c.data[:cut] + b"\xff\xd9", None))
    rng = np.random.default_rng(seed)
    for p in sorted(int(v) for v in rng.integers(b, e, size=5)):
        d = bytearray(c.data)
        d[p] ^= 0xFF
        out.append(Case(f"{c.name}_flip{p - b}", bytes(d), None))
    return out


def write_job(path, cases, lenient, split, order="rgb"):
    """jpeg_cases.write_job with pack_batch's split option -> Batch"""
    batch = jpeg.pack_batch([c.data for c in cases], order, [c.name for c in cases], split=split)
    blob = np.zeros(batch.blob_bytes, dtype=np.uint8)
    batch.fill(blob)
    want = np.zeros(batch.out_bytes, dtype=np.uint8)
    for i, c in enumerate(cases):
        if c.rgb is None:
            continue
        px = c.rgb if order == "rgb" else c.rgb[:, :, ::-1]
        o = int(batch.images[i].out_off)
        want[o:o + px.size] = np.ascontiguousarray(px).reshape(-1)
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", batch.n_images, batch.n_segments, batch.images_off, batch.segments_off, batch.blob_bytes, batch.out_bytes,
                            int(order == "bgr"), 0))
        f.write(blob.tobytes())
        f.write(want.tobytes())
        f.write(np.asarray(lenient, dtype=np.int32).tobytes())
    return batch


def build_host_program(out_dir, sanitize=True, source="jpeg_split_host_main"):
    """tests/<source>.cpp -> a stand-alone program, with AddressSanitizer and UBSan when `sanitize` (jpeg_cases.build_host_program's recipe)."""
    cxx = next((p for p in (shutil.which(c) for c in JC.CXX) if p), None)
    if cxx is None:
        raise RuntimeError(f"no C++ compiler among {', '.join(JC.CXX)}: the host program cannot be built")
    exe = os.path.join(str(out_dir), source)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, os.path.join(HERE, source + ".cpp"), "-o", exe])
    return exe


def run_host_program(exe, job, frames=None):
    """frames: a path tests/jpeg_split_host_main.cpp writes the decoded frames to.  -> (exit status, {image: (verdict, mode)}, everything it
    wrote); verdict "equal" | "differs" | "flagged <status>", mode "split" |
    "serial" | "redone" (None from tests/jpeg_host_main.cpp, which knows no modes)."""
    r = subprocess.run([exe, str(job)] + ([str(frames)] if frames else []), capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    lines = {}
    for line in r.stdout.splitlines():
        parts = line.split()
        if len(parts) >= 2 and parts[0].isdigit():
            mode = parts[-1] if parts[-1] in ("split", "serial", "redone") else None
            lines[int(parts[0])] = (" ".join(parts[1:-1] if mode else parts[1:]), mode)
    return r.returncode, lines, r.stdout + r.stderr
