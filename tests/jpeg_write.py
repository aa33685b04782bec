"""A baseline JPEG writer for the tests, in Python and numpy: what PIL's encoder cannot be made to write.  write() takes quantised coefficient
blocks and every selector as given -- it checks nothing a decoder should check -- and writes SOF0 and ONE interleaved scan with byte stuffing
and 1-padding, under a layout description that decides the markers around it.  It reports where, within each restart segment, every stuffed
FF, every block and every Huffman code and value field lies, so that a fixture can be shown to put one across a given offset.

Beside it: split() / join() and the header rewrites of an existing file (tests/golden/gen_jpeg_edge_cases.py applies them to PIL's files).

    component = dict(id=1, h=2, v=2, tq=0, td=0, ta=0, blocks=int array [block rows, block columns, 64], natural order)
    layout    = dict(app="jfif" | "adobe" | None, merged=False, first={"quant": {...}, "huff": {...}}, fill={marker or "rst": count},
                     extra=[(marker, payload)], trailer=b"", dri_segment=None)
"""
import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29,
      22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
JFIF = b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
ADOBE_YCC = b"Adobe\0\x64\0\0\0\0\x01"


def codes_of(counts, values):
    """(counts of codes per length 1..16, symbols in code order) -> {symbol: (code, length)}, the canonical assignment."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return out


def block_fields(block, pred, dc, ac):
    """One block (64 coefficients, natural order) -> [(kind, value, bits)], kind "code" or "value"; dc, ac: codes_of() tables."""
    diff = int(block[0]) - pred
    s = abs(diff).bit_length()
    out = [("code",) + dc[s]]
    if s:
        out.append(("value", diff if diff >= 0 else diff + (1 << s) - 1, s))
    run = 0
    for k in range(1, 64):
        v = int(block[ZZ[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(("code",) + ac[0xF0])
            run -= 16
        s = abs(v).bit_length()
        out.append(("code",) + ac[(run << 4) | s])
        out.append(("value", v if v >= 0 else v + (1 << s) - 1, s))
        run = 0
    if run:
        out.append(("code",) + ac[0x00])
    return out


def pack_segment(blocks_fields):
    """The fields of a restart segment's blocks -> (stuffed bytes, report).  report: length; stuffed: the offset of every stuffed FF (its 00
    follows); blocks: the offset of the byte each block starts in; fields: (kind, offset of its first byte, of its last byte).  Offsets count
    the stuffed bytes, as a reader of the file meets them."""
    bits, spans, starts = [], [], []
    n = 0
    for fields in blocks_fields:
        starts.append(n)
        for kind, value, width in fields:
            bits.append(format(value, f"0{width}b"))
            spans.append((kind, n, n + width - 1))
            n += width
    bits = "".join(bits)
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    a = np.frombuffer(raw, dtype=np.uint8)
    is_ff = a == 0xFF
    at = np.arange(a.size) + np.concatenate([[0], np.cumsum(is_ff)[:-1]]).astype(np.int64) if a.size else np.zeros(0, dtype=np.int64)
    data = raw.replace(b"\xff", b"\xff\x00")
    report = dict(length=len(data), stuffed=at[is_ff].tolist(), blocks=[int(at[s >> 3]) for s in starts],
                  fields=[(kind, int(at[b >> 3]), int(at[e >> 3])) for kind, b, e in spans])
    return data, report


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _dqt(slot, table):
    return bytes([slot]) + bytes(int(table[z]) for z in ZZ)


def _dht(key, table):
    counts, values = table
    return bytes([(key[0] << 4) | key[1]]) + bytes(counts) + bytes(values)


def write(width, height, components, quant, huff, dri=0, layout=None):
    """-> (the file's bytes, [report of every restart segment]).  quant: {slot: 64 values, natural order}; huff: {(class, id): (counts,
    values)}, class 0 DC and 1 AC; dri: MCUs per restart interval, 0 for none.  One component is written as libjpeg reads it: its sampling
    factors stand in the frame header and an MCU is one block."""
    lay = dict(app="jfif", merged=False, first=None, fill={}, extra=[], trailer=b"", dri_segment=None)
    lay.update(layout or {})
    fill = lambda m: b"\xff" * lay["fill"].get(m, 0)                                    # noqa: E731
    out = [b"\xff\xd8"]
    if lay["app"] == "jfif":
        out.append(fill(0xE0) + _segment(0xE0, JFIF))
    elif lay["app"] == "adobe":
        out.append(fill(0xEE) + _segment(0xEE, ADOBE_YCC))
    for marker, payload in lay["extra"]:
        out.append(fill(marker) + _segment(marker, payload))
    sets = ([lay["first"]] if lay["first"] else []) + [dict(quant=quant, huff=huff)]    # a table defined twice: the last one wins
    for tables in sets:
        q = tables.get("quant", {})
        if lay["merged"] and q:
            out.append(fill(0xDB) + _segment(0xDB, b"".join(_dqt(s, q[s]) for s in sorted(q))))
        else:
            out.extend(fill(0xDB) + _segment(0xDB, _dqt(s, q[s])) for s in sorted(q))
    out.append(fill(0xC0) + _segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(components)]) +
                                     b"".join(bytes([c["id"], (c["h"] << 4) | c["v"], c["tq"]]) for c in components)))
    for tables in sets:
        h = tables.get("huff", {})
        if lay["merged"] and h:
            out.append(fill(0xC4) + _segment(0xC4, b"".join(_dht(k, h[k]) for k in sorted(h))))
        else:
            out.extend(fill(0xC4) + _segment(0xC4, _dht(k, h[k])) for k in sorted(h))
    if dri or lay["dri_segment"] is not None:
        out.append(fill(0xDD) + _segment(0xDD, int(lay["dri_segment"] if lay["dri_segment"] is not None else dri).to_bytes(2, "big")))
    out.append(fill(0xDA) + _segment(0xDA, bytes([len(components)]) + b"".join(bytes([c["id"], (c["td"] << 4) | c["ta"]]) for c in components) +
                                     b"\x00\x3f\x00"))
    if len(components) == 1:
        geometry = [(1, 1)]
        mcu_w, mcu_h = -(-width // 8), -(-height // 8)
    else:
        geometry = [(c["h"], c["v"]) for c in components]
        hm, vm = max(g[0] for g in geometry), max(g[1] for g in geometry)
        mcu_w, mcu_h = -(-width // (8 * hm)), -(-height // (8 * vm))
    codes = [(codes_of(*huff[(0, c["td"])]), codes_of(*huff[(1, c["ta"])])) for c in components]
    for c, (h, v) in zip(components, geometry):
        assert np.asarray(c["blocks"]).shape == (mcu_h * v, mcu_w * h, 64), (np.asarray(c["blocks"]).shape, (mcu_h * v, mcu_w * h, 64))
    reports, current, pred = [], [], [0] * len(components)
    n_mcu = mcu_w * mcu_h
    for m in range(n_mcu):
        if dri and m and m % dri == 0:
            data, report = pack_segment(current)
            out.append(data + fill("rst") + bytes([0xFF, 0xD0 + (m // dri - 1) % 8]))
            reports.append(report)
            current, pred = [], [0] * len(components)
        my, mx = divmod(m, mcu_w)
        for ci, (c, (h, v)) in enumerate(zip(components, geometry)):
            for by in range(v):
                for bx in range(h):
                    block = c["blocks"][my * v + by][mx * h + bx]
                    current.append(block_fields(block, pred[ci], *codes[ci]))
                    pred[ci] = int(block[0])
    data, report = pack_segment(current)
    reports.append(report)
    out.append(data + fill(0xD9) + b"\xff\xd9" + lay["trailer"])
    return b"".join(out), reports


def quantise(plane, table):
    """Samples [8 r, 8 c] (0..255) -> quantised coefficient blocks int [r, c, 64], natural order: a floating-point DCT, rounded."""
    plane = np.asarray(plane, dtype=np.float64) - 128
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(0.125), 0.5)[:, None]
    tiles = plane.reshape(r, 8, c, 8).transpose(0, 2, 1, 3)
    coef = basis @ tiles @ basis.T
    return np.rint(coef.reshape(r, c, 64) / np.asarray(table, dtype=np.float64)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- rewrites of an existing file
def split(data):
    """A file -> ([[marker, payload]] of its segments up to and including the scan header, everything behind that header)."""
    segs, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        segs.append([m, data[i + 4:i + 2 + n]])
        i += 2 + n
        if m == 0xDA:
            return segs, data[i:]


def join(segs, tail, fill=None):
    """... and back.  fill: {index of a segment: FF bytes in front of its marker}."""
    fill = fill or {}
    return b"\xff\xd8" + b"".join(b"\xff" * fill.get(i, 0) + _segment(m, p) for i, (m, p) in enumerate(segs)) + tail


def patched(data, marker, offset, value, nth=0):
    """data with byte `offset` of the payload of its nth `marker` segment set to value"""
    segs, tail = split(data)
    seg = [s for s in segs if s[0] == marker][nth]
    seg[1] = seg[1][:offset] + bytes([value]) + seg[1][offset + 1:]
    return join(segs, tail)


def with_segments(data, new, before=0xDB):
    """data with the (marker, payload) segments `new` in front of its first `before` segment"""
    segs, tail = split(data)
    i = [s[0] for s in segs].index(before)
    return join(segs[:i] + [list(s) for s in new] + segs[i:], tail)


def without(data, marker):
    segs, tail = split(data)
    return join([s for s in segs if s[0] != marker], tail)


def with_component_ids(data, ids):
    segs, tail = split(data)
    for s in segs:
        if s[0] == 0xC0:
            p = bytearray(s[1])
            for c, v in enumerate(ids):
                p[6 + 3 * c] = v
            s[1] = bytes(p)
        elif s[0] == 0xDA:
            p = bytearray(s[1])
            for c, v in enumerate(ids):
                p[1 + 2 * c] = v
            s[1] = bytes(p)
    return join(segs, tail)


def with_huffman_ids_swapped(data):
    """Every Huffman table takes the other id of its class, and the scan header's selectors follow."""
    segs, tail = split(data)
    for s in segs:
        if s[0] == 0xC4:
            p, j = bytearray(s[1]), 0
            while j < len(p):
                p[j] ^= 1
                j += 17 + sum(p[j + 1:j + 17])
            s[1] = bytes(p)
        elif s[0] == 0xDA:
            p = bytearray(s[1])
            for c in range(p[0]):
                p[2 + 2 * c] ^= 0x11
            s[1] = bytes(p)
    return join(segs, tail)


def with_quant_slots(data, slots):
    """Quantisation table t moves to slot slots[t]; the frame header follows."""
    segs, tail = split(data)
    for s in segs:
        if s[0] == 0xDB:
            p = bytearray(s[1])
            for j in range(0, len(p), 65):
                p[j] = slots[p[j]]
            s[1] = bytes(p)
        elif s[0] == 0xC0:
            p = bytearray(s[1])
            for c in range(p[5]):
                p[8 + 3 * c] = slots[p[8 + 3 * c]]
            s[1] = bytes(p)
    return join(segs, tail)


def with_tables_merged(data):
    """All quantisation tables in one DQT segment, all Huffman tables in one DHT segment, where the first of each stood."""
    segs, tail = split(data)
    for m in (0xDB, 0xC4):
        first = [s[0] for s in segs].index(m)
        segs[first] = [m, b"".join(s[1] for s in segs if s[0] == m)]
        segs = [s for i, s in enumerate(segs) if s[0] != m or i == first]
    return join(segs, tail)


def with_fill(data, header=0, restart=0, end=0):
    """FF fill bytes in front of every header marker, every restart marker and the end-of-image marker."""
    segs, tail = split(data)
    assert tail.endswith(b"\xff\xd9")
    body = bytearray()
    i = 0
    while i < len(tail) - 2:
        if tail[i] == 0xFF and 0xD0 <= tail[i + 1] <= 0xD7:
            body += b"\xff" * restart
        body += tail[i:i + 2] if tail[i] == 0xFF else tail[i:i + 1]
        i += 2 if tail[i] == 0xFF else 1
    return join(segs, bytes(body) + b"\xff" * end + b"\xff\xd9", {i: header for i in range(len(segs))})
