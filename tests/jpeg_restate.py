"""A restatement of baseline JPEG decoding as libjpeg does it with its default settings (JDCT_ISLOW, fancy upsampling), in Python integers and
numpy, independent of stmask_amd.jpeg: its own marker walk, a bit-at-a-time Huffman decoder, the `islow` IDCT, h2v1 / h2v2 fancy upsampling and
the fixed-point YCbCr conversion.  decode(data) -> uint8 [H, W, 3] RGB, equal to PIL's decode bit for bit (tests/test_jpeg_cpu.py holds it to
every fixture of tests/golden/jpeg_cases.npz and, where PIL imports, to a live decode).  decode(data, stats) also counts what the fixtures must
contain (tests/golden/gen_jpeg_cases.py asserts the counts of STAT_KEYS, tests/golden/gen_jpeg_edge_cases.py those of EDGE_STAT_KEYS).  Chroma planes
of one or two columns are replicated, as jdsample.c does; fill bytes (FF) in front of any marker are passed over."""
import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29,
      22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
STAT_KEYS = ("stuffed", "zrl", "last_at_63", "long_code", "clamp_0", "clamp_255", "restart_splits_row", "chroma_one_column")
# what the edge fixtures (tests/golden/jpeg_edge_cases.npz) must hold beyond that.  Offsets are byte offsets within a restart segment, stuffed
# bytes included: what the kernel's 64-byte groups and 1 KiB staging window see.
EDGE_STAT_KEYS = ("chroma_replicated", "dc_size_11", "ac_size_10_at_63", "dense_block", "dc_code_10", "dc_code_11", "dc_code_12", "dc_code_13", "dc_code_14",
                  "dc_code_15", "dc_code_16", "ac_code_10", "ac_code_11", "ac_code_12", "ac_code_13", "ac_code_14", "ac_code_15", "ac_code_16", "quant_255",
                  "tables_crossed", "luma_on_table_1", "header_fill", "restart_fill", "end_fill", "restart_wraps", "stuffed_at_63", "stuffed_at_1023",
                  "stuffed_at_2047", "stuffed_ends_segment", "code_straddles_1024", "value_straddles_1024", "segments_over_19", "dimension_over_160")


def parse(d, stats=None):
    i, q, ht, dri = 2, {}, {}, 0
    fill = 0
    while True:
        assert d[i] == 0xFF
        while d[i + 1] == 0xFF:                             # fill bytes: any number of FF may stand in front of a marker
            i += 1
            fill += 1
        m, L = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        s = d[i + 4:i + 2 + L]
        if m == 0xDB:
            j = 0
            while j < len(s):
                assert s[j] >> 4 == 0
                tab = np.zeros(64, dtype=np.int64)
                tab[ZZ] = list(s[j + 1:j + 65])
                q[s[j] & 15] = tab
                j += 65
        elif m == 0xC0:
            H, W = (s[1] << 8) | s[2], (s[3] << 8) | s[4]
            comps = [(s[6 + 3 * k], s[7 + 3 * k] >> 4, s[7 + 3 * k] & 15, s[8 + 3 * k]) for k in range(s[5])]
        elif m == 0xC4:
            j = 0
            while j < len(s):
                tc, cnt = s[j], list(s[j + 1:j + 17])
                n = sum(cnt)
                vals = list(s[j + 17:j + 17 + n])
                j += 17 + n
                codes, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(cnt[length - 1]):
                        codes[(length, code)] = vals[k]
                        k += 1
                        code += 1
                    code <<= 1
                ht[tc] = codes
        elif m == 0xDD:
            dri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            sel = {s[1 + 2 * k]: (s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(s[0])}
            if stats is not None:
                stats["header_fill"] += fill
            return H, W, comps, q, ht, dri, sel, d[i + 2 + L:]
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
        i += 2 + L


class Bits:
    def __init__(self, d, stats):
        self.d, self.p, self.b, self.n, self.stats = d, 0, 0, 0, stats
        self.s0, self.at, self.kind = 0, 0, "dc"            # where the segment starts, the offset in it of the byte the last bit came from

    def bit(self):
        if self.n == 0:
            c = self.d[self.p]
            self.at = self.p - self.s0
            self.p += 1
            if c == 0xFF:
                assert self.d[self.p] == 0
                self.p += 1
                self.stats["stuffed"] += 1
                for at in (63, 1023, 2047):
                    if self.at == at:
                        self.stats[f"stuffed_at_{at}"] += 1
            self.b, self.n = c, 8
        self.n -= 1
        return (self.b >> self.n) & 1

    def get(self, k):
        v, first = 0, None
        for _ in range(k):
            v = (v << 1) | self.bit()
            first = self.at if first is None else first
        if k and first < 1024 <= self.at:
            self.stats["value_straddles_1024"] += 1
        return v

    def sym(self, t):
        c, first = 0, None
        for length in range(1, 17):
            c = (c << 1) | self.bit()
            first = self.at if first is None else first
            if (length, c) in t:
                if length > 9:
                    self.stats["long_code"] += 1
                    self.stats[f"{self.kind}_code_{length}"] += 1
                if first < 1024 <= self.at:
                    self.stats["code_straddles_1024"] += 1
                return t[(length, c)]
        raise ValueError("no Huffman code within 16 bits")

    def marker(self):
        """The marker that follows the bits read so far, behind any fill bytes -> its code.  The rest of the current byte is padding."""
        if self.p >= 2 and self.d[self.p - 2:self.p] == b"\xff\x00":
            self.stats["stuffed_ends_segment"] += 1
        self.n = 0
        assert self.d[self.p] == 0xFF
        fill = 0
        while self.d[self.p + 1] == 0xFF:
            self.p += 1
            fill += 1
        self.p += 2
        return self.d[self.p - 1], fill

    def restart(self, number):
        m, fill = self.marker()
        assert m == 0xD0 + number % 8
        self.stats["restart_fill"] += fill
        self.s0 = self.p


def ext(v, k):
    return v if k == 0 or v >= (1 << (k - 1)) else v - (1 << k) + 1


def _pass(i, sh):
    """One 8-point pass of jidctint.c over the leading axis of i (int64 [8, ...])."""
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 + z3 * -15137, z1 + z2 * 6270
    z2, z3 = i[0], i[4]
    t0, t1 = (z2 + z3) << 13, (z2 - z3) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3])
    return (o + (1 << (sh - 1))) >> sh


def idct_raw(blocks):
    """Dequantised coefficients int64 [n, 8, 8] -> sample - 128 [n, 8, 8], before libjpeg's range limit."""
    ws = _pass(blocks.transpose(1, 2, 0), 11)               # over rows r of [r, c, n]: the column pass
    out = _pass(ws.transpose(1, 0, 2), 18)                  # over columns c of [c, r, n]: the row pass -> [c, r, n]
    return out.transpose(2, 1, 0)


def idct(blocks):
    """Dequantised coefficients int64 [n, 8, 8] -> samples [n, 8, 8] in 0..255."""
    return np.clip(idct_raw(blocks) + 128, 0, 255)


def decode(d, stats=None):
    """-> uint8 [H, W, 3].  stats (a dict) receives the counts of STAT_KEYS and EDGE_STAT_KEYS, summed over calls, and "excursion": the largest
    |sample - 128| behind the IDCT of any call.  libjpeg's range-limit table clamps exactly only below 384 there; beyond it its C and SIMD
    transforms disagree with each other, so PIL's pixels are no oracle for such a file."""
    stats = stats if stats is not None else {}
    for k in STAT_KEYS + EDGE_STAT_KEYS + ("excursion",):
        stats.setdefault(k, 0)
    d = bytes(d)
    H, W, comps, q, ht, dri, sel, ecs = parse(d, stats)
    stats["dimension_over_160"] += int(max(H, W) > 160)
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    mw, mh = -(-W // (8 * hm)), -(-H // (8 * vm))
    if dri and dri % mw and dri < mw * mh:
        stats["restart_splits_row"] += 1
    n_seg = -(-mw * mh // dri) if dri else 1
    stats["segments_over_19"] += int(n_seg > 19)
    stats["restart_wraps"] += (n_seg - 1) // 8
    stats["quant_255"] += int(any((q[c[3]] == 255).any() for c in comps))
    if len(comps) == 3:
        y, cb, cr = [(c[3],) + sel[c[0]] for c in comps]
        stats["tables_crossed"] += int(len({y, cb, cr}) == 3 and cr[1] != cr[2])
        stats["luma_on_table_1"] += int(y[1:] == (1, 1) and cb[1:] == (0, 0))
    coefs = [np.zeros((mh * c[2], mw * c[1], 64), dtype=np.int64) for c in comps]
    br, pred = Bits(ecs, stats), [0] * len(comps)
    for m in range(mw * mh):
        if dri and m and m % dri == 0:
            br.restart(m // dri - 1)
            pred = [0] * len(comps)
        my, mx = divmod(m, mw)
        for ci, (cid, h, v, tq) in enumerate(comps):
            dc, ac = sel[cid]
            for by in range(v):
                for bx in range(h):
                    co = coefs[ci][my * v + by, mx * h + bx]
                    br.kind = "dc"
                    s = br.sym(ht[dc])
                    stats["dc_size_11"] += int(s == 11)
                    pred[ci] += ext(br.get(s), s)
                    co[0] = pred[ci]
                    br.kind = "ac"
                    k, n = 1, 0
                    while k < 64:
                        rs = br.sym(ht[0x10 | ac])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r == 15:
                                stats["zrl"] += 1
                                k += 16
                                continue
                            break
                        k += r
                        co[ZZ[k]] = ext(br.get(s), s)
                        n += 1
                        if k == 63:
                            stats["last_at_63"] += 1
                            stats["ac_size_10_at_63"] += int(s == 10)
                        k += 1
                    stats["dense_block"] += int(n == 63)
    m, fill = br.marker()
    assert m == 0xD9, "the end-of-image marker follows the last MCU"
    stats["end_fill"] += fill
    full = []
    for ci, (cid, h, v, tq) in enumerate(comps):
        bh, bw = coefs[ci].shape[:2]
        raw = idct_raw((coefs[ci] * q[tq]).reshape(bh * bw, 8, 8))
        stats["excursion"] = max(stats["excursion"], int(np.abs(raw).max()))
        px = np.clip(raw + 128, 0, 255).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        dw, dh = -(-W * h // hm), -(-H * v // vm)
        p = px[:dh, :dw]
        if h == hm and v == vm:
            full.append(p[:H, :W])
            continue
        if dw == 1:
            stats["chroma_one_column"] += 1
        if dw <= 2:                                         # jdsample.c: fancy upsampling only when downsampled_width > 2; else replication
            stats["chroma_replicated"] += int(dw == 2 if v == vm else dh > 1)        # where interpolating would give other samples
            out = np.repeat(p, 2, axis=1) if v == vm else np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
        elif v == vm:                                       # h2v1
            out = np.zeros((dh, 2 * dw), dtype=np.int64)
            for x in range(dw):
                out[:, 2 * x] = p[:, x] if x == 0 else (3 * p[:, x] + p[:, x - 1] + 1) >> 2
                out[:, 2 * x + 1] = p[:, x] if x == dw - 1 else (3 * p[:, x] + p[:, x + 1] + 2) >> 2
        else:                                               # h2v2
            t0, t1 = 3 * p + p[[0] + list(range(dh - 1))], 3 * p + p[list(range(1, dh)) + [dh - 1]]      # upper and lower output rows
            out = np.zeros((2 * dh, 2 * dw), dtype=np.int64)
            for vv, t in ((0, t0), (1, t1)):
                for x in range(dw):
                    out[vv::2, 2 * x] = (4 * t[:, x] + 8) >> 4 if x == 0 else (3 * t[:, x] + t[:, x - 1] + 8) >> 4
                    out[vv::2, 2 * x + 1] = (4 * t[:, x] + 7) >> 4 if x == dw - 1 else (3 * t[:, x] + t[:, x + 1] + 7) >> 4
        full.append(out[:H, :W])
    if len(full) == 1:
        return np.stack([full[0]] * 3, -1).astype(np.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    stats["clamp_0"] += int((rgb < 0).sum())
    stats["clamp_255"] += int((rgb > 255).sum())
    return np.clip(rgb, 0, 255).astype(np.uint8)
