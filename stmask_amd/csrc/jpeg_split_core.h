/* jpeg_split_core.h -- one entropy-coded segment decoded at several places at once (csrc/jpeg.h, "SPLIT"): the arithmetic of a lane, for the
 * host and for gfx950 alike.  csrc/jpeg_split.hip spreads it over workgroups; tests/jpeg_split_host_main.cpp runs the same functions in plain
 * loops with the kernels' grouping and round count.
 *
 * The decoder of jpeg_core.h's jpeg_decode_block as a machine that can stop and go on anywhere between two symbols.  Its state is
 *     pos, bit   the next unread bit: byte pos of the segment's raw (stuffed) bytes, bit 0..7 of it from the top.  pos never rests on the 00
 *                that follows a stuffed FF;
 *     u          the block within the MCU, 0 .. blocks per MCU - 1, which names the component and so the tables;
 *     k          the zig-zag index of the next coefficient, 0: the block's DC symbol is next.
 * A STEP is one Huffman code and the value bits behind it (at most 16 + 15 bits).  Sub-sequence i owns the steps whose first bit lies in bytes
 * i * STM_JPEG_SUB_BYTES .. + STM_JPEG_SUB_BYTES - 1; jpeg_split_run makes them from a given entry state and returns the exit state, which is
 * the entry state of sub-sequence i + 1.  A state is handed on as one word, its position counted in bits from the start of the sub-sequence it
 * enters (a step is short, so that is a small number).
 *
 * Errors do not stop the machine -- a lane started from a guess meets them by the dozen -- they are reported to the sink with the step, and
 * each has a fixed continuation (no code: 16 bits are dropped; a size out of range: its low 4 bits; an index past 63: the block ends).  Only
 * the write pass, which runs from true states, minds them.  Every step takes at least one bit, so a run is bounded by the sub-sequence's bits. */
#pragma once
#include "jpeg_core.h"

/* What is kept per sub-sequence, in the image's plane region (free until launch 2): 32 bytes. */
struct JpegSplitRec {
    uint32_t e[2];      /* the entry state the exit state was made from, by parity of the sync round */
    uint32_t x[2];      /* the exit state */
    int32_t blocks;     /* blocks that start here; after the scan: blocks that start before */
    int16_t dc[3];      /* sum of their DC differences per component, wrapped; after the scan: the predictions at entry */
    int16_t pad0;
    int32_t redo;       /* record 0 only: the serial kernel decodes the segment */
};
static_assert(sizeof(JpegSplitRec) == 32, "two records per block of plane bytes");

struct JpegSplitState {
    int pos, bit, u, k;
};

/* base: the first byte of the sub-sequence the state enters */
JPEG_HD uint32_t jpeg_split_pack(const JpegSplitState& s, int base)
{
    int rel = (s.pos - base) * 8 + s.bit;
    rel = rel < 0 ? 0 : (rel > 0xFFFF ? 0xFFFF : rel);          /* (never: an exit lies at most a step and its stuffing behind the base) */
    return (uint32_t)rel | ((uint32_t)s.u << 16) | ((uint32_t)s.k << 20);
}
JPEG_HD JpegSplitState jpeg_split_unpack(uint32_t w, int base, int bpm)
{
    JpegSplitState s;
    s.pos = base + (int)((w & 0xFFFFu) >> 3);
    s.bit = (int)(w & 7u);
    s.u = (int)((w >> 16) & 15u);
    if (s.u >= bpm) s.u = 0;
    s.k = (int)((w >> 20) & 63u);
    return s;
}

/* The bit reader of a lane.  Src::get(p) is byte p < nbytes of the segment.  fill() gathers the 5 data bytes from (pos, bit) on -- FF 00 is one
 * byte, an FF followed by anything else (or by the end) is a marker, and from a marker or the end on the bytes are zero -- which is room for one
 * step; commit() moves (pos, bit) behind what the step took.  `end` is the first byte that is no data, as far as this reader has met it. */
template <class Src>
struct JpegSplitBits {
    Src& src;
    int nbytes, end, pos, bit, used;
    uint32_t stuffed;       /* bit i: byte i of the window was an FF with its 00 behind it */
    uint64_t win;

    JPEG_HD JpegSplitBits(Src& s, int n, int p, int b) : src(s), nbytes(n), end(n), pos(p), bit(b), used(b), stuffed(0), win(0) {}
    JPEG_HD void fill()
    {
        win = 0;
        stuffed = 0;
        used = bit;
        int p = pos;
        for (int i = 0; i < 5; ++i) {
            int b = 0;
            if (p < end) {
                b = src.get(p);
                if (b == 0xFF) {
                    const int b2 = p + 1 < nbytes ? src.get(p + 1) : 0xD9;
                    if (b2 == 0) {
                        ++p;
                        stuffed |= 1u << i;
                    } else {
                        end = p;
                        b = 0;
                    }
                }
            }
            ++p;
            win = (win << 8) | (uint64_t)(unsigned)b;
        }
    }
    JPEG_HD unsigned peek16() const { return (unsigned)(win >> (24 - used)) & 0xFFFFu; }       /* used <= 7 here */
    JPEG_HD void skip(int n) { used += n; }
    JPEG_HD int get(int n) /* 0 <= n <= 15; used stays <= 7 + 16 + 15 */
    {
        used += n;
        return (int)((unsigned)(win >> (40 - used)) & ((1u << n) - 1u));
    }
    JPEG_HD void commit()
    {
        const int nb = used >> 3;
        pos += nb + __builtin_popcount(stuffed & ((1u << nb) - 1u));
        bit = used & 7;
    }
    /* the step just committed took bits the segment does not have */
    JPEG_HD bool over() const { return pos > end || (pos == end && bit > 0); }
};

/* the state a lane guesses for sub-sequence sub >= 1: a block starts at its first byte (behind the 00 of a stuffed FF that straddles it) */
template <class Src>
JPEG_HD uint32_t jpeg_split_guess(Src& src, int nbytes, int sub)
{
    const int base = sub * STM_JPEG_SUB_BYTES;
    JpegSplitState s = {base, 0, 0, 0};
    if (sub > 0 && base < nbytes && src.get(base - 1) == 0xFF && src.get(base) == 0) s.pos = base + 1;
    return jpeg_split_pack(s, base);
}

/* the table choice of an image in one word (a lane keeps no indexed copy of the descriptor): bit c DC table, bit 4 + c AC table of component c */
JPEG_HD int jpeg_split_tables(const stm_jpeg_image& im)
{
    return (im.td[0] & 1) | ((im.td[1] & 1) << 1) | ((im.td[2] & 1) << 2) | ((im.ta[0] & 1) << 4) | ((im.ta[1] & 1) << 5) | ((im.ta[2] & 1) << 6);
}

/* The steps sub-sequence `sub` owns, from `entry` -> its exit state.  huff: the image's four tables (DC 0, DC 1, AC 0, AC 1); n0: blocks of
 * component 0 in an MCU, bpm: of all components; tsel: jpeg_split_tables.  The sink is told every step:
 *     dc(c, u, diff, err, over)    a block of component c, block u of its MCU, starts with this DC difference
 *     ac(k, value, err, over)      coefficient k (zig-zag) of the current block, k < 0: a step without a coefficient (end of block, ZRL, an error)
 * err: 0 or STM_JPEG_E*; over: the step took bits beyond the data. */
template <class Src, class Sink>
JPEG_HD uint32_t jpeg_split_run(Src& src, int nbytes, const stm_jpeg_huff* huff, int n0, int bpm, int tsel, int sub, uint32_t entry, Sink& sink)
{
    const int base = sub * STM_JPEG_SUB_BYTES, sub_end = base + STM_JPEG_SUB_BYTES;
    const JpegSplitState st = jpeg_split_unpack(entry, base, bpm);
    JpegSplitBits<Src> br(src, nbytes, st.pos, st.bit);
    int u = st.u, k = st.k;
    for (int n = 0; n < 8 * STM_JPEG_SUB_BYTES + 64 && br.pos < sub_end; ++n) {
        const int c = u < n0 ? 0 : 1 + u - n0;
        int err = 0;
        br.fill();
        if (k == 0) {
            const JpegHuffRef t{huff + ((tsel >> c) & 1)};
            int s = jpeg_symbol(br, t);
            if (s < 0) {
                err = STM_JPEG_ENOCODE;
                br.skip(16);
                s = 0;
            } else if (s > 11) {
                err = STM_JPEG_ESIZE;
                s &= 15;
            }
            const int diff = jpeg_extend(br.get(s), s);
            br.commit();
            sink.dc(c, u, diff, err, br.over());
            k = 1;
        } else {
            const JpegHuffRef t{huff + 2 + ((tsel >> (4 + c)) & 1)};
            const int rs = jpeg_symbol(br, t);
            int at = -1, v = 0;
            if (rs < 0) {
                err = STM_JPEG_ENOCODE;
                br.skip(16);
            } else {
                const int r = rs >> 4, s = rs & 15;
                if (s == 0) {
                    k = r == 15 ? k + 16 : 64;      /* ZRL, end of block */
                } else {
                    if (s > 10) err = STM_JPEG_ESIZE;
                    k += r;
                    v = jpeg_extend(br.get(s), s);
                    if (k > 63) err = STM_JPEG_EINDEX;
                    else at = k;
                    ++k;
                }
            }
            br.commit();
            sink.ac(at, v, err, br.over());
        }
        if (k >= 64) {
            k = 0;
            u = u + 1 == bpm ? 0 : u + 1;
        }
    }
    const JpegSplitState out = {br.pos, br.bit, u, k};
    return jpeg_split_pack(out, sub_end);
}

/* jpeg_natural without a table to index: a lane of the write pass has its own k, and an indexed local array would live in scratch memory */
JPEG_HD int jpeg_split_natural(int k)
{
    const int r = (k >> 3) & 7;
    const uint64_t w = r == 0 ? 0x0A03020910080100ull : r == 1 ? 0x05040B1219201811ull : r == 2 ? 0x22293028211A130Cull : r == 3 ? 0x1C150E07060D141Bull :
                       r == 4 ? 0x242B323938312A23ull : r == 5 ? 0x332C251E170F161Dull : r == 6 ? 0x2E271F262D343B3Aull : 0x3F3E372F363D3C35ull;
    return (int)(w >> (8 * (k & 7))) & 63;
}

/* the sinks of the three kinds of pass: the sync rounds want the exit state alone, ... */
struct JpegSplitNull {
    JPEG_HD void dc(int, int, int, int, bool) {}
    JPEG_HD void ac(int, int, int, bool) {}
};

/* ... the last round counts what starts in the sub-sequence, ... */
struct JpegSplitCount {
    int blocks, d0, d1, d2;
    JPEG_HD void dc(int c, int, int diff, int, bool)
    {
        ++blocks;
        d0 += c == 0 ? diff : 0;
        d1 += c == 1 ? diff : 0;
        d2 += c == 2 ? diff : 0;
    }
    JPEG_HD void ac(int, int, int, bool) {}
};

/* ... and the write pass stores coefficients: coef is the batch's coefficient area, already zero for this image; seq: the blocks of the segment
 * that start before the next DC symbol; preds: the predictions; expected: the blocks of the segment.  A block is addressed as the serial
 * kernel addresses it, MCU order to raster order per component.  bad: something the serial kernel would flag (or, from a state that is not the
 * true one, nonsense) happened in a block below `expected`. */
struct JpegSplitWrite {
    int16_t* coef;
    int64_t first;          /* the image's blk_first */
    int hs, vs, mcu_w, mcu_h, mcu_first, n0, bpm;
    int expected, seq;
    uint64_t preds;         /* the predictions, 16 bits each, component c at bit 16 c (one word, shifted: three fields chosen by c become an indexed
                             * load of the struct, which puts it into scratch memory) */
    int64_t at;             /* first coefficient of the current block, -1: none to store */
    bool live;              /* the current block is below `expected` */
    int bad;

    JPEG_HD void open(int cur, int u)       /* block cur of the segment, which must be block u of its MCU */
    {
        at = -1;
        live = cur >= 0 && cur < expected;
        if (!live) return;
        if (cur % bpm != u) {
            bad = 1;
            return;
        }
        const int mcu = mcu_first + cur / bpm, my = mcu / mcu_w, mx = mcu - my * mcu_w;
        const int c = u < n0 ? 0 : 1 + u - n0;
        const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
        const int by = c == 0 ? u / hs : 0, bx = c == 0 ? u - by * hs : 0;
        const int64_t comp_first = c == 0 ? 0 : (int64_t)mcu_w * mcu_h * (hs * vs + (c - 1));
        at = (first + comp_first + (int64_t)(my * cv + by) * (mcu_w * ch) + (mx * ch + bx)) * 64;
    }
    JPEG_HD void dc(int c, int u, int diff, int err, bool over)
    {
        open(seq++, u);
        const int sh = 16 * c;
        const int p = (int16_t)((int16_t)(preds >> sh) + diff);
        preds = (preds & ~((uint64_t)0xFFFFu << sh)) | ((uint64_t)(uint16_t)p << sh);
        if (!live) return;
        if (err || over) bad = 1;
        if (at >= 0) coef[at] = (int16_t)p;
    }
    JPEG_HD void ac(int k, int v, int err, bool over)
    {
        if (!live) return;
        if (err || over) bad = 1;
        if (at >= 0 && k >= 0) coef[at + jpeg_split_natural(k)] = (int16_t)v;
    }
};
