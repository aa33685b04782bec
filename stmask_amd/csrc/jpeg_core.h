/* jpeg_core.h -- the arithmetic of the JPEG decoder (csrc/jpeg.h), per symbol, per block and per pixel, as functions that compile for the host
 * and for gfx950 alike.  csrc/jpeg_decode.hip's kernels call them; a stand-alone host program (tests/jpeg_host_main.cpp) runs the very same
 * code on the CPU, where a sanitizer can watch it.
 *
 * The result is libjpeg's for its default settings (JDCT_ISLOW, fancy upsampling), bit for bit:
 *   - Huffman decode: a first-level lookup of STM_JPEG_LOOK_BITS bits, then the canonical maxcode / valoff walk up to 16 bits;
 *   - `islow` IDCT: CONST_BITS = 13, PASS1_BITS = 2, the column pass descaled by 11 and the row pass by 18, both round-half-up;
 *   - h2v1: edge samples copied, elsewhere (3 c + prev + 1) >> 2 and (3 c + next + 2) >> 2;
 *   - h2v2: column sums t = 3 cur + neighbour row (the row above for the upper output row, the row below for the lower, both replicated at the
 *     first and last real chroma row), then (3 t + last + 8) >> 4 and (3 t + next + 7) >> 4, the edges (4 t + 8) >> 4 and (4 t + 7) >> 4;
 *   - a chroma plane of one or two real columns (dw <= 2) is not interpolated at all: libjpeg (jdsample.c) chooses fancy upsampling only when
 *     downsampled_width > 2 and replicates the sample otherwise, row[xo >> 1] for h2v1 and p[yo >> 1][xo >> 1] for h2v2 (vertically too);
 *   - YCbCr: R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16).
 * The transform's sums are formed in uint32_t, whose wrap-around is defined: coefficients no encoder writes (a damaged file) cannot overflow a
 * signed integer, and the values of a sound file are the same in either arithmetic.  Right shifts of negative values are arithmetic. */
#pragma once
#include <stdint.h>

#include "jpeg.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif
/* The entropy decoder's state is the same in every lane of its wavefront.  The compiler cannot see that of a value read from LDS, so it is told:
 * what follows is then known to be the same in every lane, and a branch on it is a branch of the whole wave, not a lane mask. */
#if defined(__HIP_DEVICE_COMPILE__)
#define JPEG_UNIFORM(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define JPEG_UNIFORM(x) ((int)(x))
#endif

/* zig-zag position k -> natural (row-major) index.  (A lane of the entropy kernel wants the position of ITS index and searches for it once.) */
JPEG_HD int jpeg_natural(int k)
{
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

/* ---- launch 1: entropy decode ------------------------------------------------------------------------------------------------------------ */

/* The bit reader of one segment.  Src::get(pos) is byte pos < nbytes of the segment.  FF 00 is un-stuffed at refill; an FF followed by anything
 * else (or by the end) is a marker: nothing from there on is data.  Past the data the reader feeds zero bits and counts them, so overrun() tells
 * whether a decoded value used bits the segment does not have. */
template <class Src>
struct JpegBits {
    Src& src;
    int nbytes;
    int pos;
    int nbits;       /* valid bits at the low end of acc */
    int fake;        /* how many of them (the lowest) are padding; saturates */
    uint64_t acc;

    JPEG_HD JpegBits(Src& s, int n) : src(s), nbytes(n), pos(0), nbits(0), fake(0), acc(0) {}

    JPEG_HD void fill() /* -> at least 57 bits; at most 8 bytes per call */
    {
        while (nbits <= 56) {
            int b = 0;
            bool data = false;
            if (pos < nbytes) {
                b = src.get(pos++);
                data = true;
                if (b == 0xFF) {
                    const int b2 = pos < nbytes ? src.get(pos) : 0xD9;
                    if (b2 == 0) {
                        ++pos;
                    } else {
                        pos = nbytes;
                        b = 0;
                        data = false;
                    }
                }
            }
            if (!data && fake < (1 << 20)) fake += 8;
            acc = (acc << 8) | (uint64_t)(unsigned)b;
            nbits += 8;
        }
    }
    JPEG_HD unsigned peek16() const { return (unsigned)(acc >> (nbits - 16)) & 0xFFFFu; }
    JPEG_HD void skip(int n) { nbits -= n; }
    JPEG_HD int get(int n) /* 0 <= n <= 16 */
    {
        nbits -= n;
        return (int)((unsigned)(acc >> nbits) & ((1u << n) - 1u));
    }
    JPEG_HD bool overrun() const { return fake > nbits; }
};

/* How the decoder reads a Huffman table: this form reads the struct where it lies (the host program; the kernel keeps the first-level lookup in
 * registers and has a form of its own, csrc/jpeg_decode.hip LaneHuff). */
struct JpegHuffRef {
    const stm_jpeg_huff* t;
    JPEG_HD int look(unsigned i) const { return t->look[i]; }
    JPEG_HD int maxcode(int l) const { return t->maxcode[l]; }
    JPEG_HD int valoff(int l) const { return t->valoff[l]; }
    JPEG_HD int huffval(int i) const { return t->huffval[i]; }
};

/* The next symbol of table t, or -1 when no code matches within 16 bits.  Needs 16 bits in the reader. */
template <class Bits, class Huff>
JPEG_HD int jpeg_symbol(Bits& br, const Huff& t)
{
    const unsigned v = br.peek16();
    const int e = t.look(v >> (16 - STM_JPEG_LOOK_BITS));
    if (e >> 8) {
        br.skip(e >> 8);
        return e & 255;
    }
    for (int l = STM_JPEG_LOOK_BITS + 1; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= t.maxcode(l)) {
            br.skip(l);
            return t.huffval((code + t.valoff(l)) & 255);
        }
    }
    return -1;
}

/* HUFF_EXTEND: the s-bit field v as a signed value */
JPEG_HD int jpeg_extend(int v, int s)
{
    return (s > 0 && v < (1 << (s - 1))) ? v - (1 << s) + 1 : v;
}

/* One 8x8 block: the DC difference (pred is the component's running prediction) and the AC run / size pairs.  Sink::put(k, value) receives
 * the non-zero coefficients by zig-zag position k (and the DC value, which may be zero) and stores them at natural index jpeg_natural(k); the
 * rest of the block is zero.  -> 0 or STM_JPEG_E*.  At most 64 symbols: every turn of the loop moves k forward. */
template <class Bits, class Huff, class Sink>
JPEG_HD int jpeg_decode_block(Bits& br, const Huff& dc, const Huff& ac, int& pred, Sink& sink)
{
    br.fill();
    int s = jpeg_symbol(br, dc);
    if (s < 0) return STM_JPEG_ENOCODE;
    if (s > 11) return STM_JPEG_ESIZE;
    pred = (int16_t)(pred + jpeg_extend(br.get(s), s));     /* what an int16 coefficient holds; a sound file never wraps */
    sink.put(0, pred);
    int k = 1;
    while (k < 64) {
        br.fill();
        const int rs = jpeg_symbol(br, ac);
        if (rs < 0) return STM_JPEG_ENOCODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;         /* end of block */
            k += 16;                    /* ZRL */
            continue;
        }
        if (s > 10) return STM_JPEG_ESIZE;
        k += r;
        if (k > 63) return STM_JPEG_EINDEX;
        sink.put(k, jpeg_extend(br.get(s), s));
        ++k;
    }
    return br.overrun() ? STM_JPEG_ETRUNCATED : 0;
}

/* ---- the geometry of an image's blocks --------------------------------------------------------------------------------------------------- */

JPEG_HD int jpeg_comp_hs(const stm_jpeg_image& im, int c) { return c == 0 ? im.hs : 1; }
JPEG_HD int jpeg_comp_vs(const stm_jpeg_image& im, int c) { return c == 0 ? im.vs : 1; }
/* blocks per row / rows of blocks of component c */
JPEG_HD int jpeg_comp_bw(const stm_jpeg_image& im, int c) { return im.mcu_w * jpeg_comp_hs(im, c); }
JPEG_HD int jpeg_comp_bh(const stm_jpeg_image& im, int c) { return im.mcu_h * jpeg_comp_vs(im, c); }
/* first block of component c among the image's */
JPEG_HD int jpeg_comp_first(const stm_jpeg_image& im, int c)
{
    return c == 0 ? 0 : im.mcu_w * im.mcu_h * (im.hs * im.vs + (c - 1));
}
JPEG_HD int jpeg_image_blocks(const stm_jpeg_image& im)
{
    return im.kind == STM_JPEG_DECODE ? im.mcu_w * im.mcu_h * (im.hs * im.vs + (im.ncomp - 1)) : 0;
}
JPEG_HD int jpeg_image_quads(const stm_jpeg_image& im) { return (im.width * im.height + 3) >> 2; }

/* A split image (csrc/jpeg.h, stm_jpeg_image.split): the sub-sequences and groups of a segment of nbytes, and whether the sub-sequences' records
 * (32 bytes each) fit in the plane region of an image of `blocks` blocks (64 bytes each). */
JPEG_HD int jpeg_blocks_per_mcu(const stm_jpeg_image& im) { return im.hs * im.vs + (im.ncomp - 1); }
JPEG_HD int jpeg_split_subs(int nbytes) { return nbytes / STM_JPEG_SUB_BYTES + (nbytes % STM_JPEG_SUB_BYTES != 0); }
JPEG_HD int jpeg_split_groups(int nbytes) { return (jpeg_split_subs(nbytes) + STM_JPEG_SUB_GROUP - 1) / STM_JPEG_SUB_GROUP; }
JPEG_HD bool jpeg_split_fits(int nbytes, int blocks)
{
    return nbytes > STM_JPEG_SUB_BYTES && nbytes <= STM_JPEG_SPLIT_MAX_BYTES && (int64_t)jpeg_split_subs(nbytes) * 32 <= (int64_t)blocks * 64;
}

/* ---- launch 2: dequantised coefficients -> samples ---------------------------------------------------------------------------------------- */

/* One 8-point pass of jidctint.c (jpeg_idct_islow) over dequantised values; shift = 11 for the column pass, 18 for the row pass. */
JPEG_HD void jpeg_idct8(const int32_t in[8], int32_t out[8], int shift)
{
    typedef uint32_t U;
    U z2 = (U)in[2], z3 = (U)in[6];
    U z1 = (z2 + z3) * 4433u;
    U t2 = z1 + z3 * (U)-15137;
    U t3 = z1 + z2 * 6270u;
    z2 = (U)in[0];
    z3 = (U)in[4];
    U t0 = (z2 + z3) << 13, t1 = (z2 - z3) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = (U)in[7];
    t1 = (U)in[5];
    t2 = (U)in[3];
    t3 = (U)in[1];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    U z4 = t1 + t3;
    const U z5 = (z3 + z4) * 9633u;
    t0 *= 2446u;
    t1 *= 16819u;
    t2 *= 25172u;
    t3 *= 12299u;
    z1 *= (U)-7373;
    z2 *= (U)-20995;
    z3 *= (U)-16069;
    z4 *= (U)-3196;
    z3 += z5;
    z4 += z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const U r = (U)1 << (shift - 1);
    out[0] = (int32_t)(t10 + t3 + r) >> shift;
    out[7] = (int32_t)(t10 - t3 + r) >> shift;
    out[1] = (int32_t)(t11 + t2 + r) >> shift;
    out[6] = (int32_t)(t11 - t2 + r) >> shift;
    out[2] = (int32_t)(t12 + t1 + r) >> shift;
    out[5] = (int32_t)(t12 - t1 + r) >> shift;
    out[3] = (int32_t)(t13 + t0 + r) >> shift;
    out[4] = (int32_t)(t13 - t0 + r) >> shift;
}

/* level shift and clamp */
JPEG_HD int jpeg_sample(int32_t v)
{
    /* v + 128 cannot overflow: v is a value shifted right by 18 */
    v += 128;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

/* ---- launch 3: planes -> pixels ----------------------------------------------------------------------------------------------------------- */

/* h2v1: output column xo of a chroma row of dw real samples */
JPEG_HD int jpeg_h2v1(const uint8_t* row, int dw, int xo)
{
    const int cx = xo >> 1, c = row[cx];
    if (dw <= 2) return c;
    if (xo & 1) return cx == dw - 1 ? c : (3 * c + row[cx + 1] + 2) >> 2;
    return cx == 0 ? c : (3 * c + row[cx - 1] + 1) >> 2;
}

/* h2v2: output (xo, yo) of a chroma plane pw wide with dw x dh real samples */
JPEG_HD int jpeg_h2v2(const uint8_t* p, int pw, int dw, int dh, int xo, int yo)
{
    const int cy = yo >> 1, cx = xo >> 1;
    if (dw <= 2) return p[(int64_t)cy * pw + cx];
    const int ny = (yo & 1) ? (cy + 1 < dh ? cy + 1 : dh - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t* cur = p + (int64_t)cy * pw;
    const uint8_t* nb = p + (int64_t)ny * pw;
    const int t = 3 * cur[cx] + nb[cx];
    if (xo & 1) return cx == dw - 1 ? (4 * t + 7) >> 4 : (3 * t + (3 * cur[cx + 1] + nb[cx + 1]) + 7) >> 4;
    return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + (3 * cur[cx - 1] + nb[cx - 1]) + 8) >> 4;
}

JPEG_HD int jpeg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

/* Pixel (x, y) of the image whose planes start at `planes` (component c's at planes + 64 * jpeg_comp_first(im, c)) -> r, g, b */
JPEG_HD void jpeg_pixel(const stm_jpeg_image& im, const uint8_t* planes, int x, int y, int& r, int& g, int& b)
{
    const int pw0 = jpeg_comp_bw(im, 0) * 8;
    const int Y = planes[(int64_t)y * pw0 + x];
    if (im.ncomp == 1) {
        r = g = b = Y;
        return;
    }
    const int pwc = im.mcu_w * 8;
    const uint8_t* pb = planes + (int64_t)64 * jpeg_comp_first(im, 1);
    const uint8_t* pr = planes + (int64_t)64 * jpeg_comp_first(im, 2);
    int cb, cr;
    if (im.hs == 1) {                      /* 4:4:4 (vs == 1 too) */
        cb = pb[(int64_t)y * pwc + x];
        cr = pr[(int64_t)y * pwc + x];
    } else {
        const int dw = (im.width + 1) >> 1;
        if (im.vs == 1) {                  /* 4:2:2 */
            cb = jpeg_h2v1(pb + (int64_t)y * pwc, dw, x);
            cr = jpeg_h2v1(pr + (int64_t)y * pwc, dw, x);
        } else {                           /* 4:2:0 */
            const int dh = (im.height + 1) >> 1;
            cb = jpeg_h2v2(pb, pwc, dw, dh, x, y);
            cr = jpeg_h2v2(pr, pwc, dw, dh, x, y);
        }
    }
    cb -= 128;
    cr -= 128;
    r = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
    b = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    g = jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
}

/* ---- the argument checks of stm_jpeg_decode_u8 over the host descriptors (host only), shared with the host program ------------------------ */

/* 0 when image `im` is one the kernels may run, else what is wrong with it */
inline const char* jpeg_image_reason(const stm_jpeg_image& im)
{
    if (im.kind != STM_JPEG_DECODE && im.kind != STM_JPEG_RAW) return "kind";
    if (im.width < 1 || im.width > STM_JPEG_MAX_DIM || im.height < 1 || im.height > STM_JPEG_MAX_DIM) return "a width or height outside 1..8192";
    if (im.out_off < 0 || im.out_off % 16 || im.src_off < 0 || im.src_off % 16) return "a misaligned or negative offset";
    if (im.kind == STM_JPEG_RAW) return im.ncomp == 3 ? 0 : "a raw image with other than 3 components";
    if (im.ncomp != 1 && im.ncomp != 3) return "a component count other than 1 or 3";
    if (!((im.hs == 1 && im.vs == 1) || (im.ncomp == 3 && im.hs == 2 && (im.vs == 1 || im.vs == 2)))) return "unsupported sampling factors";
    if (im.mcu_w != (im.width + 8 * im.hs - 1) / (8 * im.hs) || im.mcu_h != (im.height + 8 * im.vs - 1) / (8 * im.vs)) return "MCU counts that are not the size's";
    for (int c = 0; c < im.ncomp; ++c)
        if (im.tq[c] < 0 || im.tq[c] > 3 || im.td[c] < 0 || im.td[c] > 1 || im.ta[c] < 0 || im.ta[c] > 1) return "a table selector out of range";
    return 0;
}

/* The whole batch: every image, the numbering of blocks and 4-pixel groups, where frames and sources lie, and the segments, which must tile each
 * image's MCUs in order.  -> STM_OK, STM_EINVAL or STM_EUNSUPPORTED; *why (a string constant) and *which (the image or segment) say what.
 * total_blocks: the batch's 8x8 blocks (the workspace holds 192 bytes for each), total_quads: its 4-pixel groups.  (The batch's sub-sequence
 * groups: jpeg_total_groups(), once this has passed.) */
inline int jpeg_check_batch(const stm_jpeg_image* images, int n_images, const stm_jpeg_segment* segments, int n_segments, size_t blob_bytes,
                            size_t out_bytes, int64_t* total_blocks, int64_t* total_quads, const char** why, int* which)
{
    int64_t blocks = 0, quads = 0, groups = 0;
    int seg = 0;
    *why = "";
    *which = 0;
    for (int i = 0; i < n_images; ++i) {
        const stm_jpeg_image& im = images[i];
        *which = i;
        if ((*why = jpeg_image_reason(im)) != 0) return STM_EINVAL;
        *why = "";
        const int64_t q = jpeg_image_quads(im);
        if (im.blk_first != blocks || im.quad_first != quads) { *why = "blk_first / quad_first that do not continue the images before"; return STM_EINVAL; }
        if ((uint64_t)im.out_off + 12 * (uint64_t)q > out_bytes) { *why = "a frame outside out"; return STM_EINVAL; }
        const uint64_t src_bytes = im.kind == STM_JPEG_RAW ? 12 * (uint64_t)q : sizeof(stm_jpeg_tables);
        if ((uint64_t)im.src_off + src_bytes > blob_bytes) { *why = "tables or pixels outside the blob"; return STM_EINVAL; }
        blocks += jpeg_image_blocks(im);
        quads += q;
        if (blocks >= ((int64_t)1 << 31) || quads >= ((int64_t)1 << 31)) { *why = "2^31 blocks or 4-pixel groups in one batch"; return STM_EUNSUPPORTED; }
        /* the image's segments: next in the list, MCUs in order, none empty */
        const int seg_begin = seg;
        int64_t mcu = 0;
        const int64_t mcus = im.kind == STM_JPEG_DECODE ? (int64_t)im.mcu_w * im.mcu_h : 0;
        while (mcu < mcus) {
            if (seg >= n_segments || segments[seg].image != i) { *why = "segments that do not cover its MCUs"; return STM_EINVAL; }
            const stm_jpeg_segment& s = segments[seg];
            if (s.mcu_first != mcu || s.mcu_count < 1 || s.mcu_count > mcus - mcu) { *why = "segments that do not tile its MCUs in order"; return STM_EINVAL; }
            if (s.nbytes < 0 || s.byte_off < 0 || s.byte_off % 16 || (uint64_t)s.byte_off + (((uint64_t)s.nbytes + 15) & ~(uint64_t)15) > blob_bytes) {
                *why = "a segment misaligned or outside the blob";
                return STM_EINVAL;
            }
            mcu += s.mcu_count;
            ++seg;
        }
        /* the split field: the groups before this image, and whether it has any itself */
        if (im.split < 0 || (im.split >> 1) != groups) { *why = "a split field that does not continue the groups of the images before"; return STM_EINVAL; }
        if (im.split & 1) {
            if (im.kind != STM_JPEG_DECODE || seg - seg_begin != 1) { *why = "a split field and other than one segment"; return STM_EINVAL; }
            if (!jpeg_split_fits(segments[seg_begin].nbytes, jpeg_image_blocks(im))) { *why = "a split field and a segment whose records do not fit"; return STM_EINVAL; }
            groups += jpeg_split_groups(segments[seg_begin].nbytes);
            if (groups >= ((int64_t)1 << 30)) { *why = "2^30 sub-sequence groups in one batch"; return STM_EUNSUPPORTED; }
        }
    }
    if (seg != n_segments) { *which = seg; *why = "segments beyond the images'"; return STM_EINVAL; }
    *total_blocks = blocks;
    *total_quads = quads;
    return STM_OK;
}

/* the sub-sequence groups of a batch that jpeg_check_batch has passed: the last image's first group and, if it is split, those of its one
 * segment, which is the last of the list */
inline int64_t jpeg_total_groups(const stm_jpeg_image* images, int n_images, const stm_jpeg_segment* segments, int n_segments)
{
    if (n_images <= 0) return 0;
    const stm_jpeg_image& im = images[n_images - 1];
    return (im.split >> 1) + ((im.split & 1) && n_segments > 0 ? jpeg_split_groups(segments[n_segments - 1].nbytes) : 0);
}
