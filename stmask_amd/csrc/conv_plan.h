// conv_plan.h -- the launch plan of the planar convolution (conv_bf16x.hip: conv2d_planar_impl): which kernel a layer gets and how it is
// cut.  Host only, plain C++17: no HIP type, no tensor pointer, no stm_conv_geom -- the rules read a few integers and flags (ConvFacts) and
// the STM_CONV_* switches (ConvTunables; conv_bf16x.hip reads the environment) and answer with a ConvPlan.  Every rule here was measured; the
// paragraph in front of a rule is its measurement history.  stm_debug_conv2d_planar_plan prints the plan of a call without launching it
// (tests/test_conv_plan_cpu.py holds the selection to tests/golden/conv_plan.json).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace conv_plan {

// Constants that were switches until round 6 (DESIGN.md section 9 keeps what their alternatives measured):
constexpr int CV_RING64_SMALL = 512;   // grids up to this many workgroups take the ring on 128 x 64 tiles whatever K (round 2 sweep)
constexpr int CV_SK_TARGET = 256;      // workgroups the split-K rule of the 64-wide tiles aims at (one per CU)
// (removed with their code in round 7: round 1's split-K rule for every layer, nontemporal plane stores for large outputs -- no gain
// measured in rounds 2-4 --, the element-wise epilogue as a cross-check form, the regrouped tile map)
struct ConvTunables {
    int ring = 3;          // STM_CONV_RING: 2 = two-buffer loop on the 128-wide tiles, 3 = three-buffer ring (fp16 formats)
    int ring64 = 3;        // STM_CONV_RING64: 2 never / 4 always the ring on 128 x 64 tiles, 3 = by K length (rule below)
    int splitk = 0;        // STM_CONV_SPLITK: force this many K parts (0 = rule)
    int mg = 0;            // STM_CONV_MG: force 128 (1) or 256 (2) pixel tiles
    int abl = 0;           // STM_CONV_ABL (builds with -DSTM_ABLATE only)
    int kx3 = 1;           // STM_CONV_KX3: 0 = stride-1 kw = 3 layers on the 256 x 128 ring tiles stay on conv_planar_kernel (1: conv_planar_kx3_kernel, kx-reuse staging)
};

// what the kernels fix (conv_bf16x.hip asserts that these are its CV_BM, KX3_WBUF and KX3_LDS_LOOP)
constexpr int BM = 128;                                        // output pixels of a tile at MG = 1
constexpr int KX3_WBUF = 2 * 128 * 64;                         // one weight slab of conv_planar_kx3_kernel's ring
constexpr int KX3_LDS_LOOP = 2 * 2 * 272 * 64 + 3 * KX3_WBUF;  // its two activation buffers + the weight ring

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// What the rules read of a call, after its arguments were checked.
struct ConvFacts {
    int bn;                // tile width the weights were packed for: 64 or 128
    int fmt, planes;       // plane format 0 / 1 / 2 and the planes of format 0 (3, or 2 = its three-product mode)
    int groups, cout_g;
    bool full;             // (128 x 64 tiles) every group fills its 64-channel tiles: the layer can take the ring loop; the narrow ones (output layers
                           // with 41 / 5 / 32 real channels of 64, offset convolutions) keep the two-buffer loop with its skip of all-padding column tiles
    int slabs;             // K-slabs: taps x input channels / 32
    int kh, kw, sh, sw, ph, pw;
    int64_t M;             // output pixels
    int n_tiles;           // channel tiles
    bool dual, win, gated; // second source / single window launch / pixel gate set
    bool ws_usable;        // a workspace was given and is 16-byte aligned
    size_t ws_bytes;
    int ldp;               // row length of the split-K partial sums
};

// One launch: the kernel and its cut.
struct ConvPlan {
    bool kx3 = false;                                          // conv_planar_kx3_kernel<KX3_ABL, cls != 0>; else
    int npl = 0, mg = 0, nj = 0, dt = 0, st = 0, abl = 0;      // conv_planar_kernel<NPL, MG, NJ, DT, ST, ABL, DUAL, CLS>
    bool dual = false;
    int cls = 0;                                               // 0 one layer, 1 window set, 2 gated (segmented) window set
    int m_tiles = 0, splitk = 1, kslabs = 0;
    unsigned grid = 0, block = 0;
    size_t lds = 0;                                            // dynamic LDS bytes
};

// ---- LDS ----------------------------------------------------------------------------------------------------------------------------
inline size_t planar_lds(int npl, int mg, int nj, int st)
{
    size_t lds = (size_t)st * (npl * BM * mg * 64 + npl * (64 * nj) * 64);
    const size_t park = (size_t)4 * mg * 64 * (32 * nj + 4) * sizeof(float);   // the epilogue parks one 64 x 32NJ tile per wave
    return lds < park ? park : lds;
}
inline size_t kx3_lds(bool win)
{
    if (win) return 2 * 2 * 384 * 64 + 3 * KX3_WBUF;      // two 48-KB activation buffers + the weight ring (the epilogue's park needs less)
    return std::max<size_t>(8 * 64 * (64 + 4) * sizeof(float), (size_t)KX3_LDS_LOOP);
}

// ---- split-K ------------------------------------------------------------------------------------------------------------------------
// split-K for grids that would leave most CUs idle over a long K (small feature maps: ResNet stages 3/4, P5-P7):
// parts write fp32 partial sums into the caller's workspace, planar_splitk_finish_kernel adds them and runs the epilogue.
// (A fused reduction -- the part drawing a tile's last ticket adds the parts -- was built and measured twice.  Round 1 with
// device-scope fences: an L2 write-back / invalidate per workgroup, 665 vs 919 frames/s.  Round 2 without any fence -- the
// parts' sums written and read as agent-scope relaxed atomics (sc1 accesses), store -> vmcnt(0) -> ticket ... ticket -> load
// -- to save the 47 finishing launches of a single-stream step (12 % of its GPU time): 359 vs 461 frames/s at 1 clip, 965 vs
// 1047 at 8, 1201 vs 1214 at 32.  One workgroup adding a tile's parts at the end of the kernel is a longer tail than the
// finishing kernel's few thousand threads after it; removed again.)
inline void plan_splitk(ConvPlan& p, const ConvFacts& f, const ConvTunables& tn, int tiles)
{
    if (f.gated) return;         // (the finishing kernel knows no gate, and a gated launch is sized for a capacity, not for its work)
    int sk = tn.splitk;
    if (sk <= 0) {
        sk = 1;
        if (f.bn == 64) {
            // 128 x 64 tiles: grids of at most half a workgroup per CU are split until about one workgroup per CU exists,
            // with at least 16 K-slabs per part (10 on the tiniest grids).  Re-measured in round 2 with every configuration
            // replayed from a HIP graph (scripts/sweep_small_m.py; round 1's rule -- up to 256 tiles, three workgroups per
            // CU, 10 slabs per part -- dated from before the ring loop took the small grids): 240 tiles x 32 slabs 31.9 us
            // split in 3 vs 20.2 unsplit, 240 x 72 slabs 49.5 vs 39.8, 120 tiles x 64 slabs 29.8 (6 parts) vs 24.4 (2),
            // 64 x 64 19.4 (6) vs 17.3 (4), 240 x 36 (layer2's 3x3 at 4 clips) 34.3 vs 20.0.
            // The narrow layers (two-buffer loop) keep round 1's rule: 120 tiles x 72 slabs 36.8 us in 6 parts, 55.2 in 2.
            if (!f.full) {
                if (tiles <= 256 && f.slabs >= 24) sk = (int)std::min<int64_t>(std::min<int64_t>(8, 768 / tiles), f.slabs / 10);
            } else if (tiles <= 128 && f.slabs >= 24)
                sk = (int)std::min<int64_t>(std::min<int64_t>(8, CV_SK_TARGET / tiles), f.slabs / (tiles <= 40 ? 10 : 16));
        } else if (tiles < 128 && f.slabs >= 24) sk = (int)std::min<int64_t>(std::min<int64_t>(8, 256 / tiles), f.slabs / 12);
    }
    if (sk < 2) return;
    const int per = cdiv(f.slabs, sk);
    sk = cdiv(f.slabs, per);
    if (sk < 2 || !f.ws_usable || (size_t)sk * f.M * f.ldp * sizeof(float) > f.ws_bytes) return;
    p.splitk = sk; p.kslabs = per;
}

// ---- one layer ----------------------------------------------------------------------------------------------------------------------
inline ConvPlan plan_conv(const ConvFacts& f, const ConvTunables& tn)
{
    ConvPlan p;
    p.npl = f.fmt == 2 ? 1 : (f.fmt == 1 ? 2 : (f.planes == 3 ? 3 : 2));
    p.dt = f.fmt >= 1 ? 1 : 0;
    p.dual = f.dual;
    p.kslabs = f.slabs;
    if (f.bn == 64) {
        // 128 x 64 tiles, 72 KB of LDS: two independent workgroups per CU, each one's barrier / staging gaps filled by
        // the other's MFMAs
        p.mg = 1; p.nj = 1;
        p.m_tiles = cdiv(f.M, BM);
        plan_splitk(p, f, tn, p.m_tiles * f.n_tiles);
        const int tiles = p.m_tiles * f.n_tiles * p.splitk;
        // the three-buffer ring (72 KB: still two workgroups per CU) has no skip of zero-padded column tiles: `full` layers only
        // measured in the graph (bench.py --layer-table): the ring wins on the short K loops (<= 36 slabs: 35 -> 30 us,
        // 46 -> 36 us, 45 -> 37 us), where its two-slab head start hides the first DMA latency, and loses on the long and
        // the split-K ones (100 -> 114 us at 72 slabs), where two resident two-buffer workgroups already cover each other;
        // under 12 slabs the layer is HBM-bound and the two-buffer loop's 48 KB (three workgroups per CU) wins: 302 vs 389 us
        // grids of at most two workgroups per CU (single-stream / small batches: every layer; layer4 at 8 clips) have no further
        // resident workgroup to cover a workgroup's staging gaps: the ring whatever K.  Swept 0 / 128 / 256 / 512 / 1024 on one
        // box (scripts/sweep_ring64_small.sh): 1 clip 399 / 421 / 436 / 456 / 452 frames/s, 2 clips 628 .. 662, 4 clips 836 ..
        // 880, 8 clips flat (1053), 32 clips 1219 .. 1226.
        const bool small_grid = tiles <= CV_RING64_SMALL;
        const bool ring = f.full && (tn.ring64 == 3 ? (small_grid || (p.splitk == 1 && f.slabs >= 12 && f.slabs <= 40)) : tn.ring64 == 4);
        p.st = (f.fmt >= 1 && ring) ? 3 : 2;
        p.grid = 8 * cdiv(tiles, 8);
    } else {
        // 256-pixel tiles once there are enough of them, else 128-pixel tiles.  (A cost model of rounds x tile time x measured
        // efficiency was tried for this choice and for the 64-channel tile: 478-483 frames/s against 502-509 with these plain
        // thresholds in the same session -- rejected.  So was a kx-reuse kernel that stages each activation row once per kernel
        // row: 1.8x fewer DMA bytes, no gain -- 654 vs 670 us on the 145-GF proto layer -- removed.  Round 2 rebuilt it on the
        // three-buffer ring -- one staged copy of BM + 2 pixels per (channel slab, ky) serving kx = 0, 1, 2 at LDS row r + kx, an
        // all-zero LDS row for the padding columns, stage parts spread over the three K-slabs, bit-identical results: half the
        // activation DMA instructions, 1/2.8 of their L2 reads, and 1.5-2.5 % SLOWER on every 3x3 layer (proto 1465 vs 1440 us,
        // tower 1850 vs 1807, TemporalNet conv3 2993 vs 2953).  Its own ablations: no stage DMA at all 1406 -> 1188 us, no
        // per-tap register rotation 1379, never waiting for a stage to land 1378.  The cost of the activation staging follows
        // the number of DMA instructions issued (~30 clocks of a wave's issue each), not the bytes they fetch or their latency,
        // and the bookkeeping of the reuse eats what the fewer instructions give back -- removed again.  The three-slab body
        // unrolled (compile-time taps, no rotation) made the register allocator migrate the accumulators: 53 quads, 54 spills.)
        const int64_t t2 = (int64_t)cdiv(f.M, 2 * BM) * f.n_tiles;
        p.mg = tn.mg ? tn.mg : (t2 >= 192 ? 2 : 1);
        p.nj = 2;
        p.m_tiles = cdiv(f.M, BM * p.mg);
        plan_splitk(p, f, tn, p.m_tiles * f.n_tiles);
        const int tiles = p.m_tiles * f.n_tiles * p.splitk;
        const bool ring = tn.ring == 3;
        p.grid = 8 * cdiv(tiles, 8);
#ifdef STM_ABLATE
        if (f.fmt == 1 && ring && p.mg == 2 && tn.abl) {      // timing ablations of the ring loop: RESULTS ARE WRONG
            const int abl = tn.abl;
            p.abl = (abl == 1 || abl == 2 || abl == 3 || abl == 5 || abl == 8 || abl == 16 || abl == 32 || abl == 64) ? abl : 7;
            p.st = 3; p.dual = false;
        } else
#endif
        if (tn.kx3 && f.fmt == 1 && ring && p.mg == 2 && !f.dual && !f.win && p.splitk == 1 && f.kw == 3 && f.pw == 1 && f.sh == 1 && f.sw == 1 &&
            f.slabs % 3 == 0 && f.kh <= 6 && 2 * f.ph == f.kh - 1 && f.full) {
            // ("same" padding in height too: the kernel decodes a pixel index ONCE and uses it for the output and the staged input rows alike, so
            // Ho == H and Wo == W are part of its contract -- a 3x3 layer with padding (0, 1) stays on conv_planar_kernel)
            // kx-reuse staging (conv_planar_kx3_kernel): one staged run of BM + 2 pixels per (channel slab, ky) serves the three taps of a kernel row
            p.kx3 = true;
            p.block = 512;
            p.lds = kx3_lds(false);
            return p;
        } else {
            p.st = (f.fmt >= 1 && (ring || f.dual)) ? 3 : 2;      // (the 128-wide tiles of the fp16 formats always take the ring loop with a second source)
        }
    }
    p.block = 256 * p.mg;
    p.lds = planar_lds(p.npl, p.mg, p.nj, p.st);
    return p;
}

// ---- window sets --------------------------------------------------------------------------------------------------------------------
// every tap of every pixel of a Ho x Wo window (sub-kernel kh x kw, padding ph / pw <= 0) inside the H x W input map
inline bool taps_inside(int kh, int kw, int ph, int pw, int Ho, int Wo, int H, int W)
{
    return -ph >= 0 && -ph + (Ho - 1) + (kh - 1) <= H - 1 && -pw >= 0 && -pw + (Wo - 1) + (kw - 1) <= W - 1;
}
// A window of a plain set takes the kx-reuse form: every tap inside the input map (no zero fill to stage), and a tile's window rows with their two
// halo pixels fit 384 staged rows
inline bool window_takes_kx3(const ConvTunables& tn, int kh, int kw, int ph, int pw, int Ho, int Wo, int H, int W)
{
    return tn.kx3 && kw == 3 && kh <= 6 && taps_inside(kh, kw, ph, pw, Ho, Wo, H, W) && (255 / Wo + 2) * (Wo + 2) <= 384;
}
// The grid of a window set's classes on the 256 x 128 ring tiles of the fp16x2 format: cls = 1 / 2 on conv_planar_kernel<2, 2, 2, 1, 3, abl, false, cls>,
// kx3 on conv_planar_kx3_kernel<., true>.  cls_tiles = the tiles of all classes, slabs = the K-slabs of window 0 (the kernels read their class's own).
// (grid: every XCD gets the same number of pixel tiles x all channel tiles; ids past the last tile leave at once)
inline ConvPlan plan_window_set(bool kx3, int cls, int abl, int cls_tiles, int n_tiles, int slabs)
{
    ConvPlan p;
    p.kx3 = kx3; p.cls = cls;
    p.npl = 2; p.mg = 2; p.nj = 2; p.dt = 1; p.st = 3; p.abl = abl;
    p.kslabs = slabs;
    p.grid = cdiv(cls_tiles / n_tiles, 8) * 8 * n_tiles;
    p.block = 512;
    p.lds = kx3 ? kx3_lds(true) : planar_lds(p.npl, p.mg, p.nj, p.st);
    return p;
}

}  // namespace conv_plan
