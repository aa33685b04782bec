// head_sparse.hip -- the shared prediction head at the positions that pass the class threshold (stmask_amd/planar.py, sparse head).
//
// generate_candidate (TF_utils.py:54-82) keeps a prior only where max(softmax(conf)[1:]) > eval_conf_thresh, and loc / centerness /
// mask_coeff / track are read at kept priors only.  So only the class branch of the head has to be dense; the three other branches are
// computed on the 9 x 9 neighbourhoods ("patches") of the positions with a kept prior -- the receptive field of a 3x3 -> 3x3 -> (3x3 | 3x5 |
// 5x3) stack: valid convolutions 9 x 9 -> 7 x 7 -> 5 x 5, the output layers at the centre pixel.  Everything is sized by a fixed capacity and steered by device counts (no host read; the launches live in a captured graph):
//
//   head_candidates_kernel    class logits of the K kernel shapes -> list of the pixels with a kept prior (arithmetic of row_stats_kernel<true>,
//                             postproc.hip, value for value), their count
//   head_list_kernel          (split form) flags -> the list, positions with a kept prior of their own in front
//   head_control_kernel       count -> the control block the other launches read (below); more positions than the capacity -> the patch
//                             launches are empty and the dense launches of the three branches run instead (the convolution launches are gated
//                             by stm_conv_set_pixel_gate)
//   head_control_segs_kernel, head_list_segs_kernel   (shapes form) the same for (pixel, kernel shape) entries in one segment per shape, each
//                             with its own counts and gates: the patch towers then run over the rectangle that shape's output layers read
//   head_patch_gather_kernel  S x S neighbourhoods of the listed positions from the level maps (zeros outside the map)
//   head_patch_mask_kernel    zeroes the patch pixels outside the map in place (after each tower layer: the next layer's padding)
//   head_assemble_*           prediction_head_FC.py:168-195 as head_assemble_kernel (mask_ops.hip) does it, same arithmetic: conf for every prior,
//                             the four other tensors at the kept positions' rows (or, after an overflow, at every row from the dense launches)
#include <algorithm>
#include <climits>

#include "stm_common.h"

namespace {

// control block (ints on the device)
enum { CTL_RAW = 0,      // positions found (may exceed the capacity)
       CTL_N = 1,        // positions listed and computed: CTL_RAW, or 0 after an overflow
       CTL_FILL = 2,     // patches the launches cover: CTL_N rounded up to 256 (<= capacity) -- patches [CTL_N, CTL_FILL) are zeros, so that
                         // launches of any tile height cover the same whole patches and nothing reads memory no launch of this step wrote
       CTL_GATE_A = 3,   // CTL_FILL * output pixels of a patch in the first tower layer: pixel gate of that launch
       CTL_GATE_B = 4,   // CTL_FILL * output pixels of a patch in the second tower layer (= input pixels of the output layers)
       CTL_DENSE = 5,    // pixel gate of the dense launches of the three branches: all pixels after an overflow, else 0
       CTL_OVERFLOW = 6,
       CTL_GATE_POS = 7, // CTL_N: position gate of the output layers' one-pixel window launches (one output row per listed position)
       CTL_INTS = 8,
       // Split form (a negative capacity at the entry points): a second block of the same fields over the OWN positions -- the pixels with a kept
       // prior of their own, list[0, n_own); list[n_own, n) are the partner-only positions, where only centerness is read, so only the bbox branch
       // runs there.  A launch of the mask / track branches takes ctl + CTL_OWN as its control block or gate and is otherwise the same launch.
       CTL_OWN = 8,
       // Shapes form (K << 28 added to the capacity at the entry points): the list holds (pixel, kernel shape) ENTRIES in K segments of `capacity`
       // entries each, segment k = list[k capacity, (k + 1) capacity), own entries in front of the partner-only ones as in the split form.  Segment k
       // has a pair of blocks of its own at ctl + CTL_SEG (k + 1) (all entries, own entries); the pair at ctl keeps CTL_RAW / CTL_N as the sums over
       // the segments and CTL_DENSE / CTL_OVERFLOW for the dense launches (any segment over its capacity is an overflow of the step).
       CTL_SEG = 16 };
enum { FLAG_OWN = 1, FLAG_PARTNER = 2 };
constexpr int SEG_SHIFT = 28, SEG_CAP_MASK = (1 << SEG_SHIFT) - 1;      // capacity argument = entries per segment + (segments << 28)

// cumulative index j over the segments' counts c[0 .. n_seg) -> (segment, index inside it); false past the last one
__device__ __forceinline__ bool seg_locate(const int (&c)[4], int n_seg, int j, int& k, int& i)
{
    k = 0; i = j;
    int lim = c[0];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        if (k == s && s + 1 < n_seg && i >= c[s]) { i -= c[s]; k = s + 1; lim = c[s + 1]; }
    return i < lim;
}
__device__ __forceinline__ void seg_counts(const int* ctl, int n_seg, int field, int (&c)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) c[s] = s < n_seg ? ctl[CTL_SEG * (s + 1) + field] : 0;
}

struct Levels {
    int n, B;
    int start[9], h[8], w[8];
};

__device__ __forceinline__ void decode_pixel(const Levels& L, int m, int& l, int& b, int& y, int& x)
{
    l = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
        if (i < L.n && m >= L.start[i]) l = i;
    const int r = m - L.start[l], hw = L.h[l] * L.w[l];
    b = r / hw;
    const int p = r - b * hw;
    y = p / L.w[l];
    x = p - y * L.w[l];
}

struct CandArgs {
    const float* cls[4];
    int K, ld, n_cls, n_pixels, capacity;
    float thresh;
    int* list;
    int* ctl;
    int* flags;            // [n_pixels], zero on entry: 1 = the pixel is listed; split form: FLAG_OWN | FLAG_PARTNER, and two list cursors behind them
    int split;
    Levels L;
};

__global__ __launch_bounds__(256) void head_clear_kernel(int* ctl, int* flags, int n_flags, int n_ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_flags) flags[i] = 0;
    else if (i < n_flags + n_ctl) ctl[i - n_flags] = 0;
}

__device__ __forceinline__ void list_pixel(const CandArgs& a, int m)
{
    if (atomicCAS(a.flags + m, 0, 1) != 0) return;
    const int i = atomicAdd(a.ctl + CTL_RAW, 1);
    if (i < a.capacity) a.list[i] = m;
}

// split form: the first thread to make a flag non-zero counts the position, the first to set the own bit counts an own position; head_list_kernel
// writes the list
__device__ __forceinline__ void flag_pixel(const CandArgs& a, int m, int bit)
{
    const int old = atomicOr(a.flags + m, bit);
    if (old == 0) atomicAdd(a.ctl + CTL_RAW, 1);
    if (bit == FLAG_OWN && !(old & FLAG_OWN)) atomicAdd(a.ctl + CTL_OWN + CTL_RAW, 1);
}

// shapes form: a flag holds one own bit (1 << k) and one partner bit (16 << k) per kernel shape; the first thread to set either bit of shape k counts
// the entry (pixel, k) in segment k's block, the first to set the own bit counts an own entry
__device__ __forceinline__ void flag_entry(const CandArgs& a, int m, int k, bool own)
{
    const int old = atomicOr(a.flags + m, (own ? 1 : 16) << k);
    int* c = a.ctl + CTL_SEG * (k + 1);
    if (!(old & (17 << k))) atomicAdd(c + CTL_RAW, 1);
    if (own && !(old & (1 << k))) atomicAdd(c + CTL_OWN + CTL_RAW, 1);
}

// CAND_PX pixels per workgroup; the class logits of their K priors (one per kernel shape) are copied coalesced into LDS (rows of an odd stride), then
// one thread per (shape, pixel) row tests it with the candidate pass's own arithmetic (row_stats_kernel<true>: max over the foreground logits, max
// with the background, sum of exp(x - max) in class order, p = exp(m - max) / sum, keep = p > thresh).  A kept prior (pixel p, shape k) of a level
// is row r = p K + k of the level in loc / mask_coeff / track, and row r of the level in centerness -- which the reference concatenates along H
// (prediction_head_FC.py:189), so that row holds shape r / hw at pixel r % hw.  Both pixels are listed, each once.  The list order is the order of
// arrival: results land in rows fixed by the position.
constexpr int CAND_PX = 64;

__global__ __launch_bounds__(256) void head_candidates_kernel(const CandArgs a, int vec)
{
    extern __shared__ float slab[];
    __shared__ unsigned kept_s[CAND_PX];
    const int stride = a.n_cls | 1;
    const int m0 = blockIdx.x * CAND_PX;
    const int rows = min(CAND_PX, a.n_pixels - m0);
    if (threadIdx.x < CAND_PX) kept_s[threadIdx.x] = 0u;
    for (int k = 0; k < a.K; ++k) {
        const float* src = a.cls[k] + (int64_t)m0 * a.ld;
        float* dst = slab + k * CAND_PX * stride;
        if (vec) {
            const int nv = (a.n_cls + 3) >> 2;
            for (int idx = threadIdx.x; idx < rows * nv; idx += 256) {
                const int r = idx / nv, v = idx - r * nv;
                const float4 q = *reinterpret_cast<const float4*>(src + (int64_t)r * a.ld + 4 * v);
                float* d = dst + r * stride + 4 * v;
                d[0] = q.x;
                if (4 * v + 1 < a.n_cls) d[1] = q.y;
                if (4 * v + 2 < a.n_cls) d[2] = q.z;
                if (4 * v + 3 < a.n_cls) d[3] = q.w;
            }
        } else {
            for (int idx = threadIdx.x; idx < rows * a.n_cls; idx += 256) {
                const int r = idx / a.n_cls, c = idx - r * a.n_cls;
                dst[r * stride + c] = src[(int64_t)r * a.ld + c];
            }
        }
    }
    __syncthreads();
    const int k = threadIdx.x / CAND_PX, r = threadIdx.x - k * CAND_PX;
    if (k < a.K && r < rows) {
        const float* row = slab + (k * CAND_PX + r) * stride;
        float mf = row[1];
        for (int c = 2; c < a.n_cls; ++c) mf = row[c] > mf ? row[c] : mf;
        const float mx = row[0] > mf ? row[0] : mf;
        float sum = 0.0f;
        for (int c = 0; c < a.n_cls; ++c) sum += expf(row[c] - mx);
        const float p = expf(mf - mx) / sum;
        if (p > a.thresh) atomicOr(&kept_s[r], 1u << k);
    }
    __syncthreads();
    if (threadIdx.x >= rows) return;
    const unsigned kept = kept_s[threadIdx.x];
    if (!kept) return;
    const int m = m0 + threadIdx.x;
    int l, b, y, x;
    decode_pixel(a.L, m, l, b, y, x);
    const int hw = a.L.h[l] * a.L.w[l], pix = y * a.L.w[l] + x;
    if (a.split == 2) {
        // entries: the kept prior's own (pixel, shape), and the (pixel, shape) whose centerness lands in the prior's row
        for (int kk = 0; kk < a.K; ++kk)
            if (kept >> kk & 1) {
                const int r = pix * a.K + kk;
                flag_entry(a, m, kk, true);
                flag_entry(a, a.L.start[l] + b * hw + r % hw, r / hw, false);
            }
        return;
    }
    if (a.split) flag_pixel(a, m, FLAG_OWN);
    else list_pixel(a, m);
    for (int kk = 0; kk < a.K; ++kk)
        if (kept >> kk & 1) {
            const int pm = a.L.start[l] + b * hw + (pix * a.K + kk) % hw;
            if (a.split) flag_pixel(a, pm, FLAG_PARTNER);
            else list_pixel(a, pm);
        }
}

// blocks = 1: the block over all listed positions; 2: and the block over the own positions behind it (split form; its CTL_RAW holds their count)
__global__ void head_control_kernel(int* ctl, int capacity, int n_pixels, int px_a, int px_b, int blocks)
{
    if (blockIdx.x || (int)threadIdx.x >= blocks) return;
    const bool over = ctl[CTL_RAW] > capacity;
    int* c = ctl + threadIdx.x * CTL_OWN;
    const int n = over ? 0 : c[CTL_RAW];
    const int fill = min(capacity, (n + 255) & ~255);
    c[CTL_N] = n;
    c[CTL_FILL] = fill;
    c[CTL_GATE_A] = fill * px_a;
    c[CTL_GATE_B] = fill * px_b;
    c[CTL_DENSE] = over ? n_pixels : 0;
    c[CTL_OVERFLOW] = over ? 1 : 0;
    c[CTL_GATE_POS] = n;
}

// Split form, after head_control_kernel: own positions to list[0, n_own), partner-only positions to list[n_own, n).  A workgroup counts its 256
// pixels of each class, takes its ranges with one atomic per class from the two cursors behind the flags, and writes; the order inside a class is
// the order of arrival (results land in rows fixed by the position).  Nothing is listed after an overflow (n = 0).
__global__ __launch_bounds__(256) void head_list_kernel(const int* flags, int* cursors, int n_pixels, int capacity, int* list, const int* ctl)
{
    __shared__ int cnt_s[2], base_s[2];
    if (threadIdx.x < 2) cnt_s[threadIdx.x] = 0;
    __syncthreads();
    const int n = ctl[CTL_N], n_own = ctl[CTL_OWN + CTL_N];
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int f = m < n_pixels && n > 0 ? flags[m] : 0;
    const int cls = f & FLAG_OWN ? 0 : (f ? 1 : -1);
    int rank = 0;
    if (cls >= 0) rank = atomicAdd(&cnt_s[cls], 1);
    __syncthreads();
    if (threadIdx.x < 2) base_s[threadIdx.x] = cnt_s[threadIdx.x] ? atomicAdd(cursors + threadIdx.x, cnt_s[threadIdx.x]) : 0;
    __syncthreads();
    if (cls < 0) return;
    const int i = (cls ? n_own : 0) + base_s[cls] + rank;
    if (i < n && i < capacity) list[i] = m;
}

// Shapes form: thread o = 0 / 1 writes the blocks over all / over the own entries -- segment k's at ctl + CTL_SEG (k + 1) + o CTL_OWN, gates in pixels
// of shape k's window of a patch map (px_a / px_b: one 8-bit pixel count per segment), and at ctl + o CTL_OWN the sums over the segments, which no
// launch reads but the dense launches' gate.  One segment over its capacity empties every segment.
__global__ void head_control_segs_kernel(int* ctl, int K, int capacity, int n_pixels, int px_a, int px_b)
{
    const int o = threadIdx.x;
    if (blockIdx.x || o >= 2) return;
    bool over = false;
    for (int k = 0; k < K; ++k) over = over || ctl[CTL_SEG * (k + 1) + CTL_RAW] > capacity;
    int sum[CTL_INTS] = {0, 0, 0, 0, 0, over ? n_pixels : 0, over ? 1 : 0, 0};
    for (int k = 0; k < K; ++k) {
        int* c = ctl + CTL_SEG * (k + 1) + o * CTL_OWN;
        const int raw = c[CTL_RAW], n = over ? 0 : raw;
        const int fill = min(capacity, (n + 255) & ~255);
        c[CTL_N] = n;
        c[CTL_FILL] = fill;
        c[CTL_GATE_A] = fill * (px_a >> 8 * k & 255);
        c[CTL_GATE_B] = fill * (px_b >> 8 * k & 255);
        c[CTL_DENSE] = sum[CTL_DENSE];
        c[CTL_OVERFLOW] = sum[CTL_OVERFLOW];
        c[CTL_GATE_POS] = n;
        sum[CTL_RAW] += raw; sum[CTL_N] += n; sum[CTL_FILL] += fill; sum[CTL_GATE_A] += c[CTL_GATE_A]; sum[CTL_GATE_B] += c[CTL_GATE_B];
        sum[CTL_GATE_POS] += n;
    }
#pragma unroll
    for (int i = 0; i < CTL_INTS; ++i) ctl[o * CTL_OWN + i] = sum[i];
}

// Shapes form, after head_control_segs_kernel: head_list_kernel per segment -- cursors[2 k] / [2 k + 1] are segment k's own / partner-only cursors;
// a pixel with several needed shapes is listed in several segments.
__global__ __launch_bounds__(256) void head_list_segs_kernel(const int* flags, int* cursors, int n_pixels, int K, int capacity, int* list, const int* ctl)
{
    __shared__ int cnt_s[8], base_s[8];
    if (threadIdx.x < 8) cnt_s[threadIdx.x] = 0;
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int f = m < n_pixels ? flags[m] : 0;
    int rank[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < K && (f & (17 << k))) rank[k] = atomicAdd(&cnt_s[2 * k + ((f >> k & 1) ? 0 : 1)], 1);
    __syncthreads();
    if ((int)threadIdx.x < 2 * K) base_s[threadIdx.x] = cnt_s[threadIdx.x] ? atomicAdd(cursors + threadIdx.x, cnt_s[threadIdx.x]) : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < K && (f & (17 << k))) {
            const int* c = ctl + CTL_SEG * (k + 1);
            const int n = c[CTL_N], part = (f >> k & 1) ? 0 : 1;
            const int i = (part ? c[CTL_OWN + CTL_N] : 0) + base_s[2 * k + part] + rank[k];
            if (i < n && i < capacity) list[(int64_t)k * capacity + i] = m;
        }
}

struct GatherArgs {
    const uint8_t* src;    // planes [P][slabs][src_np][32] of 2-byte elements
    uint8_t* dst;          // planes [P][slabs][capacity * S * S][32]
    int rows;              // P * slabs
    int64_t src_np, dst_np;
    int S;                 // side of the patches written
    const int* list;
    const int* ctl;
    int segs, seg_cap;     // shapes form: that many segments of seg_cap patches, each with its own counts (0: one list under ctl)
    Levels L;
};

// One wave per patch pixel and 16 (plane, slab) rows: lane = (row of the 16, 16-byte chunk).  Persistent grid over the patch pixels of the
// CTL_FILL patches this step covers (shapes form: of every segment's CTL_FILL patches, patch i of segment k at slot k seg_cap + i).
__global__ __launch_bounds__(256) void head_patch_gather_kernel(const GatherArgs a)
{
    int fills[4] = {a.ctl[CTL_FILL], 0, 0, 0};
    if (a.segs) seg_counts(a.ctl, a.segs, CTL_FILL, fills);
    const int fill = fills[0] + fills[1] + fills[2] + fills[3];
    const int SS = a.S * a.S, half = a.S >> 1;
    const int row_groups = (a.rows + 15) >> 4;
    const int64_t units = (int64_t)fill * SS * row_groups;
    const int lane = threadIdx.x & 63;
    const int sub_row = lane >> 2, chunk = lane & 3;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * 4) {
        int64_t pp = u / row_groups;                       // patch pixel
        const int rg = (int)(u - pp * row_groups);
        int i = (int)(pp / SS), k = 0;
        const int q = (int)(pp - (int64_t)i * SS);
        if (a.segs) seg_locate(fills, a.segs, i, k, i);
        const int n = a.ctl[(a.segs ? CTL_SEG * (k + 1) : 0) + CTL_N];
        const int slot = k * a.seg_cap + i;
        pp = (int64_t)slot * SS + q;
        const int row = rg * 16 + sub_row;
        if (row >= a.rows) continue;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < n) {
            int l, b, y, x;
            decode_pixel(a.L, a.list[slot], l, b, y, x);
            const int dy = q / a.S - half, dx = q - (q / a.S) * a.S - half;
            const int yy = y + dy, xx = x + dx;
            if ((unsigned)yy < (unsigned)a.L.h[l] && (unsigned)xx < (unsigned)a.L.w[l]) {
                const int64_t sp = (int64_t)a.L.start[l] + ((int64_t)b * a.L.h[l] + yy) * a.L.w[l] + xx;
                v = *reinterpret_cast<const uint4*>(a.src + ((int64_t)row * a.src_np + sp) * 64 + chunk * 16);
            }
        }
        *reinterpret_cast<uint4*>(a.dst + ((int64_t)row * a.dst_np + pp) * 64 + chunk * 16) = v;
    }
}

// In place: the patch pixels of the first CTL_N patches that lie outside their level's map become zero.  One workgroup per patch at a time; a
// patch that lies inside the map (nearly all of them on the fine levels) is left after the test.
__global__ __launch_bounds__(256) void head_patch_mask_kernel(uint8_t* planes, int rows, int64_t np, int S, const int* list, const int* ctl, const Levels L,
                                                              int segs, int seg_cap)
{
    int ns[4] = {ctl[CTL_N], 0, 0, 0};
    if (segs) seg_counts(ctl, segs, CTL_N, ns);
    const int n = ns[0] + ns[1] + ns[2] + ns[3];
    const int SS = S * S, half = S >> 1;
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        int i = j, k = 0;
        if (segs) { seg_locate(ns, segs, j, k, i); i += k * seg_cap; }      // (shapes form: the patch's slot)
        int l, b, y, x;
        decode_pixel(L, list[i], l, b, y, x);
        if (y - half >= 0 && y + half < L.h[l] && x - half >= 0 && x + half < L.w[l]) continue;
        const int work = SS * rows * 4;
        for (int t = threadIdx.x; t < work; t += 256) {
            const int chunk = t & 3, r = (t >> 2) % rows, q = (t >> 2) / rows;
            const int yy = y + q / S - half, xx = x + q % S - half;
            if ((unsigned)yy < (unsigned)L.h[l] && (unsigned)xx < (unsigned)L.w[l]) continue;
            *reinterpret_cast<uint4*>(planes + ((int64_t)r * np + (int64_t)i * SS + q) * 64 + chunk * 16) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// ---- assembly ---------------------------------------------------------------------------------------------------------------------------
struct AsmArgs {
    const float* cls[4];       // per kernel shape: class logits [pixels][cls_ld]
    const float* small[4];     // per kernel shape: [rows][small_ld], centerness + bbox at column 0, mask coefficients at column gpad
    const float* trk[4];       // per kernel shape: [rows][trk_ld]
    float *conf, *loc, *mask, *track, *cen;
    int B, K, n_levels, n_cls, mask_dim, embed, gpad, cls_ld, small_ld, trk_ld, N;
    int lvl_start[9], lvl_hw[8], lvl_off[8];
    int vec4;
    int row_mul, row_add;      // sparse form: source row of listed position i = i * row_mul + row_add (the centre pixel of its output-layer patch)
    const int* list;
    const int* ctl;
    int capacity;
    int split;                 // list entries from ctl[CTL_OWN + CTL_N] on are partner-only positions: centerness and loc only
    int segs;                  // shapes form: K segments of `capacity` (pixel, shape) entries (0: a list of pixels)
};

// the tail of head_assemble_kernel (mask_ops.hip) for one (image, prior) row, 16 lanes per row: same expressions, same summation order
__device__ __forceinline__ void assemble_rest(const AsmArgs& a, const float* sm, const float* tk, int64_t o, int64_t cen_idx, int sub)
{
    if (sub < 4) a.loc[o * 4 + sub] = sm[1 + sub];
    for (int c = sub; c < a.mask_dim; c += 16) a.mask[o * a.mask_dim + c] = sm[a.gpad + c];
    if (sub == 0) a.cen[cen_idx] = tanhf(sm[0]);
    float ss = 0.0f;
    if (a.vec4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4 v[4];
        const int nv = a.embed >> 2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c4 = sub + 16 * q;
            if (c4 < nv) {
                v[q] = *reinterpret_cast<const f4*>(tk + 4 * c4);
                ss = fmaf(v[q].x, v[q].x, ss); ss = fmaf(v[q].y, v[q].y, ss); ss = fmaf(v[q].z, v[q].z, ss); ss = fmaf(v[q].w, v[q].w, ss);
            }
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) ss += __shfl_xor(ss, d);
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c4 = sub + 16 * q;
            if (c4 < nv) *reinterpret_cast<f4*>(a.track + o * a.embed + 4 * c4) = v[q] * inv;
        }
    } else {
        for (int c = sub; c < a.embed; c += 16) { const float v = tk[c]; ss = fmaf(v, v, ss); }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) ss += __shfl_xor(ss, d);
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        for (int c = sub; c < a.embed; c += 16) a.track[o * a.embed + c] = tk[c] * inv;
    }
}

// MODE 0: conf of every (image, prior) row.  MODE 1: the four other tensors of every row from dense matrices, only after an overflow.
template <int MODE>
__global__ __launch_bounds__(256) void head_assemble_rows_kernel(const AsmArgs a)
{
    if (MODE == 1 && a.ctl[CTL_OVERFLOW] == 0) return;
    const int sub = threadIdx.x & 15;
    const int64_t row = (int64_t)stm_xcd_block(((int64_t)a.B * a.N + 15) >> 4) * 16 + (threadIdx.x >> 4);
    if (row < 0 || row >= (int64_t)a.B * a.N) return;
    const int b = (int)(row / a.N), n = (int)(row - (int64_t)b * a.N);
    int l = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
        if (i < a.n_levels && n >= a.lvl_off[i]) l = i;
    const int r = n - a.lvl_off[l];
    const int p = r / a.K, k = r - p * a.K;
    const int hw = a.lvl_hw[l];
    const int64_t src = (int64_t)a.lvl_start[l] + (int64_t)b * hw + p;
    const int64_t o = (int64_t)b * a.N + n;
    if (MODE == 0) {
        const float* cl = a.cls[k] + src * a.cls_ld;
        for (int c = sub; c < a.n_cls; c += 16) a.conf[o * a.n_cls + c] = cl[c];
    } else {
        assemble_rest(a, a.small[k] + src * a.small_ld, a.trk[k] + src * a.trk_ld, o, (int64_t)b * a.N + a.lvl_off[l] + (int64_t)k * hw + p, sub);
    }
}

// the four other tensors at the K rows of every listed position
__global__ __launch_bounds__(256) void head_assemble_listed_kernel(const AsmArgs a)
{
    const int n_pos = a.ctl[CTL_N];
    int n_own = a.split ? a.ctl[CTL_OWN + CTL_N] : n_pos;
    const int sub = threadIdx.x & 15;
    // shapes form: one unit per entry -- entry i of segment k is kernel shape k at pixel list[k capacity + i], row i of small[k] / trk[k]
    int ns[4] = {0, 0, 0, 0};
    if (a.segs) seg_counts(a.ctl, a.segs, CTL_N, ns);
    const int64_t units = a.segs ? n_pos : (int64_t)n_pos * a.K;
    for (int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); u < units; u += (int64_t)gridDim.x * 16) {
        int i = (int)(u / a.K), k = (int)(u - (int64_t)i * a.K);
        int slot = i;
        if (a.segs) {
            seg_locate(ns, a.segs, (int)u, k, i);
            n_own = a.ctl[CTL_SEG * (k + 1) + CTL_OWN + CTL_N];
            slot = k * a.capacity + i;
        }
        const int m = a.list[slot];
        int l = 0;
#pragma unroll
        for (int j = 1; j < 8; ++j)
            if (j < a.n_levels && m >= a.lvl_start[j]) l = j;
        const int hw = a.lvl_hw[l];
        const int rr = m - a.lvl_start[l];
        const int b = rr / hw, p = rr - b * hw;
        const int nn = a.lvl_off[l] + p * a.K + k;
        const int64_t o = (int64_t)b * a.N + nn;
        const int64_t src = (int64_t)i * a.row_mul + a.row_add;
        const int64_t cen_idx = (int64_t)b * a.N + a.lvl_off[l] + (int64_t)k * hw + p;
        if (i >= n_own) {
            // partner-only position: the mask and track branches did not run here -- the centerness + bbox columns only
            const float* sm = a.small[k] + src * a.small_ld;
            if (sub < 4) a.loc[o * 4 + sub] = sm[1 + sub];
            if (sub == 0) a.cen[cen_idx] = tanhf(sm[0]);
            continue;
        }
        assemble_rest(a, a.small[k] + src * a.small_ld, a.trk[k] + src * a.trk_ld, o, cen_idx, sub);
    }
}

bool fill_levels(Levels& L, int n_levels, int B, const int* lvl_start, const int* lvl_h, const int* lvl_w)
{
    if (n_levels <= 0 || n_levels > 8 || B <= 0 || !lvl_start || !lvl_h || !lvl_w || lvl_start[0] != 0) return false;
    L.n = n_levels; L.B = B;
    for (int l = 0; l < 8; ++l) {
        L.start[l] = l < n_levels ? lvl_start[l] : 0;
        L.h[l] = l < n_levels ? lvl_h[l] : 1;
        L.w[l] = l < n_levels ? lvl_w[l] : 1;
        if (l < n_levels && (lvl_h[l] <= 0 || lvl_w[l] <= 0 || lvl_start[l + 1] - lvl_start[l] != B * lvl_h[l] * lvl_w[l])) return false;
    }
    L.start[8] = 0;
    L.start[n_levels] = lvl_start[n_levels];
    return true;
}

}  // namespace

extern "C" int stm_head_candidates_f32(const float* const* cls_logits, int K, int ld, int n_cls, float conf_thresh, int capacity,
                                       int patch_pixels_a, int patch_pixels_b, int n_levels, int B, const int* lvl_start, const int* lvl_h,
                                       const int* lvl_w, int* flags, int* list, int* ctl, stm_stream_t stream)
{
    const char* who = "stm_head_candidates_f32";
    STM_REQUIRE(cls_logits && list && ctl && flags, STM_ENULL, "%s: NULL argument", who);
    CandArgs a;
    STM_REQUIRE(fill_levels(a.L, n_levels, B, lvl_start, lvl_h, lvl_w), STM_EINVAL, "%s: bad level table", who);
    const int n_pixels = a.L.start[n_levels];
    // a negative capacity selects the split form: |capacity| positions, own positions in front, 16 control ints, n_pixels + 2 flag ints
    int split = capacity < 0;
    STM_REQUIRE(capacity != INT_MIN, STM_EINVAL, "%s: bad sizes", who);
    if (split) capacity = -capacity;
    // ... and K << 28 added to it the shapes form: (pixel, shape) entries in K segments of that many each, 16 (K + 1) control ints, n_pixels + 2 K flag ints
    const int segs = capacity >> SEG_SHIFT;
    if (segs) {
        STM_REQUIRE(split && segs == K && K <= 3, STM_EINVAL, "%s: the shapes form takes a negative capacity with K << 28 added, K <= 3", who);
        capacity &= SEG_CAP_MASK;
        split = 2;
        // (patch_pixels_a / _b: segment k's pixel count in bits [8 k, 8 k + 8) -- the pixels of shape k's window of the two tower layers)
        for (int k = 0; k < K; ++k)
            STM_REQUIRE((patch_pixels_a >> 8 * k & 255) > 0 && (patch_pixels_b >> 8 * k & 255) > 0, STM_EINVAL, "%s: segment %d has no patch pixels", who, k);
        STM_REQUIRE((int64_t)capacity * 255 < ((int64_t)1 << 30), STM_EINVAL, "%s: bad sizes", who);
    }
    STM_REQUIRE(K > 0 && K <= 4 && n_cls >= 2 && ld >= n_cls && n_pixels > 0 && capacity > 0 && patch_pixels_a > 0 && patch_pixels_b > 0 &&
                    (segs || (int64_t)capacity * std::max(patch_pixels_a, patch_pixels_b) < ((int64_t)1 << 30)), STM_EINVAL, "%s: bad sizes", who);
    for (int k = 0; k < 4; ++k) {
        a.cls[k] = k < K ? cls_logits[k] : nullptr;
        STM_REQUIRE(k >= K || a.cls[k], STM_ENULL, "%s: input %d is NULL", who, k);
    }
    a.K = K; a.ld = ld; a.n_cls = n_cls; a.n_pixels = n_pixels; a.capacity = capacity; a.thresh = conf_thresh; a.list = list; a.ctl = ctl;
    a.flags = flags; a.split = split;
    const int n_flags = n_pixels + (segs ? 2 * K : split ? 2 : 0), n_ctl = segs ? CTL_SEG * (K + 1) : split ? 2 * CTL_INTS : CTL_INTS;
    // (cleared by a kernel, not by memset nodes: the launches are captured into a graph that is replayed many times)
    hipLaunchKernelGGL(head_clear_kernel, dim3(stm_cdiv(n_flags + n_ctl, 256)), dim3(256), 0, stm_hs(stream), ctl, flags, n_flags, n_ctl);
    STM_CHECK_LAUNCH("head_clear_kernel");
    int vec = ld % 4 == 0 && 4 * ((n_cls + 3) / 4) <= ld;
    for (int k = 0; k < K; ++k) vec = vec && ((uintptr_t)a.cls[k] % 16) == 0;
    const size_t lds = (size_t)K * CAND_PX * (n_cls | 1) * sizeof(float);
    STM_REQUIRE(lds <= 48 * 1024, STM_EUNSUPPORTED, "%s: %d classes x %d shapes do not fit the staging buffer", who, n_cls, K);
    hipLaunchKernelGGL(head_candidates_kernel, dim3(stm_cdiv(n_pixels, CAND_PX)), dim3(256), lds, stm_hs(stream), a, vec);
    STM_CHECK_LAUNCH("head_candidates_kernel");
    if (segs) {
        hipLaunchKernelGGL(head_control_segs_kernel, dim3(1), dim3(64), 0, stm_hs(stream), ctl, K, capacity, n_pixels, patch_pixels_a, patch_pixels_b);
        STM_CHECK_LAUNCH("head_control_segs_kernel");
        hipLaunchKernelGGL(head_list_segs_kernel, dim3(stm_cdiv(n_pixels, 256)), dim3(256), 0, stm_hs(stream), flags, flags + n_pixels, n_pixels, K, capacity, list, ctl);
        STM_CHECK_LAUNCH("head_list_segs_kernel");
        return STM_OK;
    }
    hipLaunchKernelGGL(head_control_kernel, dim3(1), dim3(64), 0, stm_hs(stream), ctl, capacity, n_pixels, patch_pixels_a, patch_pixels_b,
                       split ? 2 : 1);
    STM_CHECK_LAUNCH("head_control_kernel");
    if (split) {
        hipLaunchKernelGGL(head_list_kernel, dim3(stm_cdiv(n_pixels, 256)), dim3(256), 0, stm_hs(stream), flags, flags + n_pixels, n_pixels, capacity, list, ctl);
        STM_CHECK_LAUNCH("head_list_kernel");
    }
    return STM_OK;
}

extern "C" int stm_head_patch_gather(const void* src_planes, long long src_np, void* dst_planes, int side, int n_planes, int slabs,
                                     int capacity, int n_levels, int B, const int* lvl_start, const int* lvl_h, const int* lvl_w, const int* list,
                                     const int* ctl, stm_stream_t stream)
{
    const char* who = "stm_head_patch_gather";
    STM_REQUIRE(src_planes && dst_planes && list && ctl, STM_ENULL, "%s: NULL argument", who);
    // (shapes form: segments << 28 added to the capacity, which then counts the patches of ONE segment)
    const int segs = capacity > 0 ? capacity >> SEG_SHIFT : 0;
    STM_REQUIRE(segs <= 4, STM_EINVAL, "%s: at most 4 segments", who);
    const int seg_cap = capacity & SEG_CAP_MASK;
    if (segs) capacity = segs * seg_cap;
    STM_REQUIRE(n_planes > 0 && slabs > 0 && capacity > 0 && side > 0 && (side & 1) && src_np > 0 &&
                    (uintptr_t)src_planes % 16 == 0 && (uintptr_t)dst_planes % 16 == 0, STM_EINVAL, "%s: bad sizes or alignment", who);
    GatherArgs a;
    STM_REQUIRE(fill_levels(a.L, n_levels, B, lvl_start, lvl_h, lvl_w), STM_EINVAL, "%s: bad level table", who);
    STM_REQUIRE(src_np >= a.L.start[n_levels], STM_EINVAL, "%s: the source planes hold fewer pixels than the levels", who);
    a.src = static_cast<const uint8_t*>(src_planes); a.dst = static_cast<uint8_t*>(dst_planes);
    a.rows = n_planes * slabs; a.src_np = src_np; a.dst_np = (int64_t)capacity * side * side; a.S = side;
    a.list = list; a.ctl = ctl; a.segs = segs; a.seg_cap = seg_cap;
    const int64_t units = (int64_t)capacity * side * side * ((a.rows + 15) / 16);
    const unsigned grid = (unsigned)std::min<int64_t>((units + 3) / 4, 16384);
    hipLaunchKernelGGL(head_patch_gather_kernel, dim3(grid), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("head_patch_gather_kernel");
    return STM_OK;
}

extern "C" int stm_head_patch_mask(void* planes, int side, int n_planes, int slabs, int capacity, int n_levels, int B, const int* lvl_start,
                                   const int* lvl_h, const int* lvl_w, const int* list, const int* ctl, stm_stream_t stream)
{
    const char* who = "stm_head_patch_mask";
    STM_REQUIRE(planes && list && ctl, STM_ENULL, "%s: NULL argument", who);
    const int segs = capacity > 0 ? capacity >> SEG_SHIFT : 0;      // (shapes form, as stm_head_patch_gather)
    STM_REQUIRE(segs <= 4, STM_EINVAL, "%s: at most 4 segments", who);
    const int seg_cap = capacity & SEG_CAP_MASK;
    if (segs) capacity = segs * seg_cap;
    STM_REQUIRE(n_planes > 0 && slabs > 0 && capacity > 0 && side > 0 && (side & 1) && (uintptr_t)planes % 16 == 0, STM_EINVAL, "%s: bad sizes or alignment", who);
    Levels L;
    STM_REQUIRE(fill_levels(L, n_levels, B, lvl_start, lvl_h, lvl_w), STM_EINVAL, "%s: bad level table", who);
    hipLaunchKernelGGL(head_patch_mask_kernel, dim3(std::min(capacity, 2048)), dim3(256), 0, stm_hs(stream), static_cast<uint8_t*>(planes), n_planes * slabs,
                       (int64_t)capacity * side * side, side, list, ctl, L, segs, seg_cap);
    STM_CHECK_LAUNCH("head_patch_mask_kernel");
    return STM_OK;
}

extern "C" int stm_head_assemble_sparse_f32(const float* const* cls_logits, int cls_ld, const float* const* small, const float* const* trk,
                                            const float* const* small_dense, const float* const* trk_dense, const stm_head_layout* L,
                                            int row_mul, int row_add, const int* list, const int* ctl, int capacity, float* conf, float* loc,
                                            float* mask, float* track, float* centerness, stm_stream_t stream)
{
    const char* who = "stm_head_assemble_sparse_f32";
    STM_REQUIRE(cls_logits && small && trk && small_dense && trk_dense && L && list && ctl && conf && loc && mask && track && centerness, STM_ENULL,
                "%s: NULL argument", who);
    STM_REQUIRE(L->B > 0 && L->K > 0 && L->K <= 4 && L->n_levels > 0 && L->n_levels <= 8 && L->n_cls > 0 && cls_ld >= L->n_cls && L->mask_dim > 0 &&
                    L->mask_dim <= L->group_pad && L->embed_dim > 0 && L->group_pad >= 5 && L->small_ld >= L->group_pad + L->mask_dim &&
                    L->trk_ld >= L->embed_dim && capacity != 0 && capacity != INT_MIN && row_mul > 0 && row_add >= 0 && row_add < row_mul, STM_EINVAL, "%s: bad layout", who);
    AsmArgs a;
    a.conf = conf; a.loc = loc; a.mask = mask; a.track = track; a.cen = centerness;
    a.B = L->B; a.K = L->K; a.n_levels = L->n_levels; a.n_cls = L->n_cls; a.mask_dim = L->mask_dim; a.embed = L->embed_dim;
    a.gpad = L->group_pad; a.cls_ld = cls_ld; a.small_ld = L->small_ld; a.trk_ld = L->trk_ld;
    // (a negative capacity: the split form of stm_head_candidates_f32 -- ordered list, 16 control ints)
    a.split = capacity < 0;
    if (a.split) capacity = -capacity;
    // (... with K << 28 added: the shapes form -- small[k] / trk[k] hold one row per entry of segment k)
    a.segs = capacity >> SEG_SHIFT;
    STM_REQUIRE(!a.segs || (a.split && a.segs == L->K), STM_EINVAL, "%s: the shapes form takes a negative capacity with K << 28 added", who);
    capacity &= SEG_CAP_MASK;
    STM_REQUIRE(capacity > 0, STM_EINVAL, "%s: bad capacity", who);
    a.row_mul = row_mul; a.row_add = row_add; a.list = list; a.ctl = ctl; a.capacity = capacity;
    int off = 0, start = 0;
    for (int l = 0; l < 8; ++l) {
        a.lvl_start[l] = l < L->n_levels ? L->lvl_start[l] : 0;
        a.lvl_hw[l] = l < L->n_levels ? L->lvl_hw[l] : 1;
        a.lvl_off[l] = off;
        if (l < L->n_levels) {
            STM_REQUIRE(L->lvl_hw[l] > 0 && L->lvl_start[l] == start, STM_EINVAL, "%s: level %d: bad pixel range", who, l);
            off += L->lvl_hw[l] * L->K;
            start += L->B * L->lvl_hw[l];
        }
    }
    a.lvl_start[8] = 0;
    a.N = off;
    const int64_t rows = (int64_t)a.B * a.N;
    const bool al = a.embed % 4 == 0 && a.embed <= 256 && a.trk_ld % 4 == 0 && ((uintptr_t)track % 16) == 0;
    auto set = [&](const float* const* sm, const float* const* tk) -> bool {
        a.vec4 = al;
        for (int k = 0; k < 4; ++k) {
            a.cls[k] = k < a.K ? cls_logits[k] : nullptr;
            a.small[k] = k < a.K ? sm[k] : nullptr;
            a.trk[k] = k < a.K ? tk[k] : nullptr;
            if (k < a.K && !(a.cls[k] && a.small[k] && a.trk[k])) return false;
            if (k < a.K) a.vec4 = a.vec4 && ((uintptr_t)a.trk[k] % 16) == 0;
        }
        return true;
    };
    STM_REQUIRE(set(small, trk), STM_ENULL, "%s: an input matrix is NULL", who);
    hipLaunchKernelGGL(head_assemble_rows_kernel<0>, dim3(stm_xcd_grid(stm_cdiv(rows, 16))), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("head_assemble_rows_kernel<0>");
    hipLaunchKernelGGL(head_assemble_listed_kernel, dim3((unsigned)std::min<int64_t>(stm_cdiv((int64_t)capacity * a.K, 16), 4096)), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("head_assemble_listed_kernel");
    STM_REQUIRE(set(small_dense, trk_dense), STM_ENULL, "%s: a dense input matrix is NULL", who);
    hipLaunchKernelGGL(head_assemble_rows_kernel<1>, dim3(stm_xcd_grid(stm_cdiv(rows, 16))), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("head_assemble_rows_kernel<1>");
    return STM_OK;
}
