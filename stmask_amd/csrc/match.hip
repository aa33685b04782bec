// match.hip -- training target assignment on the device: layers.box_utils.match (box_utils.py:119-197) and encode (:200-235), fp32, gfx950.
//
// Three launches for a whole batch, whatever the number of boxes or images:
//   match_overlap_kernel   (prior tile, image): the image's boxes sit in LDS, one prior per thread.  Writes the [G][P] overlaps to the workspace,
//                          the per-prior best value / first-maximum index with the multi-instance rule applied, and the classification term
//                          cla = 2 / (1 + exp(cross_entropy)) already added to the priors that pass `best > pos`.
//   match_forced_kernel    one workgroup per image: mean(cla) in a fixed order -> pos', neg'; the row maxima once (a wave per row); G serial
//                          picks with a removed-column bitmask in LDS, re-scanning only the rows whose cached maximum sat in the removed column.
//   match_finalise_kernel  (prior tile, image): thresholds, labels, ids, encode, vector stores.
// No float atomics; every sum and every arg-max has one order (first index wins a tie, as the reference's CPU max does), so outputs are
// bit-identical run to run.  Compiled with -ffp-contract=off: the overlaps, point_form and columns 0-1 of encode are the reference's IEEE
// add / sub / mul / div in its operand order.  The log of encode's columns 2-3 and the exp / log of the cross entropy are evaluated in double
// and rounded once.
#include "stm_common.h"

#include <limits.h>

namespace {

constexpr int MT_TILE = 256;
constexpr int MT_GMAX = 128;              // boxes per image
constexpr int MT_CMAX = 128;              // classes
constexpr int FM_THREADS = 1024;
constexpr int FM_WAVES = FM_THREADS / STM_WAVE;
constexpr int FM_MASK_WORDS = 8192;       // removed-column bitmask: P <= 262144
constexpr int MT_PMAX = FM_MASK_WORDS * 32;

enum { MT_ST_BAD_RANGE = 1, MT_ST_BAD_BOX = 2, MT_ST_NO_COLUMN = 4 };

struct MatchWs {
    float* ov;    // [G_total][ldp]
    float* bo;    // [B][P]   best overlap (after the multi-instance rule, + cla, then 2 at forced priors)
    int* bi;      // [B][P]   best box
    float* cla;   // [B][P]   cla of the kept priors, -1 elsewhere
    float* thr;   // [B][2]   pos', neg'
};

__host__ __device__ inline int64_t mt_ldp(int P) { return ((int64_t)P + 3) & ~(int64_t)3; }

size_t mt_ws_bytes(int B, int P, int G_total)
{
    return ((size_t)G_total * (size_t)mt_ldp(P) + 3 * (size_t)B * (size_t)P + 2 * (size_t)B) * 4 + 16;
}

MatchWs mt_carve(void* ws, int B, int P, int G_total)
{
    MatchWs w;
    w.ov = reinterpret_cast<float*>(ws);
    w.bo = w.ov + (size_t)G_total * (size_t)mt_ldp(P);
    w.bi = reinterpret_cast<int*>(w.bo + (size_t)B * P);
    w.cla = reinterpret_cast<float*>(w.bi + (size_t)B * P);
    w.thr = w.cla + (size_t)B * P;
    return w;
}

// Rows [g0, g0 + G) of image b, whatever the offsets hold: never outside [0, G_total), never more than g_max rows.
__device__ __forceinline__ bool mt_image_range(const int* __restrict__ offs, int b, int G_total, int g_max, int& g0, int& G)
{
    const int lo = offs[b], hi = offs[b + 1];
    const bool ok = lo >= 0 && hi > lo && hi <= G_total && hi - lo <= g_max;
    g0 = ok ? lo : 0;
    G = ok ? hi - lo : 0;
    return ok;
}

__global__ __launch_bounds__(MT_TILE) void match_overlap_kernel(const float4* __restrict__ boxes, const int64_t* __restrict__ labels,
                                                                const int* __restrict__ offs, int G_total, int g_max,
                                                                const float4* __restrict__ priors, int64_t prior_bstride, const float* __restrict__ conf,
                                                                int P, int C, float thr_multi, float mid, float posf, MatchWs w)
{
    __shared__ float4 s_box[MT_GMAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    int g0, G;
    mt_image_range(offs, b, G_total, g_max, g0, G);
    for (int g = tid; g < G; g += MT_TILE) s_box[g] = boxes[g0 + g];
    __syncthreads();
    const int p = blockIdx.x * MT_TILE + tid;
    if (p >= P) return;
    const int64_t bp = (int64_t)b * P + p;
    if (G == 0) {
        w.bo[bp] = 0.0f;
        w.bi[bp] = 0;
        w.cla[bp] = -1.0f;
        return;
    }
    const float4 pr = priors[(int64_t)b * prior_bstride + p];
    float4 pf;                                        // point_form (box_utils.py:20-21)
    pf.x = pr.x - pr.z / 2.0f;
    pf.y = pr.y - pr.w / 2.0f;
    pf.z = pr.x + pr.z / 2.0f;
    pf.w = pr.y + pr.w / 2.0f;
    const int64_t ldp = mt_ldp(P);
    float* __restrict__ ov = w.ov + (int64_t)g0 * ldp + p;
    float best = stm_iou(s_box[0], pf);
    int bidx = 0, many = best > thr_multi ? 1 : 0;
    ov[0] = best;
    for (int g = 1; g < G; ++g) {
        const float v = stm_iou(s_box[g], pf);
        ov[(int64_t)g * ldp] = v;
        if (v > best) {                               // strict: the first maximum keeps its index
            best = v;
            bidx = g;
        }
        many += v > thr_multi ? 1 : 0;
    }
    if (many > 1) best = mid;
    float cla = -1.0f;
    if (best > posf) {
        const float* __restrict__ row = conf + bp * C;
        int64_t lab = labels[g0 + bidx];
        lab = lab < 0 ? 0 : (lab >= C ? C - 1 : lab);
        float m = row[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += exp((double)row[c] - (double)m);
        const double ce = log(s) - ((double)row[lab] - (double)m);
        cla = (float)(2.0 / (1.0 + exp(ce)));
        best = best + cla;
    }
    w.bo[bp] = best;
    w.bi[bp] = bidx;
    w.cla[bp] = cla;
}

// (value, index) arg-max merge: the larger value wins, equal values keep the lower index
__device__ __forceinline__ void mt_argmax_merge(float& v, int& i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ __forceinline__ void mt_wave_argmax(float& v, int& i)
{
#pragma unroll
    for (int s = 1; s < STM_WAVE; s <<= 1) {
        const float ov = __shfl_xor(v, s, STM_WAVE);
        const int oi = __shfl_xor(i, s, STM_WAVE);
        mt_argmax_merge(v, i, ov, oi);
    }
}

// First maximum of one overlap row over the columns not yet removed (a wave; every lane returns the result).  No live column, or
// only NaNs: (-inf, INT_MAX).
__device__ __forceinline__ void mt_scan_row(const float* __restrict__ row, int P, const unsigned* removed, int lane, float& v, int& idx)
{
    v = -__builtin_huge_valf();
    idx = INT_MAX;
    const float4* __restrict__ row4 = reinterpret_cast<const float4*>(row);
    const int n4 = (P + 3) >> 2;
    for (int q = lane; q < n4; q += STM_WAVE) {
        const float4 x = row4[q];
        const int p0 = q * 4;
        const unsigned bits = removed[p0 >> 5] >> (p0 & 31);
        const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < P && !((bits >> k) & 1u) && xs[k] > v) {
                v = xs[k];
                idx = p0 + k;
            }
    }
    mt_wave_argmax(v, idx);
}

__global__ __launch_bounds__(FM_THREADS) void match_forced_kernel(const float4* __restrict__ boxes, const int* __restrict__ offs, int G_total,
                                                                  int g_max, int P, float posf, float negf, MatchWs w, int* __restrict__ status)
{
    __shared__ unsigned s_removed[FM_MASK_WORDS];
    __shared__ float s_rowmax[MT_GMAX];
    __shared__ int s_rowarg[MT_GMAX];
    __shared__ double s_sum[FM_THREADS];
    __shared__ int s_cnt[FM_THREADS];
    __shared__ int s_pick[2];
    __shared__ int s_status;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (STM_WAVE - 1), wave = tid / STM_WAVE;
    int g0, G;
    const bool range_ok = mt_image_range(offs, b, G_total, g_max, g0, G);
    if (tid == 0) s_status = range_ok ? 0 : MT_ST_BAD_RANGE;
    const int words = (P + 31) >> 5;
    for (int i = tid; i < words; i += FM_THREADS) s_removed[i] = 0u;
    __syncthreads();
    for (int g = tid; g < G; g += FM_THREADS) {
        const float4 bx = boxes[g0 + g];
        if (!(bx.z > bx.x && bx.w > bx.y)) s_status = MT_ST_BAD_BOX;        // (same value from every writer)
    }

    // mean(cla) over the kept priors: a strided partial sum per thread, then a tree, both in one fixed order
    const float* __restrict__ cla = w.cla + (int64_t)b * P;
    double acc = 0.0;
    int cnt = 0;
    for (int p = tid; p < P; p += FM_THREADS) {
        const float c = cla[p];
        if (c >= 0.0f) {
            acc += (double)c;
            ++cnt;
        }
    }
    s_sum[tid] = acc;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int s = FM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_sum[tid] += s_sum[tid + s];
            s_cnt[tid] += s_cnt[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        float pos2 = posf, neg2 = negf;
        if (s_cnt[0] > 0) {
            const float mean = (float)(s_sum[0] / (double)s_cnt[0]);
            pos2 = posf + mean;
            neg2 = negf + mean;
        }
        w.thr[2 * b] = pos2;
        w.thr[2 * b + 1] = neg2;
    }

    // row maxima, a wave per row
    const int64_t ldp = mt_ldp(P);
    const float* __restrict__ ov = w.ov + (int64_t)g0 * ldp;
    for (int g = wave; g < G; g += FM_WAVES) {
        float v;
        int idx;
        mt_scan_row(ov + (int64_t)g * ldp, P, s_removed, lane, v, idx);
        if (lane == 0) {
            s_rowmax[g] = v;
            s_rowarg[g] = idx;
        }
    }
    __syncthreads();

    float* __restrict__ bo = w.bo + (int64_t)b * P;
    int* __restrict__ bi = w.bi + (int64_t)b * P;
    for (int it = 0; it < G; ++it) {
        // j: the live row with the largest maximum (first such row); i: its first-maximum column.  A used row has arg -1.
        if (wave == 0) {
            float v = -__builtin_huge_valf();
            int j = INT_MAX;
            for (int g = lane; g < G; g += STM_WAVE)
                if (s_rowarg[g] >= 0) mt_argmax_merge(v, j, s_rowmax[g], s_rowarg[g] == INT_MAX ? INT_MAX : g);
            mt_wave_argmax(v, j);
            if (lane == 0) {
                int i = -1;
                if (j != INT_MAX) {
                    i = s_rowarg[j];
                    s_rowarg[j] = -1;
                    s_removed[i >> 5] |= 1u << (i & 31);
                    bo[i] = 2.0f;
                    bi[i] = j;
                } else {
                    s_status = MT_ST_NO_COLUMN;       // only NaN overlaps are left: nothing more to force
                }
                s_pick[0] = j;
                s_pick[1] = i;
            }
        }
        __syncthreads();
        const int j = s_pick[0], i = s_pick[1];
        if (j == INT_MAX) break;
        for (int g = wave; g < G; g += FM_WAVES) {
            if (s_rowarg[g] != i) continue;            // (wave-uniform; used rows hold -1, i >= 0)
            float v;
            int idx;
            mt_scan_row(ov + (int64_t)g * ldp, P, s_removed, lane, v, idx);
            if (lane == 0) {
                s_rowmax[g] = v;
                s_rowarg[g] = idx;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0 && status) status[b] = s_status;
}

__global__ __launch_bounds__(MT_TILE) void match_finalise_kernel(const float4* __restrict__ boxes, const int64_t* __restrict__ labels,
                                                                 const int64_t* __restrict__ ids, const int* __restrict__ offs, int G_total,
                                                                 int g_max, const float4* __restrict__ priors, int64_t prior_bstride, int P, MatchWs w,
                                                                 float4* __restrict__ loc_t, float4* __restrict__ gt_boxes_t,
                                                                 int64_t* __restrict__ conf_t, int64_t* __restrict__ idx_t, int64_t* __restrict__ ids_t)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * MT_TILE + threadIdx.x;
    if (p >= P) return;
    int g0, G;
    mt_image_range(offs, b, G_total, g_max, g0, G);
    const int64_t bp = (int64_t)b * P + p;
    if (G == 0) {
        loc_t[bp] = make_float4(0.f, 0.f, 0.f, 0.f);
        gt_boxes_t[bp] = make_float4(0.f, 0.f, 0.f, 0.f);
        conf_t[bp] = 0;
        idx_t[bp] = 0;
        ids_t[bp] = 0;
        return;
    }
    const float pos2 = w.thr[2 * b], neg2 = w.thr[2 * b + 1];
    const float best = w.bo[bp];
    const int g = w.bi[bp];
    const float4 m = boxes[g0 + g];
    int64_t c = labels[g0 + g], id = ids[g0 + g];
    if (best < pos2) {
        c = -1;
        id = 0;
    }
    if (best < neg2) c = 0;
    loc_t[bp] = stm_encode_one(m, priors[(int64_t)b * prior_bstride + p]);
    gt_boxes_t[bp] = m;
    conf_t[bp] = c;
    idx_t[bp] = g;
    ids_t[bp] = id;
}

__global__ __launch_bounds__(256) void encode_kernel(const float4* __restrict__ matched, const float4* __restrict__ priors, float4* __restrict__ out,
                                                     int64_t n)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = stm_encode_one(matched[t], priors[t]);
}


}  // namespace

extern "C" size_t stm_match_workspace_bytes(int B, int P, int G_total, int G_max)
{
    if (B <= 0 || P <= 0 || G_total <= 0 || G_max <= 0) return 0;
    return mt_ws_bytes(B, P, G_total);
}

extern "C" int stm_match_priors_f32(const float* boxes, const int64_t* labels, const int64_t* ids, const int* offsets, int B, int G_total,
                                    int G_max, const float* priors, int priors_batched, int P, const float* conf, int C, double pos_thresh,
                                    double neg_thresh, float* loc_t, float* gt_boxes_t, int64_t* conf_t, int64_t* idx_t, int64_t* ids_t,
                                    int* status, void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    STM_REQUIRE(B > 0 && P > 0 && C > 0, STM_EINVAL, "stm_match_priors_f32: B=%d P=%d C=%d", B, P, C);
    STM_REQUIRE(G_total >= B && G_max >= 1, STM_EINVAL,
                "stm_match_priors_f32: G_total=%d G_max=%d for B=%d: every image needs at least one ground-truth box", G_total, G_max, B);
    STM_REQUIRE(G_max <= G_total && (int64_t)G_max * B >= G_total, STM_EINVAL, "stm_match_priors_f32: G_max=%d does not fit G_total=%d, B=%d",
                G_max, G_total, B);
    STM_REQUIRE(G_max <= P, STM_EINVAL, "stm_match_priors_f32: %d boxes for %d priors (the forced matches need a prior per box)", G_max, P);
    STM_REQUIRE(G_max <= MT_GMAX, STM_EUNSUPPORTED, "stm_match_priors_f32: %d boxes in one image (limit %d)", G_max, MT_GMAX);
    STM_REQUIRE(C >= 2 && C <= MT_CMAX, STM_EUNSUPPORTED, "stm_match_priors_f32: %d classes (supported: 2..%d)", C, MT_CMAX);
    STM_REQUIRE(P <= MT_PMAX, STM_EUNSUPPORTED, "stm_match_priors_f32: %d priors (limit %d)", P, MT_PMAX);
    STM_REQUIRE(B <= 65535, STM_EUNSUPPORTED, "stm_match_priors_f32: B=%d (limit 65535)", B);
    STM_REQUIRE(boxes && labels && ids && offsets && priors && conf, STM_ENULL,
                "stm_match_priors_f32: boxes/labels/ids/offsets/priors/conf must be non-NULL");
    STM_REQUIRE(loc_t && gt_boxes_t && conf_t && idx_t && ids_t, STM_ENULL,
                "stm_match_priors_f32: loc_t/gt_boxes_t/conf_t/idx_t/ids_t must be non-NULL");
    STM_REQUIRE(stm_aligned16(boxes) && stm_aligned16(priors) && stm_aligned16(loc_t) && stm_aligned16(gt_boxes_t), STM_EINVAL,
                "stm_match_priors_f32: boxes, priors, loc_t and gt_boxes_t must be 16-byte aligned");
    const size_t need = mt_ws_bytes(B, P, G_total);
    STM_REQUIRE(workspace && workspace_bytes >= need && stm_aligned16(workspace), STM_EWORKSPACE,
                "stm_match_priors_f32: workspace of %zu bytes (16-byte aligned) needed, got %zu", need, workspace_bytes);
    const MatchWs w = mt_carve(workspace, B, P, G_total);
    const float4* b4 = reinterpret_cast<const float4*>(boxes);
    const float4* p4 = reinterpret_cast<const float4*>(priors);
    const int64_t pstride = priors_batched ? (int64_t)P : 0;
    // the reference compares fp32 tensors with Python floats: each constant is formed in double and rounded once
    const float posf = (float)pos_thresh, negf = (float)neg_thresh;
    const float thr_multi = (float)(pos_thresh - 0.1), mid = (float)((pos_thresh + neg_thresh) / 2);
    const dim3 grid(stm_cdiv(P, MT_TILE), B);
    hipLaunchKernelGGL(match_overlap_kernel, grid, dim3(MT_TILE), 0, stm_hs(stream), b4, labels, offsets, G_total, G_max, p4, pstride, conf, P, C,
                       thr_multi, mid, posf, w);
    STM_CHECK_LAUNCH("match_overlap_kernel");
    hipLaunchKernelGGL(match_forced_kernel, dim3(B), dim3(FM_THREADS), 0, stm_hs(stream), b4, offsets, G_total, G_max, P, posf, negf, w, status);
    STM_CHECK_LAUNCH("match_forced_kernel");
    hipLaunchKernelGGL(match_finalise_kernel, grid, dim3(MT_TILE), 0, stm_hs(stream), b4, labels, ids, offsets, G_total, G_max, p4, pstride, P, w,
                       reinterpret_cast<float4*>(loc_t), reinterpret_cast<float4*>(gt_boxes_t), conf_t, idx_t, ids_t);
    STM_CHECK_LAUNCH("match_finalise_kernel");
    return STM_OK;
}

extern "C" int stm_encode_boxes_f32(const float* matched, const float* priors, float* out, int64_t n, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0, STM_EINVAL, "stm_encode_boxes_f32: n=%lld", (long long)n);
    if (n == 0) return STM_OK;
    STM_REQUIRE(matched && priors && out, STM_ENULL, "stm_encode_boxes_f32: matched/priors/out must be non-NULL");
    STM_REQUIRE(stm_aligned16(matched) && stm_aligned16(priors) && stm_aligned16(out), STM_EINVAL,
                "stm_encode_boxes_f32: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(encode_kernel, dim3(stm_cdiv(n, 256)), dim3(256), 0, stm_hs(stream), reinterpret_cast<const float4*>(matched),
                       reinterpret_cast<const float4*>(priors), reinterpret_cast<float4*>(out), n);
    STM_CHECK_LAUNCH("encode_kernel");
    return STM_OK;
}
