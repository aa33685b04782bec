// t2s_loss.hip -- the reference's track_to_segment_loss (layers/modules/multibox_loss.py:247-326, called at :102-110), the loss that trains
// TemporalNet (losses['B_shift'] and losses['M_shift']), for gfx950: the target construction across the two frames of a clip, the batch-wide
// ordered list of shift-positive priors with everything the later stages gather through it, the two weighted reductions with their adjoint, and
// nothing else: RoIAlign, TemporalNet, the mask itself, the mask BCE and the mask's coefficient gradient (stm_lincomb_rows_backward_f32) are the
// existing kernels (temporal.hip, mask_ops.hip, mask_loss.hip, lincomb_backward.hip).  Conventions: include/stmask_hip.h.
//
// Prior p of clip i is shift-positive iff ids_t[i,p] > 0 and that id occurs among the clip's reference-frame ids AND its next-frame ids (int64
// equality).  Its regression target is encode(box_next(id), center_size(box_ref(id))) (stm_encode_one), its mask target the next frame's mask of
// that id.  A duplicate id resolves to the LAST reference index and the FIRST next index.  Every id and box value is data: nothing can fault.
//
// Tiles: a workgroup owns 256 consecutive priors of ONE clip, as in pos_loss.hip.
// stm_t2s_targets_f32 (3 launches):
//   1 targets   the clip's table over its G_ref <= 128 reference ids in LDS (thread j: the first next index with the same id or -1, and the
//               encoded 4-vector), then one thread per prior: a prior with ids_t <= 0 reads nothing else; the others walk the table from its end.
//               Writes pos_t, reg_t (exact zeros where not positive), idx_next (global row of the concatenated next-frame masks, -1 where not
//               positive) and the tile's count
//   2 scan      pos_index.h: the tiles' prefix, n, the [B + 1] prefix of the per-clip counts, the status word n > max_rows
//   3 index     pos_index.h: the ordered list of shift-positive rows and their weights 1 / n_i
// stm_t2s_gather_f32 (1 launch): 16 lanes per row of the list, n_rows rows with the live count in device memory: RoI (clip,
//   sanitize_coordinates_hw(decode(loc_ref, priors)): stm_decode_one and stm_roi_one, the expressions of stm_decode_boxes_f32 and
//   stm_shift_rois_f32), reg_t row, reference coefficients, next box, next mask row, clip, weight; rows past n are padding (weight 0, RoI
//   (0; 0, 0, 1, 1), box (0, 0, 1, 1), zero coefficients, target row 0).
// stm_t2s_reduce_f32 (1 launch, one workgroup): fp32 terms, weighted and added in double, thread t takes rows t, t + 256, ... whatever n_rows is,
//   so the padded and the exact form add the same numbers in the same order.  stm_t2s_reduce_backward_f32 (1 launch): one thread per row, written.
// No float atomics, no integer atomics, every grid depends on the shapes only, outputs are written, not accumulated.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no kernel of this file uses scratch.
#include "stm_common.h"
#include "pos_index.h"

namespace {

constexpr int TS_GMAX = 128;           // most boxes of one frame
constexpr int TS_LANES = 16;           // lanes per row of the gather
constexpr int TS_MAX_ROWS = 65535;     // rows of the list the later stages take (grid.y of the mask kernels: lincomb_backward.hip's LC_MAX_ROWS)

// rows [g0, g0 + G) of clip b's frame, whatever the offsets hold: never outside [0, G_total), never more than TS_GMAX rows
__device__ __forceinline__ void ts_frame_range(const int* __restrict__ offs, int b, int G_total, int& g0, int& G)
{
    const int lo = offs[b], hi = offs[b + 1];
    const bool ok = lo >= 0 && hi >= lo && hi <= G_total && hi - lo <= TS_GMAX;
    g0 = ok ? lo : 0;
    G = ok ? hi - lo : 0;
}

__global__ __launch_bounds__(256) void t2s_targets_kernel(const int64_t* __restrict__ ids_t, const float4* __restrict__ box_ref,
                                                          const int64_t* __restrict__ ids_ref, const int* __restrict__ offs_ref, int G_ref_total,
                                                          const float4* __restrict__ box_next, const int64_t* __restrict__ ids_next,
                                                          const int* __restrict__ offs_next, int G_next_total, int64_t* __restrict__ pos_t,
                                                          float4* __restrict__ reg_t, int64_t* __restrict__ idx_next,
                                                          unsigned* __restrict__ tilecnt, int P, int tpi)
{
    __shared__ int64_t s_id[TS_GMAX], s_idn[TS_GMAX];
    __shared__ float4 s_reg[TS_GMAX];
    __shared__ int s_k[TS_GMAX];                             // global next row, or -1
    __shared__ unsigned sc[4];
    int img, rows;
    int64_t row0;
    pl_tile(tpi, P, img, row0, rows);
    const int tid = threadIdx.x;
    int g0r, Gr, g0n, Gn;
    ts_frame_range(offs_ref, img, G_ref_total, g0r, Gr);
    ts_frame_range(offs_next, img, G_next_total, g0n, Gn);
    if (tid < Gn) s_idn[tid] = ids_next[g0n + tid];
    __syncthreads();
    if (tid < Gr) {
        const int64_t id = ids_ref[g0r + tid];
        int k = -1;
        for (int q = 0; q < Gn; ++q)
            if (s_idn[q] == id) {
                k = q;
                break;
            }
        s_id[tid] = id;
        s_k[tid] = k < 0 ? -1 : g0n + k;
        float4 reg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k >= 0) {
            const float4 r = box_ref[g0r + tid];
            // center_size (box_utils.py:25-35): ((x2 + x1) / 2, (y2 + y1) / 2, x2 - x1, y2 - y1)
            reg = stm_encode_one(box_next[g0n + k], make_float4((r.z + r.x) / 2.0f, (r.w + r.y) / 2.0f, r.z - r.x, r.w - r.y));
        }
        s_reg[tid] = reg;
    }
    __syncthreads();
    bool pos = false;
    if (tid < rows) {
        const int64_t row = row0 + tid;
        const int64_t id = ids_t[row];
        float4 reg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int64_t kn = -1;
        if (id > 0) {
            int j = Gr - 1;
            while (j >= 0 && s_id[j] != id) --j;
            if (j >= 0 && s_k[j] >= 0) {
                pos = true;
                reg = s_reg[j];
                kn = s_k[j];
            }
        }
        pos_t[row] = pos ? 1 : 0;
        reg_t[row] = reg;
        idx_next[row] = kn;
    }
    const unsigned long long m = __ballot(pos);
    if ((tid & 63) == 0) sc[tid >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (tid == 0) tilecnt[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

struct GatherArgs {
    const float4 *loc, *priors, *reg_t, *box_next;
    const float* coeff;
    const int64_t* idx_next;
    const unsigned* meta;
    const int* idx;
    const float* wts;
    float *rois, *coeff_rows, *w_rows;
    float4 *reg_rows, *box_rows;
    int64_t* idx_rows;
    int *row_clip, *n_dev, *status;
    int n_rows, P, M, G_next_total, fh, fw;
};

__global__ __launch_bounds__(256) void t2s_gather_kernel(const GatherArgs a)
{
    const int r = blockIdx.x * (256 / TS_LANES) + (threadIdx.x / TS_LANES), l = threadIdx.x % TS_LANES;
    const unsigned n = a.meta[TM_N];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.n_dev = (int)min(n, (unsigned)a.n_rows);
        *a.status = (int)a.meta[TM_STATUS];
    }
    if (r >= a.n_rows) return;
    const bool live = (unsigned)r < n;
    int src = 0, clip = 0;
    int64_t kn = 0;
    if (live) {
        src = a.idx[r];
        clip = src / a.P;
        kn = a.idx_next[src];
        kn = kn < 0 ? 0 : (kn >= a.G_next_total ? a.G_next_total - 1 : kn);       // (a listed row always has a valid index; any value stays inside)
    }
    if (l == 0) {
        float* o = a.rois + (int64_t)r * 5;
        if (live) {
            stm_roi_one(stm_decode_one(a.loc[src], a.priors[src - clip * a.P]), (float)clip, a.fh, a.fw, o);
        } else {
            o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 1.0f; o[4] = 1.0f;
        }
    } else if (l == 1) {
        a.reg_rows[r] = live ? a.reg_t[src] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else if (l == 2) {
        a.box_rows[r] = live ? a.box_next[kn] : make_float4(0.0f, 0.0f, 1.0f, 1.0f);
    } else if (l == 3) {
        a.idx_rows[r] = kn;
        a.row_clip[r] = clip;
        a.w_rows[r] = live ? a.wts[r] : 0.0f;
    }
    if (l < a.M / 4)
        reinterpret_cast<float4*>(a.coeff_rows + (int64_t)r * a.M)[l] =
            live ? reinterpret_cast<const float4*>(a.coeff + (int64_t)src * a.M)[l] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__device__ __forceinline__ float ts_sl1(float d)
{
    const float ad = fabsf(d);
    return ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
}

__global__ __launch_bounds__(256) void t2s_reduce_kernel(const float* __restrict__ bbox_reg, const float* __restrict__ reg_rows,
                                                         const float* __restrict__ bce, const float* __restrict__ box_rows,
                                                         const float* __restrict__ w_rows, const int* __restrict__ n_dev,
                                                         const int* __restrict__ status, float* __restrict__ b_shift, float* __restrict__ m_shift,
                                                         int n_rows, int H, int W, double scale_b, double scale_m)
{
    __shared__ double sd[4];
    const int n = min(max(*n_dev, 0), n_rows);
    double sb = 0.0, sm = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) {
        const double w = (double)w_rows[r];
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) t += (double)ts_sl1(bbox_reg[4 * (int64_t)r + c] - reg_rows[4 * (int64_t)r + c]);
        sb += w * t;
        if (m_shift) {                                       // :314-317: the box's width and height in target pixels, not clamped
            const float bw = (box_rows[4 * (int64_t)r + 2] - box_rows[4 * (int64_t)r]) * (float)W;
            const float bh = (box_rows[4 * (int64_t)r + 3] - box_rows[4 * (int64_t)r + 1]) * (float)H;
            sm += w * (double)(bce[r] / bw / bh);
        }
    }
    sb = stm_block_sum_f64(sb, sd);
    sm = stm_block_sum_f64(sm, sd);
    if (threadIdx.x == 0) {
        const bool over = *status != 0;
        const float nan = stm_nan_f32();
        *b_shift = over ? nan : (float)(scale_b * sb);
        if (m_shift) *m_shift = over ? nan : (float)(scale_m * sm);
    }
}

__global__ __launch_bounds__(256) void t2s_reduce_backward_kernel(const float* __restrict__ g_b, const float* __restrict__ g_m,
                                                                  const float* __restrict__ bbox_reg, const float* __restrict__ reg_rows,
                                                                  const float* __restrict__ box_rows, const float* __restrict__ w_rows,
                                                                  const int* __restrict__ n_dev, const int* __restrict__ status,
                                                                  float* __restrict__ grad_reg, float* __restrict__ grad_bce, int n_rows, int H, int W,
                                                                  double scale_b, double scale_m)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int n = min(max(*n_dev, 0), n_rows);
    float gr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gm = 0.0f;
    if (*status != 0) {
        gr[0] = gr[1] = gr[2] = gr[3] = gm = stm_nan_f32();
    } else if (r < n) {
        const double w = (double)w_rows[r];
        if (grad_reg && g_b) {
            const float s = (float)((double)g_b[0] * scale_b * w);           // the incoming gradient, alpha / bs and w_r: one rounding
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = bbox_reg[4 * (int64_t)r + c] - reg_rows[4 * (int64_t)r + c];
                gr[c] = s * (fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f));
            }
        }
        if (grad_bce && g_m) {
            const float bw = (box_rows[4 * (int64_t)r + 2] - box_rows[4 * (int64_t)r]) * (float)W;
            const float bh = (box_rows[4 * (int64_t)r + 3] - box_rows[4 * (int64_t)r + 1]) * (float)H;
            gm = (float)((double)g_m[0] * scale_m * w / (double)bw / (double)bh);
        }
    }
    if (grad_reg) {
#pragma unroll
        for (int c = 0; c < 4; ++c) grad_reg[4 * (int64_t)r + c] = gr[c];
    }
    if (grad_bce) grad_bce[r] = gm;
}

}  // namespace

extern "C" size_t stm_t2s_workspace_bytes(int B, int P)
{
    if (B <= 0 || P <= 0 || (int64_t)B * P > PL_MAX_N) return 64;
    return pos_layout(B, P).words * sizeof(unsigned) + 64;
}

extern "C" int stm_t2s_targets_f32(const int64_t* ids_t, const float* boxes_ref, const int64_t* ids_ref, const int* offs_ref, int G_ref_total,
                                   int G_ref_max, const float* boxes_next, const int64_t* ids_next, const int* offs_next, int G_next_total,
                                   int G_next_max, int64_t* pos_t, float* reg_t, int64_t* idx_next, int* prefix, int B, int P, int max_rows,
                                   void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_t2s_targets_f32";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(G_ref_total >= 0 && G_next_total >= 0 && G_ref_max >= 0 && G_next_max >= 0 && G_ref_max <= G_ref_total &&
                    G_next_max <= G_next_total, STM_EINVAL, "%s: box counts %d (max %d) / %d (max %d)", who, G_ref_total, G_ref_max, G_next_total,
                G_next_max);
    STM_REQUIRE(G_ref_max <= TS_GMAX && G_next_max <= TS_GMAX, STM_EUNSUPPORTED, "%s: %d / %d boxes in one frame (limit %d)", who, G_ref_max,
                G_next_max, TS_GMAX);
    STM_REQUIRE(ids_t && offs_ref && offs_next && pos_t && reg_t && idx_next, STM_ENULL,
                "%s: ids_t/offs_ref/offs_next/pos_t/reg_t/idx_next must be non-NULL", who);
    STM_REQUIRE((G_ref_total == 0 || (boxes_ref && ids_ref)) && (G_next_total == 0 || (boxes_next && ids_next)), STM_ENULL,
                "%s: boxes and ids of a frame set with rows must be non-NULL", who);
    STM_REQUIRE(stm_aligned16(boxes_ref) && stm_aligned16(boxes_next) && stm_aligned16(reg_t), STM_EINVAL,
                "%s: boxes_ref, boxes_next and reg_t must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_t2s_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned", who);
    const PosLayout L = pos_layout(B, P);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    const int tpi = stm_cdiv(P, PL_TILE), nT = B * tpi;
    hipStream_t st = stm_hs(stream);
    hipLaunchKernelGGL(t2s_targets_kernel, dim3(nT), dim3(256), 0, st, ids_t, reinterpret_cast<const float4*>(boxes_ref), ids_ref, offs_ref,
                       G_ref_total, reinterpret_cast<const float4*>(boxes_next), ids_next, offs_next, G_next_total, pos_t,
                       reinterpret_cast<float4*>(reg_t), idx_next, ws + L.tilecnt, P, tpi);
    STM_CHECK_LAUNCH("t2s_targets_kernel");
    return pos_list(pos_t, false, prefix, max_rows, B, P, ws, L, st);   // (the target kernel wrote the tiles' counts)
}

extern "C" int stm_t2s_gather_f32(const float* loc_ref, const float* priors, const float* coeff_ref, const float* reg_t, const int64_t* idx_next,
                                  const float* boxes_next, int G_next_total, float* rois, float* reg_rows, float* coeff_rows, float* box_rows,
                                  int64_t* idx_rows, int* row_clip, float* w_rows, int* n_dev, int* status, int n_rows, int B, int P, int M,
                                  int feat_h, int feat_w, const void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_t2s_gather_f32";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(n_rows >= 1 && G_next_total >= 1 && feat_h >= 1 && feat_w >= 1, STM_EINVAL, "%s: n_rows=%d G_next_total=%d feature map %dx%d", who,
                n_rows, G_next_total, feat_h, feat_w);
    STM_REQUIRE(n_rows <= TS_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, TS_MAX_ROWS);
    STM_REQUIRE(M == 8 || M == 32 || M == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, M);
    STM_REQUIRE(loc_ref && priors && coeff_ref && reg_t && idx_next && boxes_next && rois && reg_rows && coeff_rows && box_rows && idx_rows &&
                    row_clip && w_rows && n_dev && status, STM_ENULL, "%s: NULL argument", who);
    STM_REQUIRE(stm_aligned16(loc_ref) && stm_aligned16(priors) && stm_aligned16(coeff_ref) && stm_aligned16(reg_t) && stm_aligned16(boxes_next) &&
                    stm_aligned16(reg_rows) && stm_aligned16(coeff_rows) && stm_aligned16(box_rows), STM_EINVAL,
                "%s: the fp32 inputs and the row outputs must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_t2s_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned (it is the one stm_t2s_targets_f32 filled)", who);
    const PosLayout L = pos_layout(B, P);
    const unsigned* ws = reinterpret_cast<const unsigned*>(workspace);
    GatherArgs a;
    a.loc = reinterpret_cast<const float4*>(loc_ref);
    a.priors = reinterpret_cast<const float4*>(priors);
    a.reg_t = reinterpret_cast<const float4*>(reg_t);
    a.box_next = reinterpret_cast<const float4*>(boxes_next);
    a.coeff = coeff_ref;
    a.idx_next = idx_next;
    a.meta = ws + L.meta;
    a.idx = reinterpret_cast<const int*>(ws + L.idx);
    a.wts = reinterpret_cast<const float*>(ws + L.wts);
    a.rois = rois;
    a.coeff_rows = coeff_rows;
    a.w_rows = w_rows;
    a.reg_rows = reinterpret_cast<float4*>(reg_rows);
    a.box_rows = reinterpret_cast<float4*>(box_rows);
    a.idx_rows = idx_rows;
    a.row_clip = row_clip;
    a.n_dev = n_dev;
    a.status = status;
    a.n_rows = n_rows; a.P = P; a.M = M; a.G_next_total = G_next_total; a.fh = feat_h; a.fw = feat_w;
    hipLaunchKernelGGL(t2s_gather_kernel, dim3(stm_cdiv(n_rows, 256 / TS_LANES)), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("t2s_gather_kernel");
    return STM_OK;
}

extern "C" int stm_t2s_reduce_f32(const float* bbox_reg, const float* reg_rows, const float* bce, const float* box_rows, const float* w_rows,
                                  const int* n_dev, const int* status, float* b_shift, float* m_shift, int n_rows, int B, int H, int W,
                                  double boxshift_alpha, double maskshift_alpha, stm_stream_t stream)
{
    const char* who = "stm_t2s_reduce_f32";
    STM_REQUIRE(n_rows >= 1 && B >= 1, STM_EINVAL, "%s: n_rows=%d B=%d", who, n_rows, B);
    STM_REQUIRE(bbox_reg && reg_rows && w_rows && n_dev && status && b_shift, STM_ENULL,
                "%s: bbox_reg/reg_rows/w_rows/n_dev/status/b_shift must be non-NULL", who);
    STM_REQUIRE(!m_shift || (bce && box_rows && H >= 1 && W >= 1), STM_ENULL, "%s: m_shift needs bce, box_rows and the mask size", who);
    hipLaunchKernelGGL(t2s_reduce_kernel, dim3(1), dim3(256), 0, stm_hs(stream), bbox_reg, reg_rows, bce, box_rows, w_rows, n_dev, status, b_shift,
                       m_shift, n_rows, H, W, boxshift_alpha / (double)B, maskshift_alpha / (double)B);
    STM_CHECK_LAUNCH("t2s_reduce_kernel");
    return STM_OK;
}

extern "C" int stm_t2s_reduce_backward_f32(const float* grad_b, const float* grad_m, const float* bbox_reg, const float* reg_rows,
                                           const float* box_rows, const float* w_rows, const int* n_dev, const int* status, float* grad_bbox_reg,
                                           float* grad_bce, int n_rows, int B, int H, int W, double boxshift_alpha, double maskshift_alpha,
                                           stm_stream_t stream)
{
    const char* who = "stm_t2s_reduce_backward_f32";
    STM_REQUIRE(n_rows >= 1 && B >= 1, STM_EINVAL, "%s: n_rows=%d B=%d", who, n_rows, B);
    if (!grad_bbox_reg && !grad_bce) return STM_OK;
    STM_REQUIRE(bbox_reg && reg_rows && w_rows && n_dev && status, STM_ENULL, "%s: bbox_reg/reg_rows/w_rows/n_dev/status must be non-NULL", who);
    STM_REQUIRE(!grad_bce || (box_rows && H >= 1 && W >= 1), STM_ENULL, "%s: grad_bce needs box_rows and the mask size", who);
    hipLaunchKernelGGL(t2s_reduce_backward_kernel, dim3(stm_cdiv(n_rows, 256)), dim3(256), 0, stm_hs(stream), grad_b, grad_m, bbox_reg, reg_rows,
                       box_rows, w_rows, n_dev, status, grad_bbox_reg, grad_bce, n_rows, H, W, boxshift_alpha / (double)B,
                       maskshift_alpha / (double)B);
    STM_CHECK_LAUNCH("t2s_reduce_backward_kernel");
    return STM_OK;
}
