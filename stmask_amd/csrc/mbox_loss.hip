// mbox_loss.hip -- the batched mask term of the reference's MultiBoxLoss (lincomb_mask_loss, layers/modules/multibox_loss.py:544-616, :636:
// losses['M']) for gfx950: the batch-wide ordered list of the positive priors, the gather of everything the mask kernels read through it, the
// weighted reduction with its adjoint and the return of the coefficient rows to grad mask_data.  The mask itself, its BCE and its two
// gradients (stm_lincomb_rows_backward_f32, stm_lincomb_rows_proto_backward_f32) are the existing kernels (mask_ops.hip, mask_loss.hip,
// lincomb_backward.hip).  Conventions: include/stmask_hip_train.h.
//
// A prior is positive iff conf_t > 0.  Row r of the list is prior src of image b; its crop box is the reference's :559-563 -- decode
// (stm_decode_one), center_size, width and height times 1.2f, point_form, clamp to [1e-5, 1] -- in IEEE fp32, the reference's operand order
// (-ffp-contract=off).  idx_t is data: it is clamped into its image's masks, then into the concatenated masks; nothing can fault.
//
// stm_mbox_positives (3 launches): pos_index.h -- count, scan (with the [B + 1] prefix and the status word n > max_rows), index.
// stm_mbox_gather_f32 (1 launch): 16 lanes per row, n_rows rows with the live count in device memory; rows past it are padding (zero
//   coefficients, box (0, 0, 1, 1), image 0, mask row 0, scale 0).
// stm_mbox_reduce_f32 (1 launch, one workgroup): fp32 terms, products and sums in double, thread t takes rows t, t + 256, ... whatever n_rows
//   is, so the padded and the exact form add the same numbers in the same order.  stm_mbox_reduce_backward_f32 (1 launch): one thread per row.
// stm_mbox_scatter_coeff_f32 (1 launch): the tiles of the list again: every row of grad mask_data is written once -- its list row's gradient,
//   or exact zeros -- without atomics and without reading mask_data.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no kernel of this file uses scratch.
#include "stm_common.h"
#include "pos_index.h"
#include "../../include/stmask_hip_train.h"

namespace {

constexpr int MB_LANES = 16;           // lanes per row of the gather
constexpr int MB_MAX_ROWS = 65535;     // rows the mask kernels take (their grid.y: lincomb_backward.hip's LC_MAX_ROWS)

// torch.clamp(x, min=lo, max=hi): a NaN stays a NaN
__device__ __forceinline__ float mb_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// multibox_loss.py:559-563 on one decoded box
__device__ __forceinline__ float4 mb_crop_box(const float4 d)
{
    const float cx = (d.z + d.x) / 2.0f, cy = (d.w + d.y) / 2.0f;            // center_size (box_utils.py:33-34)
    float w = d.z - d.x, h = d.w - d.y;
    w = w * 1.2f;
    h = h * 1.2f;
    const float hw = w / 2.0f, hh = h / 2.0f;                                  // point_form (box_utils.py:20-21)
    return make_float4(mb_clamp(cx - hw, 1e-5f, 1.0f), mb_clamp(cy - hh, 1e-5f, 1.0f), mb_clamp(cx + hw, 1e-5f, 1.0f),
                       mb_clamp(cy + hh, 1e-5f, 1.0f));
}

struct MbGatherArgs {
    const float4 *loc, *priors;
    const float* mask_data;
    const int64_t* idx_t;
    const int* mask_offs;
    const unsigned* meta;
    const int* idx;
    const float* wts;
    float *coeff_rows, *scale_rows;
    float4* box_rows;
    int64_t* idx_rows;
    int *row_img, *n_dev, *status;
    int n_rows, B, P, M, G_total, H, W, priors_per_image;
};

__global__ __launch_bounds__(256) void mbox_gather_kernel(const MbGatherArgs a)
{
    const int r = blockIdx.x * (256 / MB_LANES) + (threadIdx.x / MB_LANES), l = threadIdx.x % MB_LANES;
    const unsigned n = a.meta[TM_N];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.n_dev = (int)min(n, (unsigned)a.n_rows);
        *a.status = (int)a.meta[TM_STATUS];
    }
    if (r >= a.n_rows) return;
    const bool live = (unsigned)r < n;
    int src = 0, img = 0;
    if (live) {
        src = a.idx[r];
        src = src < 0 ? 0 : (src >= a.B * a.P ? a.B * a.P - 1 : src);        // (the list holds valid rows; any value stays inside)
        img = src / a.P;
    }
    if (l == 0) {
        float4 box = make_float4(0.0f, 0.0f, 1.0f, 1.0f);
        float scale = 0.0f;
        if (live) {
            box = mb_crop_box(stm_decode_one(a.loc[src], a.priors[a.priors_per_image ? src : src - img * a.P]));
            // :608-613: the box's width and height in target pixels, each at least 1
            float bw = (box.z - box.x) * (float)a.W, bh = (box.w - box.y) * (float)a.H;
            bw = bw < 1.0f ? 1.0f : bw;
            bh = bh < 1.0f ? 1.0f : bh;
            scale = a.wts[r] / bw / bh;
        }
        a.box_rows[r] = box;
        a.scale_rows[r] = scale;
    } else if (l == 1) {
        int64_t g = 0;
        if (live) {
            int lo = a.mask_offs[img], hi = a.mask_offs[img + 1];
            lo = lo < 0 ? 0 : (lo > a.G_total ? a.G_total : lo);
            hi = hi < lo ? lo : (hi > a.G_total ? a.G_total : hi);
            int64_t k = a.idx_t[src];
            k = k < 0 ? 0 : (k >= hi - lo ? (int64_t)(hi - lo) - 1 : k);      // into the image's masks ...
            g = (int64_t)lo + k;
            g = g < 0 ? 0 : (g >= a.G_total ? (int64_t)a.G_total - 1 : g);    // ... and, for an image without masks, into the concatenation
        }
        a.idx_rows[r] = g;
        a.row_img[r] = img;
    }
    if (l < a.M / 4)
        reinterpret_cast<float4*>(a.coeff_rows + (int64_t)r * a.M)[l] =
            live ? reinterpret_cast<const float4*>(a.mask_data + (int64_t)src * a.M)[l] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(256) void mbox_reduce_kernel(const float* __restrict__ bce, const float* __restrict__ scale_rows,
                                                          const int* __restrict__ n_dev, const int* __restrict__ status,
                                                          float* __restrict__ loss, int n_rows, double alpha)
{
    __shared__ double sd[4];
    const int n = min(max(*n_dev, 0), n_rows);
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) s += (double)scale_rows[r] * (double)bce[r];
    s = stm_block_sum_f64(s, sd);
    if (threadIdx.x == 0) *loss = *status != 0 ? stm_nan_f32() : (float)(alpha * s);
}

__global__ __launch_bounds__(256) void mbox_reduce_backward_kernel(const float* __restrict__ g, const float* __restrict__ scale_rows,
                                                                   const int* __restrict__ n_dev, const int* __restrict__ status,
                                                                   float* __restrict__ grad_bce, int n_rows, double alpha)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int n = min(max(*n_dev, 0), n_rows);
    float v = 0.0f;
    if (*status != 0) v = stm_nan_f32();
    else if (r < n) v = (float)((double)g[0] * alpha * (double)scale_rows[r]);
    grad_bce[r] = v;
}

// ------------------------------------------------------------------------------------------ the coefficient rows back to grad mask_data
__global__ __launch_bounds__(256) void mbox_scatter_kernel(const float* __restrict__ grad_rows, const int64_t* __restrict__ conf_t,
                                                           const unsigned* __restrict__ tilepre, const int* __restrict__ n_dev,
                                                           const int* __restrict__ status, float* __restrict__ grad, int n_rows, int P, int tpi,
                                                           int M)
{
    __shared__ unsigned sw[4];
    __shared__ int s_rank[PL_TILE];                  // the list row of the tile's prior, or -1
    int img, rows;
    int64_t row0;
    pl_tile(tpi, P, img, row0, rows);
    const int tid = threadIdx.x;
    const bool pos = tid < rows && conf_t[row0 + tid] > 0;
    unsigned total;
    const unsigned rank = tilepre[blockIdx.x] + stm_block_excl_scan(pos ? 1u : 0u, sw, total);
    s_rank[tid] = pos ? (int)min(rank, 0x7FFFFFFFu) : -1;
    __syncthreads();
    const int n = min(max(*n_dev, 0), n_rows);
    const bool over = *status != 0;
    const int q4 = M / 4;
    const float4* src = reinterpret_cast<const float4*>(grad_rows);
    float4* dst = reinterpret_cast<float4*>(grad + row0 * M);
    for (int i = tid; i < rows * q4; i += 256) {
        const int row = i / q4, q = i - row * q4;
        const int r = s_rank[row];
        const float fill = r < 0 ? 0.0f : stm_nan_f32();
        float x = fill, y = fill, z = fill, w = fill;
        if (r >= 0 && !over && r < n) {
            const float4 v = src[(int64_t)r * q4 + q];
            x = v.x; y = v.y; z = v.z; w = v.w;
        }
        dst[i] = make_float4(x, y, z, w);
    }
}

}  // namespace

extern "C" size_t stm_mbox_workspace_bytes(int B, int P)
{
    if (B <= 0 || P <= 0 || (int64_t)B * P > PL_MAX_N) return 64;
    return pos_layout(B, P).words * sizeof(unsigned) + 64;
}

extern "C" int stm_mbox_positives(const int64_t* conf_t, int* prefix, int B, int P, int max_rows, void* workspace, size_t workspace_bytes,
                                  stm_stream_t stream)
{
    const char* who = "stm_mbox_positives";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(max_rows >= 0, STM_EINVAL, "%s: max_rows=%d", who, max_rows);
    STM_REQUIRE(max_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: max_rows=%d > %d", who, max_rows, MB_MAX_ROWS);
    STM_REQUIRE(conf_t && prefix, STM_ENULL, "%s: conf_t and prefix must be non-NULL", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_mbox_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned", who);
    const PosLayout L = pos_layout(B, P);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    return pos_list(conf_t, true, prefix, max_rows, B, P, ws, L, stm_hs(stream));
}

extern "C" int stm_mbox_gather_f32(const float* loc, const float* priors, int priors_per_image, const float* mask_data, const int64_t* idx_t,
                                   const int* mask_offs, int G_total, float* coeff_rows, float* box_rows, int* row_img, int64_t* idx_rows,
                                   float* scale_rows, int* n_dev, int* status, int n_rows, int B, int P, int M, int H, int W,
                                   const void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_mbox_gather_f32";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(n_rows >= 1 && G_total >= 1 && H >= 1 && W >= 1, STM_EINVAL, "%s: n_rows=%d G_total=%d masks %dx%d", who, n_rows, G_total, H, W);
    STM_REQUIRE(n_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, MB_MAX_ROWS);
    STM_REQUIRE(M == 8 || M == 32 || M == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, M);
    STM_REQUIRE(loc && priors && mask_data && idx_t && mask_offs && coeff_rows && box_rows && row_img && idx_rows && scale_rows && n_dev && status,
                STM_ENULL, "%s: NULL argument", who);
    STM_REQUIRE(stm_aligned16(loc) && stm_aligned16(priors) && stm_aligned16(mask_data) && stm_aligned16(coeff_rows) && stm_aligned16(box_rows),
                STM_EINVAL, "%s: the fp32 inputs and the row outputs must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_mbox_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned (it is the one stm_mbox_positives filled)", who);
    const PosLayout L = pos_layout(B, P);
    const unsigned* ws = reinterpret_cast<const unsigned*>(workspace);
    MbGatherArgs a;
    a.loc = reinterpret_cast<const float4*>(loc);
    a.priors = reinterpret_cast<const float4*>(priors);
    a.mask_data = mask_data;
    a.idx_t = idx_t;
    a.mask_offs = mask_offs;
    a.meta = ws + L.meta;
    a.idx = reinterpret_cast<const int*>(ws + L.idx);
    a.wts = reinterpret_cast<const float*>(ws + L.wts);
    a.coeff_rows = coeff_rows;
    a.scale_rows = scale_rows;
    a.box_rows = reinterpret_cast<float4*>(box_rows);
    a.idx_rows = idx_rows;
    a.row_img = row_img;
    a.n_dev = n_dev;
    a.status = status;
    a.n_rows = n_rows; a.B = B; a.P = P; a.M = M; a.G_total = G_total; a.H = H; a.W = W; a.priors_per_image = priors_per_image ? 1 : 0;
    hipLaunchKernelGGL(mbox_gather_kernel, dim3(stm_cdiv(n_rows, 256 / MB_LANES)), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("mbox_gather_kernel");
    return STM_OK;
}

extern "C" int stm_mbox_reduce_f32(const float* bce, const float* scale_rows, const int* n_dev, const int* status, float* loss, int n_rows,
                                   double mask_alpha, stm_stream_t stream)
{
    const char* who = "stm_mbox_reduce_f32";
    STM_REQUIRE(n_rows >= 1, STM_EINVAL, "%s: n_rows=%d", who, n_rows);
    STM_REQUIRE(n_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, MB_MAX_ROWS);
    STM_REQUIRE(bce && scale_rows && n_dev && status && loss, STM_ENULL, "%s: NULL argument", who);
    hipLaunchKernelGGL(mbox_reduce_kernel, dim3(1), dim3(256), 0, stm_hs(stream), bce, scale_rows, n_dev, status, loss, n_rows, mask_alpha);
    STM_CHECK_LAUNCH("mbox_reduce_kernel");
    return STM_OK;
}

extern "C" int stm_mbox_reduce_backward_f32(const float* grad_loss, const float* scale_rows, const int* n_dev, const int* status,
                                            float* grad_bce, int n_rows, double mask_alpha, stm_stream_t stream)
{
    const char* who = "stm_mbox_reduce_backward_f32";
    STM_REQUIRE(n_rows >= 1, STM_EINVAL, "%s: n_rows=%d", who, n_rows);
    STM_REQUIRE(n_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, MB_MAX_ROWS);
    STM_REQUIRE(grad_loss && scale_rows && n_dev && status && grad_bce, STM_ENULL, "%s: NULL argument", who);
    hipLaunchKernelGGL(mbox_reduce_backward_kernel, dim3(stm_cdiv(n_rows, 256)), dim3(256), 0, stm_hs(stream), grad_loss, scale_rows, n_dev,
                       status, grad_bce, n_rows, mask_alpha);
    STM_CHECK_LAUNCH("mbox_reduce_backward_kernel");
    return STM_OK;
}

extern "C" int stm_mbox_scatter_coeff_f32(const float* grad_rows, const int64_t* conf_t, const int* n_dev, const int* status,
                                          float* grad_mask_data, int n_rows, int B, int P, int M, const void* workspace, size_t workspace_bytes,
                                          stm_stream_t stream)
{
    const char* who = "stm_mbox_scatter_coeff_f32";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(n_rows >= 1, STM_EINVAL, "%s: n_rows=%d", who, n_rows);
    STM_REQUIRE(n_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, MB_MAX_ROWS);
    STM_REQUIRE(M == 8 || M == 32 || M == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, M);
    STM_REQUIRE(grad_rows && conf_t && n_dev && status && grad_mask_data, STM_ENULL, "%s: NULL argument", who);
    STM_REQUIRE(stm_aligned16(grad_rows) && stm_aligned16(grad_mask_data), STM_EINVAL, "%s: grad_rows and grad_mask_data must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_mbox_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned (it is the one stm_mbox_positives filled)", who);
    const PosLayout L = pos_layout(B, P);
    const unsigned* ws = reinterpret_cast<const unsigned*>(workspace);
    const int tpi = stm_cdiv(P, PL_TILE);
    hipLaunchKernelGGL(mbox_scatter_kernel, dim3(B * tpi), dim3(256), 0, stm_hs(stream), grad_rows, conf_t, ws + L.tilepre, n_dev, status,
                       grad_mask_data, n_rows, P, tpi, M);
    STM_CHECK_LAUNCH("mbox_scatter_kernel");
    return STM_OK;
}
