// mbox_loss.hip -- the batched mask term of the reference's MultiBoxLoss (lincomb_mask_loss, layers/modules/multibox_loss.py:544-616, :636:
// losses['M']) for gfx950: the batch-wide ordered list of the positive priors, the gather of everything the mask kernels read through it, the
// weighted reduction with its adjoint, the PROTOTYPE gradient of the row-prototype form of stm_lincomb_sigmoid_crop_f32 and the return of the
// coefficient rows to grad mask_data.  The mask itself, its BCE and the coefficient gradient are the existing kernels (mask_ops.hip,
// mask_loss.hip, t2s_loss.hip).  Conventions: include/stmask_hip_train.h.
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
// stm_lincomb_rows_proto_backward_f32 (1 or 2 launches): one thread is one prototype pixel with its M prototype values and M accumulators in
//   registers (lincomb_backward_kernel's layout, mask_backward.hip); grid (pixel blocks, images, row splits); a workgroup reads its image's
//   row range prefix[b] .. prefix[b + 1] on the device and walks it in row order in chunks of 16 whose tanh(coeff) and rectangles sit in LDS;
//   z = grad_out * e / (1 + e)^2 inside the rectangle, grad_out is not read outside.  The number of splits depends on h, w and the number of
//   images only (never on the number of rows), so the exact and the padded form make the same sums; the second launch adds the splits'
//   partials in split order.  An image without positives gets exact zeros.
// stm_mbox_scatter_coeff_f32 (1 launch): the tiles of the list again: every row of grad mask_data is written once -- its list row's gradient,
//   or exact zeros -- without atomics and without reading mask_data.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no kernel of this file uses scratch.
#include "stm_common.h"
#include "pos_index.h"
#include "../../include/stmask_hip_train.h"

namespace {

constexpr int MB_LANES = 16;           // lanes per row of the gather
constexpr int MB_MAX_ROWS = 65535;     // rows the mask kernels take (their grid.y)
constexpr int MB_DCHUNK = 16;          // rows per LDS chunk of the prototype gradient
constexpr int MB_MAX_SPLITS = 8;       // most row splits per (pixel block, image)

struct MbLayout {
    size_t meta, tilecnt, tilepre, npos, idx, wts, words;
};

MbLayout mb_layout(int B, int P)
{
    const size_t nT = (size_t)B * stm_cdiv(P, PL_TILE), N = (size_t)B * P;
    MbLayout L;
    size_t o = 0;
    L.meta = o;    o += TM_WORDS;
    L.tilecnt = o; o += nT;
    L.tilepre = o; o += nT;
    L.npos = o;    o += (size_t)B;
    L.idx = o;     o += N;
    L.wts = o;     o += N;
    L.words = o;
    return L;
}

__device__ __forceinline__ float mb_nan() { return __int_as_float(0x7FC00000); }

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
    if (threadIdx.x == 0) *loss = *status != 0 ? mb_nan() : (float)(alpha * s);
}

__global__ __launch_bounds__(256) void mbox_reduce_backward_kernel(const float* __restrict__ g, const float* __restrict__ scale_rows,
                                                                   const int* __restrict__ n_dev, const int* __restrict__ status,
                                                                   float* __restrict__ grad_bce, int n_rows, double alpha)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int n = min(max(*n_dev, 0), n_rows);
    float v = 0.0f;
    if (*status != 0) v = mb_nan();
    else if (r < n) v = (float)((double)g[0] * alpha * (double)scale_rows[r]);
    grad_bce[r] = v;
}

// ------------------------------------------------------------------------------------------ grad_proto of the row-prototype mask
template <int M>
__global__ __launch_bounds__(256) void rows_proto_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ proto,
                                                                  const float* __restrict__ coeff, const float* __restrict__ boxes,
                                                                  const int* __restrict__ prefix, const int* __restrict__ status,
                                                                  float* __restrict__ gp_out, int h, int w, int n, int n_proto)
{
    static_assert(M % 4 == 0, "layout");
    __shared__ float sc[MB_DCHUNK * M];
    __shared__ float sb[MB_DCHUNK * 4];              // x1, x2, y1, y2 (float bounds, padding 1)
    __shared__ int hit[MB_DCHUNK];
    const int hw = h * w;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * 256;
    const int pix = p0 + tid;
    const bool live = pix < hw;
    const int set = blockIdx.y, splits = gridDim.z;
    // this image's rows, whatever the prefix holds: never outside [0, n)
    int lo = prefix[set], hi = prefix[set + 1];
    lo = min(max(lo, 0), n);
    hi = min(max(hi, lo), n);
    const int per = ((hi - lo + MB_DCHUNK - 1) / MB_DCHUNK + splits - 1) / splits * MB_DCHUNK;   // rows per split: whole chunks
    const int r0 = min(hi, lo + (int)blockIdx.z * per), r1 = min(hi, r0 + per);
    const int y = pix / w, x = pix - y * w;
    const float fx = (float)x, fy = (float)y;

    float p[M], gp[M];
    if (live) {
        const float4* pr = reinterpret_cast<const float4*>(proto + ((int64_t)set * hw + pix) * M);
#pragma unroll
        for (int q = 0; q < M / 4; ++q) {
            const float4 v = pr[q];
            p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < M; ++k) p[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < M; ++k) gp[k] = 0.0f;

    for (int c0 = r0; c0 < r1; c0 += MB_DCHUNK) {
        const int nd = min(MB_DCHUNK, r1 - c0);
        __syncthreads();                             // the previous chunk's readers of sc / sb / hit are done
        for (int i = tid; i < nd * M; i += 256) sc[i] = tanhf(coeff[(int64_t)c0 * M + i]);
        if (tid < MB_DCHUNK) {
            int touch = 0;
            if (tid < nd) {
                float x1, x2, y1, y2;
                const float* b = boxes + (int64_t)(c0 + tid) * 4;
                stm_sanitize(b[0], b[2], w, 1, x1, x2);
                stm_sanitize(b[1], b[3], h, 1, y1, y2);
                sb[tid * 4 + 0] = x1;
                sb[tid * 4 + 1] = x2;
                sb[tid * 4 + 2] = y1;
                sb[tid * 4 + 3] = y2;
                // does the rectangle touch this workgroup's pixel span at all (the forward's test)
                const int pl = min(p0 + 255, hw - 1);
                const int ya = p0 / w, yb = pl / w;
                bool t = (float)yb >= y1 && (float)ya < y2;
                if (t && ya == yb) t = (float)(pl - ya * w) >= x1 && (float)(p0 - ya * w) < x2;
                touch = t ? 1 : 0;
            }
            hit[tid] = touch;
        }
        __syncthreads();
        for (int d = 0; d < nd; ++d) {
            if (!hit[d]) continue;                   // workgroup-uniform
            const bool inside = live && fx >= sb[d * 4] && fx < sb[d * 4 + 1] && fy >= sb[d * 4 + 2] && fy < sb[d * 4 + 3];
            if (inside) {
                float a = 0.0f;
#pragma unroll
                for (int k = 0; k < M; ++k) a = fmaf(p[k], sc[d * M + k], a);
                const float e = expf(-fabsf(a));
                const float ope = 1.0f + e;
                const float z = grad_out[(int64_t)(c0 + d) * hw + pix] * (e / (ope * ope));
#pragma unroll
                for (int k = 0; k < M; ++k) gp[k] = fmaf(z, sc[d * M + k], gp[k]);
            }
        }
    }
    if (live) {
        if (status && *status != 0) {
#pragma unroll
            for (int k = 0; k < M; ++k) gp[k] = mb_nan();
        }
        float4* o = reinterpret_cast<float4*>(gp_out + (((int64_t)blockIdx.z * n_proto + set) * hw + pix) * M);
#pragma unroll
        for (int q = 0; q < M / 4; ++q) o[q] = make_float4(gp[4 * q], gp[4 * q + 1], gp[4 * q + 2], gp[4 * q + 3]);
    }
}

// grad_proto = sum over the row splits, in split order, of part[s]; 4 floats per thread
__global__ __launch_bounds__(256) void rows_proto_reduce_kernel(const float4* __restrict__ part, float4* __restrict__ grad_proto, int64_t total4,
                                                                int splits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    float4 s = part[i];
    for (int b = 1; b < splits; ++b) {
        const float4 v = part[(int64_t)b * total4 + i];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    grad_proto[i] = s;
}

// rows are split over workgroups until the grid has ~2 workgroups per CU; a function of the SHAPES only (not of the number of rows)
int mb_splits(int n_proto, int64_t hw)
{
    const int64_t wgs = (int64_t)stm_cdiv(hw, 256) * n_proto;
    return (int)std::min<int64_t>(MB_MAX_SPLITS, std::max<int64_t>(1, 512 / wgs));
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
        const float fill = r < 0 ? 0.0f : mb_nan();
        float x = fill, y = fill, z = fill, w = fill;
        if (r >= 0 && !over && r < n) {
            const float4 v = src[(int64_t)r * q4 + q];
            x = v.x; y = v.y; z = v.z; w = v.w;
        }
        dst[i] = make_float4(x, y, z, w);
    }
}

int mb_check(const char* who, int B, int P)
{
    STM_REQUIRE(B >= 1 && P >= 1, STM_EINVAL, "%s: B=%d P=%d", who, B, P);
    STM_REQUIRE((int64_t)B * P <= PL_MAX_N, STM_EUNSUPPORTED, "%s: B*P=%lld > %d rows", who, (long long)B * P, PL_MAX_N);
    return STM_OK;
}

bool mb_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" size_t stm_mbox_workspace_bytes(int B, int P)
{
    if (B <= 0 || P <= 0 || (int64_t)B * P > PL_MAX_N) return 64;
    return mb_layout(B, P).words * sizeof(unsigned) + 64;
}

extern "C" int stm_mbox_positives(const int64_t* conf_t, int* prefix, int B, int P, int max_rows, void* workspace, size_t workspace_bytes,
                                  stm_stream_t stream)
{
    const char* who = "stm_mbox_positives";
    const int rc = mb_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(max_rows >= 0, STM_EINVAL, "%s: max_rows=%d", who, max_rows);
    STM_REQUIRE(max_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: max_rows=%d > %d", who, max_rows, MB_MAX_ROWS);
    STM_REQUIRE(conf_t && prefix, STM_ENULL, "%s: conf_t and prefix must be non-NULL", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_mbox_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned", who);
    const MbLayout L = mb_layout(B, P);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    const int tpi = stm_cdiv(P, PL_TILE), nT = B * tpi;
    hipStream_t st = stm_hs(stream);
    hipLaunchKernelGGL(pos_count_kernel, dim3(nT), dim3(256), 0, st, conf_t, ws + L.tilecnt, P, tpi);
    STM_CHECK_LAUNCH("pos_count_kernel");
    hipLaunchKernelGGL(pos_scan_kernel, dim3(1), dim3(256), 0, st, ws + L.tilecnt, ws + L.tilepre, ws + L.npos, ws + L.meta, prefix,
                       max_rows > 0 ? (unsigned)max_rows : 0xFFFFFFFFu, nT, B, tpi);
    STM_CHECK_LAUNCH("pos_scan_kernel");
    hipLaunchKernelGGL(pos_index_kernel, dim3(nT), dim3(256), 0, st, conf_t, ws + L.tilepre, ws + L.npos, reinterpret_cast<int*>(ws + L.idx),
                       reinterpret_cast<float*>(ws + L.wts), P, tpi);
    STM_CHECK_LAUNCH("pos_index_kernel");
    return STM_OK;
}

extern "C" int stm_mbox_gather_f32(const float* loc, const float* priors, int priors_per_image, const float* mask_data, const int64_t* idx_t,
                                   const int* mask_offs, int G_total, float* coeff_rows, float* box_rows, int* row_img, int64_t* idx_rows,
                                   float* scale_rows, int* n_dev, int* status, int n_rows, int B, int P, int M, int H, int W,
                                   const void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_mbox_gather_f32";
    const int rc = mb_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(n_rows >= 1 && G_total >= 1 && H >= 1 && W >= 1, STM_EINVAL, "%s: n_rows=%d G_total=%d masks %dx%d", who, n_rows, G_total, H, W);
    STM_REQUIRE(n_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, MB_MAX_ROWS);
    STM_REQUIRE(M == 8 || M == 32 || M == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, M);
    STM_REQUIRE(loc && priors && mask_data && idx_t && mask_offs && coeff_rows && box_rows && row_img && idx_rows && scale_rows && n_dev && status,
                STM_ENULL, "%s: NULL argument", who);
    STM_REQUIRE(mb_aligned16(loc) && mb_aligned16(priors) && mb_aligned16(mask_data) && mb_aligned16(coeff_rows) && mb_aligned16(box_rows),
                STM_EINVAL, "%s: the fp32 inputs and the row outputs must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_mbox_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned (it is the one stm_mbox_positives filled)", who);
    const MbLayout L = mb_layout(B, P);
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

extern "C" size_t stm_lincomb_rows_proto_backward_workspace_bytes(int n_proto, int h, int w, int m)
{
    // the shapes stm_lincomb_rows_proto_backward_f32 refuses: 64
    if (n_proto <= 0 || n_proto > 65535 || h <= 0 || w <= 0 || !(m == 8 || m == 32 || m == 64)) return 64;
    const int64_t hw = (int64_t)h * w;
    if (hw * n_proto >= (1ll << 31) - 256) return 64;
    const int splits = mb_splits(n_proto, hw);
    return (splits > 1 ? (size_t)splits * n_proto * hw * m * sizeof(float) : 0) + 64;
}

extern "C" int stm_lincomb_rows_proto_backward_f32(const float* grad_out, const float* proto, int n_proto, const float* coeff,
                                                   const float* boxes, const int* prefix, const int* status, float* grad_proto, int h, int w,
                                                   int m, int n, void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_lincomb_rows_proto_backward_f32";
    STM_REQUIRE(n >= 1 && n_proto >= 1 && n_proto <= 65535, STM_EINVAL, "%s: n=%d n_proto=%d", who, n, n_proto);
    STM_REQUIRE(h > 0 && w > 0 && (int64_t)h * w * n_proto < (1ll << 31) - 256, STM_EINVAL, "%s: bad mask size %dx%d x %d sets", who, h, w, n_proto);
    STM_REQUIRE(m == 8 || m == 32 || m == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, m);
    STM_REQUIRE(n <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n=%d > %d", who, n, MB_MAX_ROWS);
    STM_REQUIRE(grad_out && proto && coeff && boxes && prefix && grad_proto, STM_ENULL,
                "%s: grad_out/proto/coeff/boxes/prefix/grad_proto must be non-NULL", who);
    STM_REQUIRE(mb_aligned16(proto) && mb_aligned16(grad_proto) && mb_aligned16(workspace), STM_EINVAL,
                "%s: proto, grad_proto and the workspace must be 16-byte aligned", who);
    const int hw = h * w;
    const int splits = mb_splits(n_proto, hw);
    STM_REQUIRE(splits == 1 || (workspace && workspace_bytes >= stm_lincomb_rows_proto_backward_workspace_bytes(n_proto, h, w, m)), STM_EWORKSPACE,
                "%s: workspace missing or too small", who);
    float* gp_out = splits > 1 ? reinterpret_cast<float*>(workspace) : grad_proto;
    const dim3 grid(stm_cdiv(hw, 256), n_proto, splits);
    hipStream_t st = stm_hs(stream);
    if (m == 32)
        hipLaunchKernelGGL((rows_proto_backward_kernel<32>), grid, dim3(256), 0, st, grad_out, proto, coeff, boxes, prefix, status, gp_out, h, w, n,
                           n_proto);
    else if (m == 8)
        hipLaunchKernelGGL((rows_proto_backward_kernel<8>), grid, dim3(256), 0, st, grad_out, proto, coeff, boxes, prefix, status, gp_out, h, w, n,
                           n_proto);
    else
        hipLaunchKernelGGL((rows_proto_backward_kernel<64>), grid, dim3(256), 0, st, grad_out, proto, coeff, boxes, prefix, status, gp_out, h, w, n,
                           n_proto);
    STM_CHECK_LAUNCH("rows_proto_backward_kernel");
    if (splits > 1) {
        const int64_t total4 = (int64_t)n_proto * hw * m / 4;
        hipLaunchKernelGGL(rows_proto_reduce_kernel, dim3(stm_cdiv(total4, 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(gp_out),
                           reinterpret_cast<float4*>(grad_proto), total4, splits);
        STM_CHECK_LAUNCH("rows_proto_reduce_kernel");
    }
    return STM_OK;
}

extern "C" int stm_mbox_scatter_coeff_f32(const float* grad_rows, const int64_t* conf_t, const int* n_dev, const int* status,
                                          float* grad_mask_data, int n_rows, int B, int P, int M, const void* workspace, size_t workspace_bytes,
                                          stm_stream_t stream)
{
    const char* who = "stm_mbox_scatter_coeff_f32";
    const int rc = mb_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(n_rows >= 1, STM_EINVAL, "%s: n_rows=%d", who, n_rows);
    STM_REQUIRE(n_rows <= MB_MAX_ROWS, STM_EUNSUPPORTED, "%s: n_rows=%d > %d", who, n_rows, MB_MAX_ROWS);
    STM_REQUIRE(M == 8 || M == 32 || M == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, M);
    STM_REQUIRE(grad_rows && conf_t && n_dev && status && grad_mask_data, STM_ENULL, "%s: NULL argument", who);
    STM_REQUIRE(mb_aligned16(grad_rows) && mb_aligned16(grad_mask_data), STM_EINVAL, "%s: grad_rows and grad_mask_data must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_mbox_workspace_bytes(B, P) && (uintptr_t)workspace % 8 == 0, STM_EWORKSPACE,
                "%s: workspace missing, too small or not 8-byte aligned (it is the one stm_mbox_positives filled)", who);
    const MbLayout L = mb_layout(B, P);
    const unsigned* ws = reinterpret_cast<const unsigned*>(workspace);
    const int tpi = stm_cdiv(P, PL_TILE);
    hipLaunchKernelGGL(mbox_scatter_kernel, dim3(B * tpi), dim3(256), 0, stm_hs(stream), grad_rows, conf_t, ws + L.tilepre, n_dev, status,
                       grad_mask_data, n_rows, P, tpi, M);
    STM_CHECK_LAUNCH("mbox_scatter_kernel");
    return STM_OK;
}
