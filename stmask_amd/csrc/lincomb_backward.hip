// lincomb_backward.hip -- every adjoint of generate_mask (stm_lincomb_sigmoid_crop_f32 and its row-prototype form), fp32, for gfx950.  This file
// is the only place the mask adjoint arithmetic lives: the crop rectangle, the workgroup-span test, the two derivative forms and the fmaf chain
// are written once (the lc_* helpers below) and the three kernels are held to each other bit for bit by the tests.
//   stm_lincomb_backward_f32             one prototype set: grad_proto and / or grad_coeff (lincomb_backward_kernel)
//   stm_lincomb_rows_backward_f32        a prototype set per row: grad_coeff (lincomb_rows_backward_kernel)
//   stm_lincomb_rows_proto_backward_f32  a prototype set per image, its rows prefix[b] .. prefix[b + 1]: grad_proto (rows_proto_backward_kernel)
//
// Lincomb backward.  With t = tanh(coeff) (or coeff), a = proto . t_d, s = sigmoid(a):
//     z[d,pix]        = grad_out[d,pix] * s (1 - s)   inside row d's crop rectangle (the forward's stm_sanitize, padding 1), 0 outside
//     grad_proto[pix] = sum_d   z[d,pix] * t[d]
//     grad_coeff[d]   = (sum_pix z[d,pix] * proto[pix]) * (1 - t^2)
//   Only inputs are read: s is recomputed.  s (1 - s) = e / (1 + e)^2 with e = exp(-|a|) (the form of deform_backward.hip: no cancellation near
//   s = 1, no overflow).  grad_out is not loaded outside the rectangle (the reference's BCE leaves ~-1e12 there).
//   As in the forward one thread is one prototype pixel with its M prototype values in registers, and a workgroup of 256 pixels walks rows in
//   chunks of 16 whose tanh(coeff) and rectangles sit in LDS; rows whose rectangle misses the workgroup's pixel span are skipped.
//     grad_proto: M register accumulators per pixel, rows added in row order.
//     grad_coeff: a sum over PIXELS, i.e. across the workgroup.  A wave reduction per (row, k) would cost ~8 DPP / VALU steps for every product;
//       instead the chunk's z goes to LDS as [pixel][row] and the workgroup turns to a second layout: thread (g, k) owns prototype k of the M
//       pixels g*M .. g*M+M-1 (their M values in registers, loaded once) and adds z * proto over them in pixel order for the 16 rows; the
//       256 / M groups are then added in group order through LDS.  One FMA and a quarter of a broadcast ds_read_b128 per product.
//   No float atomics anywhere: the pixel blocks' partial grad_coeff [pixel block][n][M] are added in block order by lc_gc_reduce_kernel
//   (which applies 1 - t^2), and when the rows are split over several workgroups per pixel block (60 pixel blocks at 96x160 would leave
//   three quarters of the CUs idle) the splits' partial grad_proto [split][hw][M] are added in split order by lc_split_sum_kernel.
//   Both gradients are therefore bit-identical from run to run.
// Row form (2 launches): grid (pixel blocks of 256, rows), one row per workgroup.  A workgroup whose pixel span misses the row's rectangle
//   writes M zeros and leaves; otherwise the products z * proto are added per group of M pixels in pixel order and the 256 / M groups in group
//   order, which is the order of lincomb_backward_kernel: with one prototype set the result equals stm_lincomb_backward_f32's bit for bit.
//   Rows past the device-side live count n_dev get zeros from the reduce, which does not read their partials.
// Row-prototype form (1 or 2 launches): lincomb_backward_kernel's grad_proto layout on a grid (pixel blocks, images, row splits); a workgroup
//   reads its image's row range on the device and walks it in row order.  The number of splits depends on h, w and the number of images only
//   (never on the number of rows), so the exact and the padded form make the same sums.  An image without positives gets exact zeros; a set
//   status word turns every output into NaN.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no kernel of this file uses scratch.
#include "stm_common.h"
#include "../../include/stmask_hip_train.h"
#include <type_traits>

namespace {

constexpr int LC_DCHUNK = 16;        // rows per LDS chunk
constexpr int LC_ZLD = 20;           // floats per pixel of the z tile: 16 rows + 4 of padding (80-byte pitch: the 16-byte writes of 8 lanes hit 32 distinct banks)
constexpr int LC_MAX_SPLITS = 8;     // most row splits per pixel block (bounds the grad_proto partials: 8 x hw x M floats per set)
constexpr int LC_MAX_ROWS = 65535;   // rows (and prototype sets) a grid's y takes; t2s_loss.hip's TS_MAX_ROWS and mbox_loss.hip's MB_MAX_ROWS are this value

struct LcRect {
    float x1, x2, y1, y2;            // float bounds, padding 1
};

// row r's crop rectangle; a null boxes is the whole image
__device__ __forceinline__ LcRect lc_rect(const float* boxes, int64_t r, int h, int w)
{
    LcRect c = {0.f, (float)w, 0.f, (float)h};
    if (boxes) {
        const float* b = boxes + r * 4;
        stm_sanitize(b[0], b[2], w, 1, c.x1, c.x2);
        stm_sanitize(b[1], b[3], h, 1, c.y1, c.y2);
    }
    return c;
}

// does the rectangle touch the pixel span p0 .. p0 + 255 at all (the forward's test)
__device__ __forceinline__ bool lc_touches(const LcRect& c, int p0, int hw, int w)
{
    const int pl = min(p0 + 255, hw - 1);
    const int ya = p0 / w, yb = pl / w;
    bool t = (float)yb >= c.y1 && (float)ya < c.y2;
    if (t && ya == yb) t = (float)(pl - ya * w) >= c.x1 && (float)(p0 - ya * w) < c.x2;
    return t;
}

// s (1 - s) = e / (1 + e)^2, e = exp(-|a|): no cancellation near s = 1, no overflow
__device__ __forceinline__ float lc_dsigmoid(float a)
{
    const float e = expf(-fabsf(a));
    const float ope = 1.0f + e;
    return e / (ope * ope);
}

// 1 - tanh(c)^2 = 4 e / (1 + e)^2, e = exp(-2 |c|): no cancellation where tanh is near 1
__device__ __forceinline__ float lc_dtanh(float c)
{
    const float e = expf(-2.0f * fabsf(c));
    const float ope = 1.0f + e;
    return 4.0f * e / (ope * ope);
}

// a pixel's M values (at src) into registers; zeros for a dead pixel
template <int M>
__device__ __forceinline__ void lc_load_pixel(const float* src, bool live, float (&p)[M])
{
    if (live) {
        const float4* pr = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int q = 0; q < M / 4; ++q) {
            const float4 v = pr[q];
            p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < M; ++k) p[k] = 0.0f;
    }
}

template <int M>
__device__ __forceinline__ void lc_store_pixel(float* dst, const float (&v)[M])
{
    float4* o = reinterpret_cast<float4*>(dst);
#pragma unroll
    for (int q = 0; q < M / 4; ++q) o[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// z of a pixel INSIDE the row's rectangle: p the pixel's prototype values, t the row's M coefficients (LDS), go the pixel's grad_out
template <int M>
__device__ __forceinline__ float lc_z(const float (&p)[M], const float* t, const float* go)
{
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < M; ++k) a = fmaf(p[k], t[k], a);
    return *go * lc_dsigmoid(a);
}

// The rectangles of rows c0 .. c0 + nd - 1 into LDS: sb (x1, x2, y1, y2), and hit: does the rectangle touch the workgroup's span p0 .. p0 + 255
// (0 for the rows past nd).  The chunk's coefficients are staged by a loop of the kernel's own: with that loop in here the compiler vectorises
// lincomb_backward_kernel<8>'s group sums and the kernel loses a wave of occupancy.
__device__ __forceinline__ void lc_stage_chunk(float* sb, int* hit, const float* boxes, int c0, int nd, int p0, int h, int w)
{
    const int tid = threadIdx.x;
    if (tid < LC_DCHUNK) {
        int touch = 0;
        if (tid < nd) {
            const LcRect c = lc_rect(boxes, c0 + tid, h, w);
            sb[tid * 4 + 0] = c.x1;
            sb[tid * 4 + 1] = c.x2;
            sb[tid * 4 + 2] = c.y1;
            sb[tid * 4 + 3] = c.y2;
            touch = lc_touches(c, p0, h * w, w) ? 1 : 0;
        }
        hit[tid] = touch;
    }
}

// ------------------------------------------------------------------------------------------ one prototype set
template <int M, bool WANT_P, bool WANT_C>
__global__ __launch_bounds__(256) void lincomb_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ proto,
                                                               const float* __restrict__ coeff, const float* __restrict__ boxes,
                                                               float* __restrict__ gp_out, float* __restrict__ gc_part, int h, int w, int n,
                                                               int apply_tanh, int rows_per_split)
{
    constexpr int G = 256 / M;                       // pixel groups of the grad_coeff layout
    static_assert(256 % M == 0 && M % 4 == 0 && 256 * LC_ZLD >= 256 * LC_DCHUNK, "layout");
    __shared__ float sc[LC_DCHUNK * M];
    __shared__ float sb[LC_DCHUNK * 4];
    __shared__ int hit[LC_DCHUNK];
    __shared__ __attribute__((aligned(16))) float zr[256 * LC_ZLD];   // z tile [pixel][row]; then the groups' sums [group][row][k]
    const int hw = h * w;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * 256;
    const int pix = p0 + tid;
    const bool live = pix < hw;
    const int r0 = blockIdx.y * rows_per_split, r1 = min(n, r0 + rows_per_split);
    const int y = pix / w, x = pix - y * w;
    const float fx = (float)x, fy = (float)y;

    float p[M], gp[M];
    lc_load_pixel<M>(proto + (int64_t)pix * M, live, p);
#pragma unroll
    for (int k = 0; k < M; ++k) gp[k] = 0.0f;

    const int kk = tid % M, g = tid / M;             // the grad_coeff layout: prototype kk of pixels p0 + g*M + j
    float pq[WANT_C ? M : 1];
    if (WANT_C) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int pj = p0 + g * M + j;
            pq[WANT_C ? j : 0] = pj < hw ? proto[(int64_t)pj * M + kk] : 0.0f;
        }
    }

    for (int c0 = r0; c0 < r1; c0 += LC_DCHUNK) {
        const int nd = min(LC_DCHUNK, r1 - c0);
        __syncthreads();                             // the previous chunk's readers of sc / sb / hit / zr are done
        for (int idx = tid; idx < nd * M; idx += 256) {
            const float v = coeff[(int64_t)c0 * M + idx];
            sc[idx] = apply_tanh ? tanhf(v) : v;
        }
        lc_stage_chunk(sb, hit, boxes, c0, nd, p0, h, w);
        __syncthreads();

        int hit4[LC_DCHUNK / 4];
#pragma unroll
        for (int d4 = 0; d4 < LC_DCHUNK / 4; ++d4) {
            hit4[d4] = hit[4 * d4] | hit[4 * d4 + 1] | hit[4 * d4 + 2] | hit[4 * d4 + 3];
            if (!hit4[d4]) continue;                 // workgroup-uniform
            float zz[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 4 * d4 + r;
                float z = 0.0f;
                if (hit[d]) {
                    const bool inside = live && fx >= sb[d * 4] && fx < sb[d * 4 + 1] && fy >= sb[d * 4 + 2] && fy < sb[d * 4 + 3];
                    if (inside) {
                        z = lc_z<M>(p, sc + d * M, grad_out + (int64_t)(c0 + d) * hw + pix);
                        if (WANT_P) {
#pragma unroll
                            for (int k = 0; k < M; ++k) gp[k] = fmaf(z, sc[d * M + k], gp[k]);
                        }
                    }
                }
                zz[r] = z;
            }
            if (WANT_C) *reinterpret_cast<float4*>(&zr[tid * LC_ZLD + 4 * d4]) = make_float4(zz[0], zz[1], zz[2], zz[3]);
        }

        if (WANT_C) {
            __syncthreads();
            float acc[LC_DCHUNK];
#pragma unroll
            for (int d = 0; d < LC_DCHUNK; ++d) acc[d] = 0.0f;
#pragma unroll
            for (int d4 = 0; d4 < LC_DCHUNK / 4; ++d4) {
                if (!hit4[d4]) continue;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const float4 z4 = *reinterpret_cast<const float4*>(&zr[(g * M + j) * LC_ZLD + 4 * d4]);
                    const float pv = pq[WANT_C ? j : 0];
                    acc[4 * d4 + 0] = fmaf(z4.x, pv, acc[4 * d4 + 0]);
                    acc[4 * d4 + 1] = fmaf(z4.y, pv, acc[4 * d4 + 1]);
                    acc[4 * d4 + 2] = fmaf(z4.z, pv, acc[4 * d4 + 2]);
                    acc[4 * d4 + 3] = fmaf(z4.w, pv, acc[4 * d4 + 3]);
                }
            }
            __syncthreads();                         // every read of the z tile is done: the groups' sums take its place
#pragma unroll
            for (int d = 0; d < LC_DCHUNK; ++d) zr[(g * LC_DCHUNK + d) * M + kk] = acc[d];
            __syncthreads();
            for (int idx = tid; idx < nd * M; idx += 256) {
                const int d = idx / M, k2 = idx - d * M;
                float s = 0.0f;
#pragma unroll
                for (int g2 = 0; g2 < G; ++g2) s += zr[(g2 * LC_DCHUNK + d) * M + k2];
                gc_part[((int64_t)blockIdx.x * n + c0) * M + idx] = s;
            }
        }
    }
    if (WANT_P && live) lc_store_pixel<M>(gp_out + ((int64_t)blockIdx.y * hw + pix) * M, gp);
}

// ------------------------------------------------------------------------------------------ a prototype set per row: grad_coeff
template <int M>
__global__ __launch_bounds__(256) void lincomb_rows_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ proto,
                                                                    const float* __restrict__ coeff, const float* __restrict__ boxes,
                                                                    const int* __restrict__ row_proto, const int* __restrict__ n_dev,
                                                                    float* __restrict__ part, int h, int w, int n, int n_proto, int apply_tanh)
{
    constexpr int G = 256 / M;
    static_assert(256 % M == 0 && M % 4 == 0, "layout");
    __shared__ float sc[M];
    __shared__ float zs[256];
    __shared__ float gs[256];
    const int r = blockIdx.y;
    const int nv = n_dev ? min(max(*n_dev, 0), n) : n;
    if (r >= nv) return;                                     // workgroup-uniform; the reduce writes this row's zeros without reading part
    const int hw = h * w, tid = threadIdx.x;
    const int p0 = blockIdx.x * 256;
    const LcRect c = lc_rect(boxes, r, h, w);
    float* out = part + ((int64_t)blockIdx.x * n + r) * M;
    if (!lc_touches(c, p0, hw, w)) {                         // workgroup-uniform
        if (tid < M) out[tid] = 0.0f;
        return;
    }
    int set = row_proto ? row_proto[r] : 0;
    set = set < 0 ? 0 : (set >= n_proto ? n_proto - 1 : set);
    const float* pset = proto + (int64_t)set * hw * M;
    if (tid < M) {
        const float v = coeff[(int64_t)r * M + tid];
        sc[tid] = apply_tanh ? tanhf(v) : v;
    }
    __syncthreads();
    const int pix = p0 + tid;
    const int y = pix / w, x = pix - y * w;
    const float fx = (float)x, fy = (float)y;
    float z = 0.0f;
    if (pix < hw && fx >= c.x1 && fx < c.x2 && fy >= c.y1 && fy < c.y2) {
        float p[M];
        lc_load_pixel<M>(pset + (int64_t)pix * M, true, p);
        z = lc_z<M>(p, sc, grad_out + (int64_t)r * hw + pix);
    }
    zs[tid] = z;
    __syncthreads();
    const int kk = tid % M, g = tid / M;                     // prototype kk of pixels p0 + g * M + j, added in pixel order
    float acc = 0.0f;
#pragma unroll 8
    for (int j = 0; j < M; ++j) {
        const int pj = p0 + g * M + j;
        const float pv = pj < hw ? pset[(int64_t)pj * M + kk] : 0.0f;
        acc = fmaf(zs[g * M + j], pv, acc);
    }
    gs[g * M + kk] = acc;
    __syncthreads();
    if (tid < M) {
        float s = 0.0f;
#pragma unroll
        for (int g2 = 0; g2 < G; ++g2) s += gs[g2 * M + tid];
        out[tid] = s;
    }
}

// ------------------------------------------------------------------------------------------ a prototype set per image: grad_proto
template <int M>
__global__ __launch_bounds__(256) void rows_proto_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ proto,
                                                                  const float* __restrict__ coeff, const float* __restrict__ boxes,
                                                                  const int* __restrict__ prefix, const int* __restrict__ status,
                                                                  float* __restrict__ gp_out, int h, int w, int n, int n_proto)
{
    static_assert(M % 4 == 0, "layout");
    __shared__ float sc[LC_DCHUNK * M];
    __shared__ float sb[LC_DCHUNK * 4];
    __shared__ int hit[LC_DCHUNK];
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
    const int per = ((hi - lo + LC_DCHUNK - 1) / LC_DCHUNK + splits - 1) / splits * LC_DCHUNK;   // rows per split: whole chunks
    const int r0 = min(hi, lo + (int)blockIdx.z * per), r1 = min(hi, r0 + per);
    const int y = pix / w, x = pix - y * w;
    const float fx = (float)x, fy = (float)y;

    float p[M], gp[M];
    lc_load_pixel<M>(proto + ((int64_t)set * hw + pix) * M, live, p);
#pragma unroll
    for (int k = 0; k < M; ++k) gp[k] = 0.0f;

    for (int c0 = r0; c0 < r1; c0 += LC_DCHUNK) {
        const int nd = min(LC_DCHUNK, r1 - c0);
        __syncthreads();                             // the previous chunk's readers of sc / sb / hit are done
        for (int i = tid; i < nd * M; i += 256) sc[i] = tanhf(coeff[(int64_t)c0 * M + i]);
        lc_stage_chunk(sb, hit, boxes, c0, nd, p0, h, w);
        __syncthreads();
        for (int d = 0; d < nd; ++d) {
            if (!hit[d]) continue;                   // workgroup-uniform
            const bool inside = live && fx >= sb[d * 4] && fx < sb[d * 4 + 1] && fy >= sb[d * 4 + 2] && fy < sb[d * 4 + 3];
            if (inside) {
                const float z = lc_z<M>(p, sc + d * M, grad_out + (int64_t)(c0 + d) * hw + pix);
#pragma unroll
                for (int k = 0; k < M; ++k) gp[k] = fmaf(z, sc[d * M + k], gp[k]);
            }
        }
    }
    if (live) {
        if (status && *status != 0) {
#pragma unroll
            for (int k = 0; k < M; ++k) gp[k] = stm_nan_f32();
        }
        lc_store_pixel<M>(gp_out + (((int64_t)blockIdx.z * n_proto + set) * hw + pix) * M, gp);
    }
}

// ------------------------------------------------------------------------------------------ the partial sums
// grad_coeff[r] = (sum over the pixel blocks, in block order, of part[b][r]) * (1 - tanh(coeff[r])^2); rows past the live count (n_dev, or
// n where it is null): zeros, without reading part
__global__ __launch_bounds__(256) void lc_gc_reduce_kernel(const float* __restrict__ part, const float* __restrict__ coeff,
                                                           const int* __restrict__ n_dev, float* __restrict__ grad_coeff, int n, int M, int blocks,
                                                           int apply_tanh)
{
    const int64_t total = (int64_t)n * M;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int nv = n_dev ? min(max(*n_dev, 0), n) : n;
    float s = 0.0f;
    if (i / M < nv) {
        for (int b0 = 0; b0 < blocks; b0 += 8) {             // 8 loads in flight, added in block order (one dependent load per block took 15 us at 60 blocks)
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = b0 + j < blocks ? part[(int64_t)(b0 + j) * total + i] : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        if (apply_tanh) s = s * lc_dtanh(coeff[i]);
    }
    grad_coeff[i] = s;
}

// out = sum over the row splits, in split order, of part[s]; 4 floats per thread
__global__ __launch_bounds__(256) void lc_split_sum_kernel(const float4* __restrict__ part, float4* __restrict__ out, int64_t total4, int splits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    float4 s = part[i];
    for (int b = 1; b < splits; ++b) {
        const float4 v = part[(int64_t)b * total4 + i];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    out[i] = s;
}

int lc_launch_gc_reduce(const float* part, const float* coeff, const int* n_dev, float* grad_coeff, int n, int m, int pb, int apply_tanh,
                        hipStream_t st)
{
    hipLaunchKernelGGL(lc_gc_reduce_kernel, dim3(stm_cdiv((int64_t)n * m, 256)), dim3(256), 0, st, part, coeff, n_dev, grad_coeff, n, m, pb,
                       apply_tanh);
    STM_CHECK_LAUNCH("lc_gc_reduce_kernel");
    return STM_OK;
}

int lc_launch_split_sum(const float* part, float* out, int64_t total4, int splits, hipStream_t st)
{
    hipLaunchKernelGGL(lc_split_sum_kernel, dim3(stm_cdiv(total4, 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(part),
                       reinterpret_cast<float4*>(out), total4, splits);
    STM_CHECK_LAUNCH("lc_split_sum_kernel");
    return STM_OK;
}

// The two split rules differ on purpose.
int lb_splits(int n, int hw)
{
    // rows are split over workgroups until the grid has ~2 workgroups per CU, at most LC_MAX_SPLITS ways and never finer than one LDS chunk
    const int pb = stm_cdiv(hw, 256), chunks = stm_cdiv(n, LC_DCHUNK);
    int s = std::min(std::min(chunks, LC_MAX_SPLITS), std::max(1, 512 / pb));
    const int forced = STM_ENV_INT("STM_LCB_SPLITS", 0);    // A/B: scripts/bench_mask_backward.py
    if (forced > 0) s = std::min(std::min(chunks, LC_MAX_SPLITS), forced);
    return s;
}

// ... until the grid has ~2 workgroups per CU; a function of the SHAPES only (not of the number of rows)
int mb_splits(int n_proto, int64_t hw)
{
    const int64_t wgs = (int64_t)stm_cdiv(hw, 256) * n_proto;
    return (int)std::min<int64_t>(LC_MAX_SPLITS, std::max<int64_t>(1, 512 / wgs));
}

// f(std::integral_constant<int, m>) for the mask dimensions the kernels are built for (the callers have refused every other m)
template <class F>
void lc_dispatch_m(int m, F&& f)
{
    if (m == 32) f(std::integral_constant<int, 32>{});
    else if (m == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 64>{});
}

}  // namespace

extern "C" size_t stm_lincomb_backward_workspace_bytes(int n, int h, int w, int m)
{
    if (n <= 0 || h <= 0 || w <= 0 || m <= 0) return 64;
    const int64_t hw = (int64_t)h * w;
    const size_t pb = (size_t)((hw + 255) / 256);
    const size_t splits = (size_t)std::min(stm_cdiv(n, LC_DCHUNK), LC_MAX_SPLITS);
    return (pb * (size_t)n * m + splits * (size_t)hw * m) * sizeof(float) + 64;
}

extern "C" int stm_lincomb_backward_f32(const float* grad_out, const float* proto, const float* coeff, const float* boxes, float* grad_proto,
                                        float* grad_coeff, int h, int w, int m, int n, int apply_tanh, void* workspace, size_t workspace_bytes,
                                        stm_stream_t stream)
{
    STM_REQUIRE(n >= 0, STM_EINVAL, "stm_lincomb_backward_f32: n=%d", n);
    STM_REQUIRE(h > 0 && w > 0 && (int64_t)h * w < (1ll << 31) - 256, STM_EINVAL, "stm_lincomb_backward_f32: bad mask size %dx%d", h, w);
    STM_REQUIRE(m == 8 || m == 32 || m == 64, STM_EUNSUPPORTED, "stm_lincomb_backward_f32: mask_dim %d not in {8,32,64}", m);
    if (!grad_proto && !grad_coeff) return STM_OK;
    const int hw = h * w;
    if (n == 0) {                                            // no rows: the prototypes get a zero gradient
        if (grad_proto) (void)hipMemsetAsync(grad_proto, 0, sizeof(float) * (size_t)hw * m, stm_hs(stream));
        return STM_OK;
    }
    STM_REQUIRE(grad_out && proto && coeff, STM_ENULL, "stm_lincomb_backward_f32: grad_out/proto/coeff must be non-NULL");
    STM_REQUIRE(stm_aligned16(proto) && stm_aligned16(grad_proto) && stm_aligned16(workspace), STM_EINVAL,
                "stm_lincomb_backward_f32: proto, grad_proto and the workspace must be 16-byte aligned");
    STM_REQUIRE(workspace && workspace_bytes >= stm_lincomb_backward_workspace_bytes(n, h, w, m), STM_EWORKSPACE,
                "stm_lincomb_backward_f32: workspace too small");
    const int pb = stm_cdiv(hw, 256);
    const int splits = lb_splits(n, hw);
    const int rows_per_split = stm_cdiv(stm_cdiv(n, LC_DCHUNK), splits) * LC_DCHUNK;
    const int ny = stm_cdiv(n, rows_per_split);              // <= splits; every split holds at least one row
    float* gc_part = reinterpret_cast<float*>(workspace);
    float* gp_part = gc_part + (size_t)pb * n * m;           // pb * n * m * 4 bytes: a multiple of 16 (m % 4 == 0)
    float* gp_out = ny > 1 ? gp_part : grad_proto;
    const dim3 grid(pb, ny);
    const bool wp = grad_proto != nullptr, wc = grad_coeff != nullptr;
    hipStream_t st = stm_hs(stream);
    lc_dispatch_m(m, [&](auto mc) {
        constexpr int M = decltype(mc)::value;
        const auto kernel = wp && wc ? lincomb_backward_kernel<M, true, true>
                            : wp     ? lincomb_backward_kernel<M, true, false>
                                     : lincomb_backward_kernel<M, false, true>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, grad_out, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
    });
    STM_CHECK_LAUNCH("lincomb_backward_kernel");
    if (wc) {
        const int rc = lc_launch_gc_reduce(gc_part, coeff, nullptr, grad_coeff, n, m, pb, apply_tanh, st);
        if (rc != STM_OK) return rc;
    }
    if (wp && ny > 1) return lc_launch_split_sum(gp_part, grad_proto, (int64_t)hw * m / 4, ny, st);
    return STM_OK;
}

extern "C" size_t stm_lincomb_rows_backward_workspace_bytes(int n, int h, int w, int m)
{
    if (n <= 0 || h <= 0 || w <= 0 || m <= 0) return 64;
    const size_t pb = (size_t)(((int64_t)h * w + 255) / 256);
    return pb * (size_t)n * m * sizeof(float) + 64;
}

extern "C" int stm_lincomb_rows_backward_f32(const float* grad_out, const float* proto, int n_proto, const float* coeff, const float* boxes,
                                             const int* row_proto, const int* n_dev, float* grad_coeff, int h, int w, int m, int n, int apply_tanh,
                                             void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_lincomb_rows_backward_f32";
    STM_REQUIRE(n >= 0 && n_proto >= 1, STM_EINVAL, "%s: n=%d n_proto=%d", who, n, n_proto);
    STM_REQUIRE(h > 0 && w > 0 && (int64_t)h * w * n_proto < (1ll << 31) - 256, STM_EINVAL, "%s: bad mask size %dx%d x %d sets", who, h, w, n_proto);
    STM_REQUIRE(m == 8 || m == 32 || m == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, m);
    STM_REQUIRE(n <= LC_MAX_ROWS, STM_EUNSUPPORTED, "%s: n=%d > %d", who, n, LC_MAX_ROWS);
    if (n == 0 || !grad_coeff) return STM_OK;
    STM_REQUIRE(grad_out && proto && coeff, STM_ENULL, "%s: grad_out/proto/coeff must be non-NULL", who);
    STM_REQUIRE(stm_aligned16(proto), STM_EINVAL, "%s: proto must be 16-byte aligned", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_lincomb_rows_backward_workspace_bytes(n, h, w, m) && (uintptr_t)workspace % 4 == 0,
                STM_EWORKSPACE, "%s: workspace missing or too small", who);
    const int pb = stm_cdiv((int64_t)h * w, 256);
    float* part = reinterpret_cast<float*>(workspace);
    const dim3 grid(pb, n);
    hipStream_t st = stm_hs(stream);
    lc_dispatch_m(m, [&](auto mc) {
        hipLaunchKernelGGL((lincomb_rows_backward_kernel<decltype(mc)::value>), grid, dim3(256), 0, st, grad_out, proto, coeff, boxes, row_proto,
                           n_dev, part, h, w, n, n_proto, apply_tanh);
    });
    STM_CHECK_LAUNCH("lincomb_rows_backward_kernel");
    return lc_launch_gc_reduce(part, coeff, n_dev, grad_coeff, n, m, pb, apply_tanh, st);
}

extern "C" size_t stm_lincomb_rows_proto_backward_workspace_bytes(int n_proto, int h, int w, int m)
{
    // the shapes stm_lincomb_rows_proto_backward_f32 refuses: 64
    if (n_proto <= 0 || n_proto > LC_MAX_ROWS || h <= 0 || w <= 0 || !(m == 8 || m == 32 || m == 64)) return 64;
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
    STM_REQUIRE(n >= 1 && n_proto >= 1 && n_proto <= LC_MAX_ROWS, STM_EINVAL, "%s: n=%d n_proto=%d", who, n, n_proto);
    STM_REQUIRE(h > 0 && w > 0 && (int64_t)h * w * n_proto < (1ll << 31) - 256, STM_EINVAL, "%s: bad mask size %dx%d x %d sets", who, h, w, n_proto);
    STM_REQUIRE(m == 8 || m == 32 || m == 64, STM_EUNSUPPORTED, "%s: mask_dim %d not in {8,32,64}", who, m);
    STM_REQUIRE(n <= LC_MAX_ROWS, STM_EUNSUPPORTED, "%s: n=%d > %d", who, n, LC_MAX_ROWS);
    STM_REQUIRE(grad_out && proto && coeff && boxes && prefix && grad_proto, STM_ENULL,
                "%s: grad_out/proto/coeff/boxes/prefix/grad_proto must be non-NULL", who);
    STM_REQUIRE(stm_aligned16(proto) && stm_aligned16(grad_proto) && stm_aligned16(workspace), STM_EINVAL,
                "%s: proto, grad_proto and the workspace must be 16-byte aligned", who);
    const int hw = h * w;
    const int splits = mb_splits(n_proto, hw);
    STM_REQUIRE(splits == 1 || (workspace && workspace_bytes >= stm_lincomb_rows_proto_backward_workspace_bytes(n_proto, h, w, m)), STM_EWORKSPACE,
                "%s: workspace missing or too small", who);
    float* gp_out = splits > 1 ? reinterpret_cast<float*>(workspace) : grad_proto;
    const dim3 grid(stm_cdiv(hw, 256), n_proto, splits);
    hipStream_t st = stm_hs(stream);
    lc_dispatch_m(m, [&](auto mc) {
        hipLaunchKernelGGL((rows_proto_backward_kernel<decltype(mc)::value>), grid, dim3(256), 0, st, grad_out, proto, coeff, boxes, prefix, status,
                           gp_out, h, w, n, n_proto);
    });
    STM_CHECK_LAUNCH("rows_proto_backward_kernel");
    if (splits > 1) return lc_launch_split_sum(gp_out, grad_proto, (int64_t)n_proto * hw * m / 4, splits, st);
    return STM_OK;
}
