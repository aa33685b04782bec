// mask_backward.hip -- backward of the three layer functions the reference's loss differentiates through (layers/modules/multibox_loss.py):
// generate_mask (stm_lincomb_sigmoid_crop_f32), decode (stm_decode_boxes_f32) and jaccard (stm_jaccard_f32), fp32, for gfx950.
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
//   No float atomics anywhere: the pixel blocks' partial grad_coeff [pixel block][n][M] are added in block order by lincomb_gc_reduce_kernel
//   (which applies 1 - t^2), and when the rows are split over several workgroups per pixel block (60 pixel blocks at 96x160 would leave
//   three quarters of the CUs idle) the splits' partial grad_proto [split][hw][M] are added in split order by lincomb_gp_reduce_kernel.
//   Both gradients are therefore bit-identical from run to run.
#include "stm_common.h"

namespace {

constexpr int LB_DCHUNK = 16;      // rows per LDS chunk
constexpr int LB_ZLD = 20;         // floats per pixel of the z tile: 16 rows + 4 of padding (80-byte pitch: the 16-byte writes of 8 lanes hit 32 distinct banks)
constexpr int LB_MAX_SPLITS = 8;   // most row splits per pixel block (bounds the grad_proto partials: 8 x hw x M floats)

template <int M, bool WANT_P, bool WANT_C>
__global__ __launch_bounds__(256) void lincomb_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ proto,
                                                               const float* __restrict__ coeff, const float* __restrict__ boxes,
                                                               float* __restrict__ gp_out, float* __restrict__ gc_part, int h, int w, int n,
                                                               int apply_tanh, int rows_per_split)
{
    constexpr int G = 256 / M;                       // pixel groups of the grad_coeff layout
    static_assert(256 % M == 0 && M % 4 == 0 && 256 * LB_ZLD >= 256 * LB_DCHUNK, "layout");
    __shared__ float sc[LB_DCHUNK * M];
    __shared__ float sb[LB_DCHUNK * 4];              // x1, x2, y1, y2 (float bounds, padding 1)
    __shared__ int hit[LB_DCHUNK];
    __shared__ __attribute__((aligned(16))) float zr[256 * LB_ZLD];   // z tile [pixel][row]; then the groups' sums [group][row][k]
    const int hw = h * w;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * 256;
    const int pix = p0 + tid;
    const bool live = pix < hw;
    const int r0 = blockIdx.y * rows_per_split, r1 = min(n, r0 + rows_per_split);
    const int y = pix / w, x = pix - y * w;
    const float fx = (float)x, fy = (float)y;

    float p[M], gp[M];
    if (live) {
        const float4* pr = reinterpret_cast<const float4*>(proto + (int64_t)pix * M);
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

    const int kk = tid % M, g = tid / M;             // the grad_coeff layout: prototype kk of pixels p0 + g*M + j
    float pq[WANT_C ? M : 1];
    if (WANT_C) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int pj = p0 + g * M + j;
            pq[WANT_C ? j : 0] = pj < hw ? proto[(int64_t)pj * M + kk] : 0.0f;
        }
    }

    for (int c0 = r0; c0 < r1; c0 += LB_DCHUNK) {
        const int nd = min(LB_DCHUNK, r1 - c0);
        __syncthreads();                             // the previous chunk's readers of sc / sb / hit / zr are done
        for (int idx = tid; idx < nd * M; idx += 256) {
            const float v = coeff[(int64_t)c0 * M + idx];
            sc[idx] = apply_tanh ? tanhf(v) : v;
        }
        if (tid < LB_DCHUNK) {
            int touch = 0;
            if (tid < nd) {
                float x1 = 0.f, x2 = (float)w, y1 = 0.f, y2 = (float)h;
                if (boxes) {
                    const float* b = boxes + (int64_t)(c0 + tid) * 4;
                    stm_sanitize(b[0], b[2], w, 1, x1, x2);
                    stm_sanitize(b[1], b[3], h, 1, y1, y2);
                }
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

        int hit4[LB_DCHUNK / 4];
#pragma unroll
        for (int d4 = 0; d4 < LB_DCHUNK / 4; ++d4) {
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
                        float a = 0.0f;
#pragma unroll
                        for (int k = 0; k < M; ++k) a = fmaf(p[k], sc[d * M + k], a);
                        const float e = expf(-fabsf(a));
                        const float ope = 1.0f + e;
                        z = grad_out[(int64_t)(c0 + d) * hw + pix] * (e / (ope * ope));
                        if (WANT_P) {
#pragma unroll
                            for (int k = 0; k < M; ++k) gp[k] = fmaf(z, sc[d * M + k], gp[k]);
                        }
                    }
                }
                zz[r] = z;
            }
            if (WANT_C) *reinterpret_cast<float4*>(&zr[tid * LB_ZLD + 4 * d4]) = make_float4(zz[0], zz[1], zz[2], zz[3]);
        }

        if (WANT_C) {
            __syncthreads();
            float acc[LB_DCHUNK];
#pragma unroll
            for (int d = 0; d < LB_DCHUNK; ++d) acc[d] = 0.0f;
#pragma unroll
            for (int d4 = 0; d4 < LB_DCHUNK / 4; ++d4) {
                if (!hit4[d4]) continue;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const float4 z4 = *reinterpret_cast<const float4*>(&zr[(g * M + j) * LB_ZLD + 4 * d4]);
                    const float pv = pq[WANT_C ? j : 0];
                    acc[4 * d4 + 0] = fmaf(z4.x, pv, acc[4 * d4 + 0]);
                    acc[4 * d4 + 1] = fmaf(z4.y, pv, acc[4 * d4 + 1]);
                    acc[4 * d4 + 2] = fmaf(z4.z, pv, acc[4 * d4 + 2]);
                    acc[4 * d4 + 3] = fmaf(z4.w, pv, acc[4 * d4 + 3]);
                }
            }
            __syncthreads();                         // every read of the z tile is done: the groups' sums take its place
#pragma unroll
            for (int d = 0; d < LB_DCHUNK; ++d) zr[(g * LB_DCHUNK + d) * M + kk] = acc[d];
            __syncthreads();
            for (int idx = tid; idx < nd * M; idx += 256) {
                const int d = idx / M, k2 = idx - d * M;
                float s = 0.0f;
#pragma unroll
                for (int g2 = 0; g2 < G; ++g2) s += zr[(g2 * LB_DCHUNK + d) * M + k2];
                gc_part[((int64_t)blockIdx.x * n + c0) * M + idx] = s;
            }
        }
    }
    if (WANT_P && live) {
        float4* o = reinterpret_cast<float4*>(gp_out + ((int64_t)blockIdx.y * hw + pix) * M);
#pragma unroll
        for (int q = 0; q < M / 4; ++q) o[q] = make_float4(gp[4 * q], gp[4 * q + 1], gp[4 * q + 2], gp[4 * q + 3]);
    }
}

// grad_coeff[i] = (sum over the pixel blocks, in block order, of part[b][i]) * (1 - tanh(coeff[i])^2)
__global__ void lincomb_gc_reduce_kernel(const float* __restrict__ part, const float* __restrict__ coeff, float* __restrict__ grad_coeff,
                                         int64_t total, int blocks, int apply_tanh)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float s = 0.0f;
    for (int b0 = 0; b0 < blocks; b0 += 8) {                 // 8 loads in flight, added in block order (one dependent load per block took 15 us at 60 blocks)
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = b0 + j < blocks ? part[(int64_t)(b0 + j) * total + i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    if (apply_tanh) {                                        // 1 - tanh(c)^2 = 4 e / (1 + e)^2, e = exp(-2 |c|): no cancellation where tanh is near 1
        const float e = expf(-2.0f * fabsf(coeff[i]));
        const float ope = 1.0f + e;
        s = s * (4.0f * e / (ope * ope));
    }
    grad_coeff[i] = s;
}

// grad_proto = sum over the row splits, in split order, of part[s]; 4 floats per thread
__global__ void lincomb_gp_reduce_kernel(const float4* __restrict__ part, float4* __restrict__ grad_proto, int64_t total4, int splits)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    float4 s = part[i];
    for (int b = 1; b < splits; ++b) {
        const float4 v = part[(int64_t)b * total4 + i];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    grad_proto[i] = s;
}

int lb_splits(int n, int hw)
{
    // rows are split over workgroups until the grid has ~2 workgroups per CU, at most LB_MAX_SPLITS ways and never finer than one LDS chunk
    const int pb = stm_cdiv(hw, 256), chunks = stm_cdiv(n, LB_DCHUNK);
    int s = std::min(std::min(chunks, LB_MAX_SPLITS), std::max(1, 512 / pb));
    const int forced = STM_ENV_INT("STM_LCB_SPLITS", 0);    // A/B: scripts/bench_mask_backward.py
    if (forced > 0) s = std::min(std::min(chunks, LB_MAX_SPLITS), forced);
    return s;
}

template <int M>
void lb_launch(bool want_p, bool want_c, dim3 grid, hipStream_t st, const float* go, const float* proto, const float* coeff, const float* boxes,
               float* gp_out, float* gc_part, int h, int w, int n, int apply_tanh, int rows_per_split)
{
    if (want_p && want_c)
        hipLaunchKernelGGL((lincomb_backward_kernel<M, true, true>), grid, dim3(256), 0, st, go, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
    else if (want_p)
        hipLaunchKernelGGL((lincomb_backward_kernel<M, true, false>), grid, dim3(256), 0, st, go, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
    else
        hipLaunchKernelGGL((lincomb_backward_kernel<M, false, true>), grid, dim3(256), 0, st, go, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
}

// ------------------------------------------------------------------------------------------ decode
// The forward and its adjoint are stm_decode_one / stm_decode_one_adjoint of stm_common.h (pos_loss.hip uses the same expressions).
__global__ void decode_backward_kernel(const float4* __restrict__ grad_boxes, const float4* __restrict__ loc, const float4* __restrict__ priors,
                                       float4* __restrict__ grad_loc, float4* __restrict__ grad_priors, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 gl, gp;
    stm_decode_one_adjoint(grad_boxes[i], loc[i], priors[i], gl, gp);
    if (grad_loc) grad_loc[i] = gl;
    if (grad_priors) grad_priors[i] = gp;
}

// ------------------------------------------------------------------------------------------ jaccard
// The pair's adjoint with its tie and clamp conventions is stm_iou_adjoint of stm_common.h.
// grad_a: one wave per row of a; lane l adds columns l, l + 64, ... in that order, then the lanes are added in the fixed order of stm_wave_sum
__global__ __launch_bounds__(256) void jaccard_backward_a_kernel(const float* __restrict__ grad_out, const float4* __restrict__ a, int na,
                                                                 const float4* __restrict__ b, int nb, float4* __restrict__ grad_a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= na) return;                                   // wave-uniform
    const float4 ai = a[i];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = lane; j < nb; j += 64) {
        float4 da, db;
        stm_iou_adjoint(ai, b[j], grad_out[(int64_t)i * nb + j], da, db);
        s.x += da.x; s.y += da.y; s.z += da.z; s.w += da.w;
    }
    s.x = stm_wave_sum(s.x); s.y = stm_wave_sum(s.y); s.z = stm_wave_sum(s.z); s.w = stm_wave_sum(s.w);
    if (lane == 0) grad_a[i] = s;
}

// grad_b: one thread per column of b walking the rows of a in order (the reads of grad_out coalesce across the threads)
__global__ void jaccard_backward_b_kernel(const float* __restrict__ grad_out, const float4* __restrict__ a, int na, const float4* __restrict__ b,
                                          int nb, float4* __restrict__ grad_b)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const float4 bj = b[j];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < na; ++i) {
        float4 da, db;
        stm_iou_adjoint(a[i], bj, grad_out[(int64_t)i * nb + j], da, db);
        s.x += db.x; s.y += db.y; s.z += db.z; s.w += db.w;
    }
    grad_b[j] = s;
}

}  // namespace

extern "C" size_t stm_lincomb_backward_workspace_bytes(int n, int h, int w, int m)
{
    if (n <= 0 || h <= 0 || w <= 0 || m <= 0) return 64;
    const int64_t hw = (int64_t)h * w;
    const size_t pb = (size_t)((hw + 255) / 256);
    const size_t splits = (size_t)std::min(stm_cdiv(n, LB_DCHUNK), LB_MAX_SPLITS);
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
    STM_REQUIRE((uintptr_t)proto % 16 == 0 && (uintptr_t)grad_proto % 16 == 0 && (uintptr_t)workspace % 16 == 0, STM_EINVAL,
                "stm_lincomb_backward_f32: proto, grad_proto and the workspace must be 16-byte aligned");
    STM_REQUIRE(workspace && workspace_bytes >= stm_lincomb_backward_workspace_bytes(n, h, w, m), STM_EWORKSPACE,
                "stm_lincomb_backward_f32: workspace too small");
    const int pb = stm_cdiv(hw, 256);
    const int splits = lb_splits(n, hw);
    const int rows_per_split = stm_cdiv(stm_cdiv(n, LB_DCHUNK), splits) * LB_DCHUNK;
    const int ny = stm_cdiv(n, rows_per_split);              // <= splits; every split holds at least one row
    float* gc_part = reinterpret_cast<float*>(workspace);
    float* gp_part = gc_part + (size_t)pb * n * m;           // pb * n * m * 4 bytes: a multiple of 16 (m % 4 == 0)
    float* gp_out = ny > 1 ? gp_part : grad_proto;
    const dim3 grid(pb, ny);
    const bool wp = grad_proto != nullptr, wc = grad_coeff != nullptr;
    hipStream_t st = stm_hs(stream);
    if (m == 32) lb_launch<32>(wp, wc, grid, st, grad_out, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
    else if (m == 8) lb_launch<8>(wp, wc, grid, st, grad_out, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
    else lb_launch<64>(wp, wc, grid, st, grad_out, proto, coeff, boxes, gp_out, gc_part, h, w, n, apply_tanh, rows_per_split);
    STM_CHECK_LAUNCH("lincomb_backward_kernel");
    if (wc) {
        const int64_t total = (int64_t)n * m;
        hipLaunchKernelGGL(lincomb_gc_reduce_kernel, dim3(stm_cdiv(total, 256)), dim3(256), 0, st, gc_part, coeff, grad_coeff, total, pb, apply_tanh);
        STM_CHECK_LAUNCH("lincomb_gc_reduce_kernel");
    }
    if (wp && ny > 1) {
        const int64_t total4 = (int64_t)hw * m / 4;
        hipLaunchKernelGGL(lincomb_gp_reduce_kernel, dim3(stm_cdiv(total4, 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(gp_part),
                           reinterpret_cast<float4*>(grad_proto), total4, ny);
        STM_CHECK_LAUNCH("lincomb_gp_reduce_kernel");
    }
    return STM_OK;
}

extern "C" int stm_decode_boxes_backward_f32(const float* grad_boxes, const float* loc, const float* priors, float* grad_loc, float* grad_priors,
                                             int64_t n, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0, STM_EINVAL, "stm_decode_boxes_backward_f32: n=%lld", (long long)n);
    if (n == 0 || (!grad_loc && !grad_priors)) return STM_OK;
    STM_REQUIRE(grad_boxes && loc && priors, STM_ENULL, "stm_decode_boxes_backward_f32: grad_boxes/loc/priors must be non-NULL");
    STM_REQUIRE((uintptr_t)grad_boxes % 16 == 0 && (uintptr_t)loc % 16 == 0 && (uintptr_t)priors % 16 == 0 && (uintptr_t)grad_loc % 16 == 0 &&
                    (uintptr_t)grad_priors % 16 == 0, STM_EINVAL, "stm_decode_boxes_backward_f32: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(decode_backward_kernel, dim3(stm_cdiv(n, 256)), dim3(256), 0, stm_hs(stream), reinterpret_cast<const float4*>(grad_boxes),
                       reinterpret_cast<const float4*>(loc), reinterpret_cast<const float4*>(priors), reinterpret_cast<float4*>(grad_loc),
                       reinterpret_cast<float4*>(grad_priors), n);
    STM_CHECK_LAUNCH("decode_backward_kernel");
    return STM_OK;
}

extern "C" int stm_jaccard_backward_f32(const float* grad_out, const float* a, int na, const float* b, int nb, float* grad_a, float* grad_b,
                                        stm_stream_t stream)
{
    STM_REQUIRE(na >= 0 && nb >= 0, STM_EINVAL, "stm_jaccard_backward_f32: negative size");
    if (!grad_a && !grad_b) return STM_OK;
    if (na == 0 || nb == 0) {                                // an empty sum
        if (grad_a && na > 0) (void)hipMemsetAsync(grad_a, 0, sizeof(float) * 4 * (size_t)na, stm_hs(stream));
        if (grad_b && nb > 0) (void)hipMemsetAsync(grad_b, 0, sizeof(float) * 4 * (size_t)nb, stm_hs(stream));
        return STM_OK;
    }
    STM_REQUIRE(grad_out && a && b, STM_ENULL, "stm_jaccard_backward_f32: grad_out/a/b must be non-NULL");
    STM_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && (uintptr_t)grad_a % 16 == 0 && (uintptr_t)grad_b % 16 == 0, STM_EINVAL,
                "stm_jaccard_backward_f32: boxes and their gradients must be 16-byte aligned");
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    if (grad_a) {
        hipLaunchKernelGGL(jaccard_backward_a_kernel, dim3(stm_cdiv(na, 4)), dim3(256), 0, stm_hs(stream), grad_out, a4, na, b4, nb,
                           reinterpret_cast<float4*>(grad_a));
        STM_CHECK_LAUNCH("jaccard_backward_a_kernel");
    }
    if (grad_b) {
        hipLaunchKernelGGL(jaccard_backward_b_kernel, dim3(stm_cdiv(nb, 256)), dim3(256), 0, stm_hs(stream), grad_out, a4, na, b4, nb,
                           reinterpret_cast<float4*>(grad_b));
        STM_CHECK_LAUNCH("jaccard_backward_b_kernel");
    }
    return STM_OK;
}
