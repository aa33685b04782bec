// mask_backward.hip -- backward of two of the layer functions the reference's loss differentiates through (layers/modules/multibox_loss.py):
// decode (stm_decode_boxes_f32) and jaccard (stm_jaccard_f32), fp32, for gfx950.  generate_mask's adjoints are in lincomb_backward.hip.
#include "stm_common.h"

namespace {

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
