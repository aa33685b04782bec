/* det_backward.h -- the deterministic mode of the training backward (stmask_amd/autograd.py: set_deterministic), gfx950 (MI355X).
 *
 * Package-private: exported by libstmask_hip.so, restated in stmask_amd/_lib.py DET_SIGNATURES and bound on first use by _lib.private_call().
 * Not part of the drop-in boundary of include/ (the fp32-atomic entries of stmask_hip.h stay what a C client calls), so STM_ABI_VERSION does
 * not count these.
 *
 * The two scatters of the backward pass -- grad_x of the deformable im2col and grad_feat of RoIAlign -- address exactly the elements
 * stm_deform_col2im_f32 and stm_roi_align_backward_f32 address, with the very fp32 products those add, but accumulate them in 64-bit fixed
 * point with integer atomics (det_accum.h):   grad = fp32( (sum_i rint(t_i * 2^p)) / 2^p ).   Three passes on the stream, no host read:
 *   1  the maximum of |gradient| (and of |mask| for an explicit DCNv2 mask, which is not bounded by 1), as bit patterns, into two words;
 *   2  the scatter; every thread derives the same p from the two words and from q, the bits the shapes leave (det_accum.h);
 *   3  the int64 accumulator to fp32.  The output is written, not accumulated: it need not be cleared.
 * The accumulator and the two words are the workspace: stm_det_workspace_bytes(numel of the output) bytes, 8-byte aligned, cleared by the call.
 * The result does not depend on arrival order, grid shape or channel chunking; it differs from the exact sum of the fp32 terms by at most
 * L * 2^-(p+1) for a destination of L terms, plus the final rounding.
 *
 * Defined for every input, never a fault: a maximum of zero gives exact zeros; an inf or NaN ANYWHERE in the incoming gradient (or the explicit
 * mask), or maxima whose product overflows fp32, makes the WHOLE output NaN -- the atomic entries poison only the elements such a value
 * reaches.  GuardedSGD skips such a step either way.
 *
 * Refused before any launch: what the atomic entries refuse; a NULL, misaligned or too small workspace (STM_EWORKSPACE); shapes that leave
 * q < STM_DET_MIN_BITS (36) bits between the bound of the maximum and the fixed-point unit (STM_EUNSUPPORTED).
 *
 * stm_upsample_bilinear_backward_f32 is the adjoint of F.interpolate(mode="bilinear", align_corners=False) as a gather: one thread per input
 * element, a fixed order, no atomics, no LDS. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/stmask_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The exponent rule on the host (no device needed).  bits_a, bits_b: the bit patterns of the two maxima (sign bit clear; 0x3F800000, 1.0f, for an
 * absent second factor); terms_bound, mass_bound: the largest number of terms and the largest sum of |t_i|, in units of the maximum, one
 * destination can receive.  *state is STM_DET_FINITE (0), STM_DET_ZERO (1) or STM_DET_NONFINITE (2); *p the exponent when it is 0, else 0;
 * *q the bits the bounds leave.  STM_ENULL: a NULL pointer; STM_EINVAL: a negative bit pattern, terms_bound < 0 or mass_bound < 1; STM_EUNSUPPORTED: q < 36. */
int stm_det_exponent(int bits_a, int bits_b, int64_t terms_bound, int64_t mass_bound, int* p, int* state, int* q);

/* bytes of workspace for an output of numel elements: 8 * numel for the accumulator + 8 for the two words (0 for numel < 0) */
size_t stm_det_workspace_bytes(int64_t numel);

/* stm_deform_col2im_f32 with the arguments in its order, then the workspace.  terms_bound = mass_bound = kh * kw * Ho * Wo. */
int stm_deform_col2im_det_f32(const float* grad_cols, const float* offset, int64_t off_bstride, const float* mask, int64_t mask_bstride,
                              int mask_is_logit, float* grad_x, const stm_deform_geom* g, void* workspace, size_t workspace_bytes,
                              stm_stream_t stream);

/* stm_roi_align_backward_f32 with the arguments in its order, then the workspace.  n == 0 writes zeros. */
int stm_roi_align_backward_det_f32(const float* grad_out, const float* rois, float* grad_feat, int B, int C, int H, int W, int n, int PH, int PW,
                                   float spatial_scale, int sampling_ratio, int aligned, void* workspace, size_t workspace_bytes,
                                   stm_stream_t stream);

/* grad_in [planes][h_in][w_in] from grad_out [planes][h_out][w_out], both dense.  Per axis, in fp32, ATen's rule:
 *     scale = scale_factor > 0 ? (float)(1.0 / scale_factor) : (float)in / (float)out
 *     src = max(scale * (o + 0.5f) - 0.5f, 0);   i0 = (int)src;   i1 = i0 + (i0 < in - 1);   l = src - i0;   h = 1 - l
 * and  grad_in[y][x] = sum_oy wy(oy, y) * (sum_ox wx(ox, x) * grad_out[oy][ox]),  w(o, i) = (i0 == i ? h : 0) + (i1 == i ? l : 0), over the
 * outputs whose i0 or i1 is i, rows and columns ascending, every operation rounded once.  Sizes up to 2^20 per axis. */
int stm_upsample_bilinear_backward_f32(const float* grad_out, float* grad_in, int64_t planes, int h_in, int w_in, int h_out, int w_out,
                                       double scale_factor_h, double scale_factor_w, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
