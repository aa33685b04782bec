/* stmask_hip_t2s_feat.h -- T2S_concat_feat, the input of the temporal-fusion loss, and its adjoint: from the interleaved maps of a batch of frame
 * pairs (the reference frame of clip b at image 2 b, the next frame at image 2 b + 1) straight to
 *     relu(cat([leaky_relu(correlation(ref, next) / C, 0.1), t2s_ref, t2s_next], 1)).
 * A sixth header beside stmask_hip.h, stmask_hip_output.h, stmask_hip_tracker.h, stmask_hip_train.h and stmask_hip_eval.h (whose prototype lists
 * and STM_ABI_VERSION are unchanged): new entry points only, same library, same error codes, same stream convention.  INTEGRATION.md section 19
 * restates the contract; stmask_amd/ops.py (t2s_concat_feat, t2s_concat_feat_backward) is the caller.
 *
 * Layout.  fpn [2 bs][C][H][W] and t2s [2 bs][Cu][H][W] fp32, contiguous, read in place through their batch strides;
 * out [bs][P*P + 2 Cu][H][W] with R = P / 2:
 *     channel i * P + j        max(0, (1 / C) * sum_c fpn[2b][c][y][x] * fpn[2b+1][c][y + i - R][x + j - R])     (zero outside the map)
 *     channel P*P + k          max(0, t2s[2b][k])
 *     channel P*P + Cu + k     max(0, t2s[2b+1][k])
 * relu(leaky_relu(v, 0.1)) = max(0, v) exactly, so one clamp stands for both activations.  Every sum runs in channel order (forward) or in
 * displacement order (backward) through one fmaf chain: no atomics, the same bits from run to run.  No workspace, no host synchronisation.
 *
 * Refused before any launch: bs, C, Cu, H or W below 1, an even or non-positive P, P*P*H*W or C*H*W or Cu*H*W >= 2^31, NULL pointers.
 */
#ifndef STMASK_HIP_T2S_FEAT_H
#define STMASK_HIP_T2S_FEAT_H

#include "stmask_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The feature in two launches: the correlation channels, then the copied channels. */
int stm_t2s_feat_forward_f32(const float* fpn, const float* t2s, float* out, int bs, int C, int Cu, int H, int W, int P, stm_stream_t stream);

/* The adjoint in at most three launches.  grad_out and out [bs][P*P + 2 Cu][H][W] (out: what the forward wrote; its sign gates the correlation
 * channels), fpn and t2s the forward's inputs.  With g~ = grad_out * [out > 0]:
 *     grad_fpn[2b][c][y][x]   = (1 / C) * sum_ij g~[ij][y][x] * fpn[2b+1][c][y + dy][x + dx]
 *     grad_fpn[2b+1][c][y][x] = (1 / C) * sum_ij g~[ij][y - dy][x - dx] * fpn[2b][c][y - dy][x - dx]
 *     grad_t2s[2b + k][c]     = grad_out[P*P + k Cu + c] * [t2s[2b + k][c] > 0]
 * grad_fpn [2 bs][C][H][W] and grad_t2s [2 bs][Cu][H][W] are written, not accumulated; either may be NULL and is then not computed (one launch
 * for grad_t2s, two for grad_fpn).  fpn may be NULL when grad_fpn is, t2s when grad_t2s is. */
int stm_t2s_feat_backward_f32(const float* grad_out, const float* out, const float* fpn, const float* t2s, float* grad_fpn, float* grad_t2s,
                              int bs, int C, int Cu, int H, int W, int P, stm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* STMASK_HIP_T2S_FEAT_H */
