/* dp_step.h -- the finish of a data-parallel training step (stmask_amd/optim.py: DataParallelSGD), gfx950 (MI355X).
 *
 * Package-private: exported by libstmask_hip.so, restated in stmask_amd/_lib.py DP_SIGNATURES and bound on first use by _lib.private_call().
 * Not part of the drop-in boundary of include/ (no C client of that boundary runs an optimizer), so STM_ABI_VERSION does not count it.
 *
 * The entry is stm_sgd_step_multi_f32 of optim.h in the same table form: host arrays of `count` device pointers and element counts,
 * 1 <= count <= STM_DP_MAX_TENSORS, the table by value in the kernel arguments, one workgroup per chunk of STM_DP_CHUNK elements, 16-byte accesses
 * where the three addresses of a chunk allow and 4-byte accesses for its last n % 4 elements and for a tensor at an odd offset.  No LDS, no
 * scratch, no atomics.  A tensor of n[i] == 0 elements may have NULL pointers.
 *
 * Refused before any launch: count < 1, n[i] < 0, a NULL pointer of a tensor with elements, a NULL array, lr / mu / wd not finite, inv_world not
 * in (0, 1], NULL counters (STM_EINVAL); count > STM_DP_MAX_TENSORS, 2^31 chunks or more in one call (STM_EUNSUPPORTED). */
#pragma once
#include <stdint.h>

#include "../../include/stmask_hip.h"
#include "chunk_table.h"

#define STM_DP_MAX_TENSORS STM_CHUNK_MAX_ROWS
#define STM_DP_CHUNK STM_CHUNK_ELEMS

#ifdef __cplusplus
extern "C" {
#endif

/* g holds the SUM of the ranks' gradients (the all-reduced arena).  Per element, in IEEE fp32, unfused, in this order:
 *     s = g;   g = 0.0f;   ga = s * inv_world;   g' = ga + wd * p;   m = mu * m + g';   p = p - lr * m
 * inv_world is the fp32 value of 1 / world, computed by the caller.  Every element of g that the launch covers is overwritten with 0.0f, also
 * when the guard skips the step: the next backward pass accumulates from zero and a NaN does not survive the iteration.
 * Guard: every workgroup first reads loss_sum[0] (the reduced sum of the ranks' losses; may be NULL) and bad[0] (int32, may be NULL); if the sum
 * is not finite or bad != 0 the launch leaves p and m untouched.  Both are functions of the reduced buffer alone, so every rank decides alike.
 * first_launch != 0 (the first launch of an optimizer step): one thread adds 1 to counters[0] (applied) or counters[1] (skipped), a plain load
 * and store -- the launches of a stream are ordered.  loss_sum, bad and counters are device pointers; loss_sum may point into the arena that g
 * points into, outside every tensor of the table. */
int stm_dp_sgd_finish_multi_f32(float* const* p, float* const* g, float* const* m, const int64_t* n, int count, const float* loss_sum,
                                const int* bad, int* counters, int first_launch, float inv_world, float lr, float mu, float wd,
                                stm_stream_t stream);

#ifdef __cplusplus
}
#endif
