/* optim.h -- the optimizer step of the training loop (stmask_amd/optim.py: GuardedSGD), gfx950 (MI355X).
 *
 * Package-private: exported by libstmask_hip.so, restated in stmask_amd/_lib.py PRIVATE_SIGNATURES and bound on first use by _lib.private_call().
 * Not part of the drop-in boundary of include/ (no C client of that boundary runs an optimizer), so STM_ABI_VERSION does not count these.
 *
 * Both entries take a batch of tensors as host arrays of `count` device pointers and element counts, 1 <= count <= STM_OPTIM_MAX_TENSORS.  The
 * table travels to the kernel by value in its arguments (no table in device memory, nothing uploaded); work is cut into chunks of
 * STM_OPTIM_CHUNK elements, one workgroup each.  A tensor of n[i] == 0 elements may have NULL pointers.
 *
 * Refused before any launch: count < 1, n[i] < 0, a NULL pointer of a tensor with elements, a NULL array, lr / mu / wd not finite, NULL counters
 * (STM_EINVAL); count > STM_OPTIM_MAX_TENSORS, 2^31 chunks or more in one call (STM_EUNSUPPORTED). */
#pragma once
#include <stdint.h>

#include "../../include/stmask_hip.h"
#include "chunk_table.h"

#define STM_OPTIM_MAX_TENSORS STM_CHUNK_MAX_ROWS
#define STM_OPTIM_CHUNK STM_CHUNK_ELEMS

#ifdef __cplusplus
extern "C" {
#endif

/* SGD with momentum and weight decay (dampening 0, no Nesterov term) over `count` fp32 tensors in one launch, per element in IEEE fp32, unfused, in
 * this order:   g' = g + wd * p;   m = mu * m + g';   p = p - lr * m.
 * Guard: every workgroup first reads loss[0] (may be NULL) and bad[0] (int32, may be NULL); if the loss is not finite or bad != 0 the launch
 * leaves p and m untouched.  first_launch != 0 (the first launch of an optimizer step): one thread adds 1 to counters[0] (applied) or counters[1]
 * (skipped), a plain load and store -- the launches of a stream are ordered.  loss, bad and counters are device pointers. */
int stm_sgd_step_multi_f32(float* const* p, const float* const* g, float* const* m, const int64_t* n, int count, const float* loss, const int* bad,
                           int* counters, int first_launch, float lr, float mu, float wd, stm_stream_t stream);

/* bad[0] = 1 when any element of the `count` gradient tensors is NaN or +-inf (racing stores of the same value, no atomic); otherwise bad is left as
 * it is.  first_launch != 0: bad[0] is set to 0 on the stream before the launch. */
int stm_grads_nonfinite_multi_f32(const float* const* g, const int64_t* n, int count, int* bad, int first_launch, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
