/* fold.h -- the parameter write of the inference twin (stmask_amd/validate.py: InferenceTwin.refresh), gfx950 (MI355X).
 *
 * Package-private: exported by libstmask_hip.so, restated in stmask_amd/_lib.py FOLD_SIGNATURES and bound on first use by _lib.private_call().
 * Not part of the drop-in boundary of include/ (no C client of that boundary keeps a folded copy of a net in training), so STM_ABI_VERSION
 * does not count these.
 *
 * One call writes up to STM_FOLD_MAX_ROWS fp32 tensors from the live net's: a plain copy, or eval-mode BatchNorm folded into the convolution in
 * front of it (stmask_amd/fuse.py _fold), per element in IEEE fp32, every operation rounded once, nothing contracted, sqrt and division
 * correctly rounded:
 *     s = gamma[c] / sqrt(var[c] + eps)          c = index / inner, the output channel of the element
 *     STM_FOLD_WEIGHT   dst = src * s
 *     STM_FOLD_BIAS     dst = (src - mean[c]) * s + beta[c]          a NULL src is a convolution without bias: src = 0
 *     STM_FOLD_COPY     dst = src
 * which is what torch computes on the CPU for those expressions, bit for bit; NaN and inf travel through the arithmetic as they do there.
 *
 * The rows reach the kernel by value in its arguments (no table in device memory, nothing uploaded); work is cut into chunks of STM_FOLD_CHUNK
 * elements, one workgroup each.  eps is one kernel argument: consecutive rows of equal eps share a launch (a net's BatchNorm layers share
 * theirs, so a call is one launch).  A chunk whose dst and src are 16-byte aligned moves 16 bytes per access, its last numel % 4 elements and
 * every chunk of a tensor that starts at an odd offset 4 bytes.  No LDS, no scratch, no atomics; the host reads nothing back.
 *
 * Refused before any launch: count < 0, a NULL rows with count > 0, numel < 0, an unknown kind, a NULL dst or (copy, weight) src of a row with
 * elements, a fold row without the BatchNorm pointers it reads, inner < 1 or numel not a multiple of inner in a fold row (STM_EINVAL);
 * count > STM_FOLD_MAX_ROWS, numel >= 2^31 (STM_EUNSUPPORTED).  dst may not overlap any source. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/stmask_hip.h"
#include "chunk_table.h"

#define STM_FOLD_MAX_ROWS STM_CHUNK_MAX_ROWS
#define STM_FOLD_CHUNK STM_CHUNK_ELEMS

#define STM_FOLD_COPY 0
#define STM_FOLD_WEIGHT 1
#define STM_FOLD_BIAS 2

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor to write.  gamma / beta / mean / var: the BatchNorm's weight, bias, running_mean, running_var, numel / inner elements each; NULL
 * where the kind does not read them (copy: all four; weight: beta and mean). */
typedef struct stm_fold_row {
    float* dst;
    const float* src;
    const float* gamma;
    const float* beta;
    const float* mean;
    const float* var;
    int64_t numel;
    int64_t inner;     /* elements per output channel: C * kh * kw of a weight, 1 of a bias; not read for a copy */
    int kind;
    float eps;
} stm_fold_row;

/* which = 0: sizeof(stm_fold_row); anything else 0 */
size_t stm_fold_struct_bytes(int which);

/* rows: a host array of `count` rows holding device pointers.  Rows without elements are passed over; count == 0 launches nothing. */
int stm_fold_rows_f32(const stm_fold_row* rows, int count, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
