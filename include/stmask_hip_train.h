/* stmask_hip_train.h -- the batched mask term of the training criterion (the reference's lincomb_mask_loss, layers/modules/multibox_loss.py
 * :544-616, :636) on the device: the ordered list of the positive priors of a batch, the gather that forms every per-row input of the mask
 * kernels (the crop box of :559-563 among them), the weighted reduction with its adjoint, the prototype gradient of the row-prototype form of
 * stm_lincomb_sigmoid_crop_f32 and the return of the coefficient rows to grad mask_data.
 * A fourth header beside stmask_hip.h, stmask_hip_output.h and stmask_hip_tracker.h (whose prototype lists and STM_ABI_VERSION are unchanged):
 * new entry points only, same library, same error codes, same stream convention.  INTEGRATION.md section 14 describes the composition.
 *
 * Nothing in conf_t or idx_t can fault: a prior is positive iff conf_t > 0, and an idx_t outside its image's masks is CLAMPED into
 * [0, G_b - 1] on the device (then into [0, G_total - 1], for an image without masks).
 * Refused from the shapes before any launch: B or P below 1, B * P > 2^22, more than 65535 rows, M outside {8, 32, 64}.
 * No float atomics, no integer atomics; every grid depends on the shapes only; outputs are written, not accumulated.
 */
#ifndef STMASK_HIP_TRAIN_H
#define STMASK_HIP_TRAIN_H

#include "stmask_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the list state of stm_mbox_positives for B images of P priors (64 for shapes the entry points refuse). */
size_t stm_mbox_workspace_bytes(int B, int P);

/* The ordered list of the positives (conf_t > 0) of the batch, flattened index order: count, scan, index (three launches, no host read).
 *   conf_t [B * P] int64; prefix [B + 1] int32: the exclusive prefix of the per-image counts, prefix[B] = n
 *   max_rows > 0: the status word of the state becomes 1 when n > max_rows; 0: no cap
 *   workspace: the list state, kept by the caller until the last gather / scatter that reads it has run */
int stm_mbox_positives(const int64_t* conf_t, int* prefix, int B, int P, int max_rows, void* workspace, size_t workspace_bytes,
                       stm_stream_t stream);

/* n_rows rows through the list in one launch.  Row r < n (the live count) is prior src = list[r] of image b = src / P:
 *   coeff_rows [n_rows * M]  mask_data[src]
 *   box_rows [n_rows * 4]    clamp(point_form(center_size(decode(loc[src], priors[src])) with width and height * 1.2f), 1e-5, 1): IEEE fp32 in the
 *                            reference's operand order (stm_decode_one; center_size (x2 + x1) / 2, x2 - x1; point_form cx - w / 2, cx + w / 2)
 *   row_img [n_rows]         b
 *   idx_rows [n_rows]        mask_offs[b] + clamp(idx_t[src], 0, G_b - 1), clamped into [0, G_total - 1]
 *   scale_rows [n_rows]      w_r / max(bw W, 1) / max(bh H, 1) in fp32, w_r = 1 / max(n_b, 1), bw = box.x2 - box.x1, bh = box.y2 - box.y1
 * Rows past the live count are padding: zero coefficients, box (0, 0, 1, 1), image 0, mask row 0, scale 0.
 *   n_dev [1] = min(n, n_rows); status [1] = the state's status word
 * priors [P * 4] (priors_per_image = 0) or [B * P * 4] (1); mask_offs [B + 1] int32: first row of every image in the concatenated masks. */
int stm_mbox_gather_f32(const float* loc, const float* priors, int priors_per_image, const float* mask_data, const int64_t* idx_t,
                        const int* mask_offs, int G_total, float* coeff_rows, float* box_rows, int* row_img, int64_t* idx_rows, float* scale_rows,
                        int* n_dev, int* status, int n_rows, int B, int P, int M, int H, int W, const void* workspace, size_t workspace_bytes,
                        stm_stream_t stream);

/* loss [1] = (float)(mask_alpha * sum over r < n_dev of (double)scale_rows[r] * (double)bce[r]): one workgroup, thread t takes rows t, t + 256,
 * ..., so the padded and the exact form add the same numbers in the same order.  NaN when status != 0. */
int stm_mbox_reduce_f32(const float* bce, const float* scale_rows, const int* n_dev, const int* status, float* loss, int n_rows,
                        double mask_alpha, stm_stream_t stream);

/* grad_bce [n_rows] = (float)(grad_loss * mask_alpha * scale_rows[r]) for r < n_dev, exact zeros past it; NaN everywhere when status != 0. */
int stm_mbox_reduce_backward_f32(const float* grad_loss, const float* scale_rows, const int* n_dev, const int* status, float* grad_bce,
                                 int n_rows, double mask_alpha, stm_stream_t stream);

/* grad_proto [n_proto * h * w * m] of the row-prototype form of stm_lincomb_sigmoid_crop_f32 (apply_tanh = 1), the rows sorted by prototype
 * set: rows prefix[b] .. prefix[b + 1] (clamped into [0, n]) use set b.  One thread is one prototype pixel with m register accumulators; grid
 * (pixel blocks of 256, sets, row splits), the number of splits a function of h, w and n_proto only; a workgroup walks its rows in row order in
 * chunks of 16, z = grad_out * e / (1 + e)^2 inside the row's crop rectangle (grad_out is not read outside); with more than one split a second
 * launch adds the partials in split order.  A set without rows gets exact zeros.  status [1] or NULL: NaN everywhere when *status != 0.
 * The workspace size is 64 for the shapes the launch entry refuses. */
size_t stm_lincomb_rows_proto_backward_workspace_bytes(int n_proto, int h, int w, int m);
int stm_lincomb_rows_proto_backward_f32(const float* grad_out, const float* proto, int n_proto, const float* coeff, const float* boxes,
                                        const int* prefix, const int* status, float* grad_proto, int h, int w, int m, int n, void* workspace,
                                        size_t workspace_bytes, stm_stream_t stream);

/* grad_mask_data [B * P * M]: row list[r] = grad_rows[r] for r < n_dev; every row that is not positive is written as exact zeros (mask_data is
 * not read); a positive row past n_dev, or any positive row when *status != 0, is NaN.  One launch over the tiles of the list, no atomics: the
 * list's rows are unique.  workspace: the state stm_mbox_positives filled for this conf_t. */
int stm_mbox_scatter_coeff_f32(const float* grad_rows, const int64_t* conf_t, const int* n_dev, const int* status, float* grad_mask_data,
                               int n_rows, int B, int P, int M, const void* workspace, size_t workspace_bytes, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
