/* stmask_hip_data.h -- training batches on the device: the frame pairs of a YouTube-VIS batch resized, normalised, flipped and padded from their
 * uint8 sources, the ground-truth masks rendered straight from COCO run lengths to the resized, flipped, padded uint8 target the mask loss reads
 * (a mask at source resolution is never built), and the box transform.  What the reference does per sample on the host in datasets/ytvos.py
 * prepare_train_img and datasets/transforms.py (ImageTransform, MaskTransform, BboxTransform) for img_scale=[(w, h)], resize_keep_ratio=False.
 * A seventh header beside stmask_hip.h, stmask_hip_output.h, stmask_hip_tracker.h, stmask_hip_train.h, stmask_hip_eval.h and
 * stmask_hip_t2s_feat.h (whose prototype lists and STM_ABI_VERSION are unchanged): new entry points only, same library, same error codes, same
 * stream convention.  INTEGRATION.md section 20 restates the contract; stmask_amd/datasets.py is the caller.
 *
 * Compressed RLE strings go through stm_vis_rle_decode (stmask_hip_eval.h) first; the status bits are that header's STM_VIS_RLE_*.
 * Integer arithmetic and fixed operation orders throughout, no atomics: the same bytes from run to run.  No entry point reads anything back.
 */
#ifndef STMASK_HIP_DATA_H
#define STMASK_HIP_DATA_H

#include "stmask_hip_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

/* struct sizes as the library was compiled: 0 stm_data_frame_desc, 1 stm_data_mask_desc; anything else 0 */
size_t stm_data_struct_bytes(int which);

/* ---- frames: ImageTransform.__call__ (keep_ratio=False) in one pass over the output ------------------------------------------------------
 * frames[i]: uint8 HWC (BGR as cv2 reads it) rows of W0 * 3 contiguous bytes, row_stride_bytes apart (>= 3 * W0); flip != 0 mirrors the image.
 * out [n, 3, Hp, Wp] fp32.  Per output pixel (x, y) with y < h and x < w, in the reference's order:
 *   1. the cv2 8-bit INTER_LINEAR resize to (w, h) at column xs = flip ? w - 1 - x : x (the arithmetic of stm_preprocess_u8_multi_f32);
 *   2. to_rgb != 0: output channel c holds source channel 2 - c;
 *   3. (v - mean[c]) / stdv[c] with mean / stdv in the OUTPUT's channel order, in double, rounded to fp32 once;
 * zeros where y >= h or x >= w.  With flip = 0 and to_rgb = 0 image i is bit-identical to stm_preprocess_u8_multi_f32 (mode 1).
 * The descriptors are read on the host and travel in the kernel arguments, 64 frames per launch. */
typedef struct stm_data_frame_desc {
    const uint8_t* ptr;
    int H0, W0;
    int64_t row_stride_bytes;
    int flip;
    int reserved;
} stm_data_frame_desc;
int stm_data_frames_u8_f32(const stm_data_frame_desc* frames, int n, float* out, int h, int w, int Hp, int Wp, const double* mean,
                           const double* stdv, int to_rgb, stm_stream_t stream);

/* ---- run lengths -> exclusive prefix sums ------------------------------------------------------------------------------------------------
 * runs [total_runs] uint32: the run lengths of n masks; mask i owns the slot runs[offsets[i] .. offsets[i + 1]) (offsets [n + 1] int64).
 * n_runs_in [n] int32 or NULL: how many runs of the slot are in use (what stm_vis_rle_decode reported; clamped to the slot); NULL: all of it.
 * status_in [n] int32 or NULL: status bits a mask already carries (stm_vis_rle_decode's); such a mask stays flagged.
 * hw [n] int64: H0 * W0 of each mask, < 2^32 (the caller checks: a start must fit 32 bits).
 *   starts [total_runs] uint32: starts[offsets[i] + j] = runs[offsets[i]] + .. + runs[offsets[i] + j - 1]
 *   n_runs [n] int32, area [n] int64 (the sum of the odd-indexed runs), status [n] int32: STM_VIS_RLE_SUM when the runs do not sum to hw[i],
 *   STM_VIS_RLE_RANGE when the slot holds 2^31 runs or more.  A flagged mask gets n_runs = 0 and area = 0.
 * n_runs_in / status_in may alias n_runs / status.  One wavefront per mask, 64 runs per pass, the running total carried between passes. */
int stm_data_rle_starts(const unsigned int* runs, const int64_t* offsets, const int* n_runs_in, const int* status_in, const int64_t* hw, int n,
                        int64_t total_runs, unsigned int* starts, int* n_runs, int64_t* area, int* status, stm_stream_t stream);

/* ---- ground-truth masks: MaskTransform.__call__ (keep_ratio=False) from the run starts ---------------------------------------------------
 * desc [n] in DEVICE memory: the source size and the flip flag of output mask i, and `list`: which of the n_lists run lists it is drawn from
 * (the lists may be stored in another order than the masks are wanted, compressed strings first for instance; a list outside [0, n_lists)
 * gives zeros).  starts / offsets [n_lists + 1] / n_runs [n_lists] as stm_data_rle_starts wrote them.
 * out [n, Hp, Wp] uint8, values 0 / 1; every byte is written by this launch (zeros where y >= h or x >= w, and for a mask with n_runs = 0 or a
 * non-positive size): no memset.  Wp must be a multiple of 4 (every lane stores 4 bytes at a time; a wavefront writes 256 contiguous bytes).
 * The rule is cv2.resize(mask, (w, h), interpolation=INTER_NEAREST), then [:, ::-1] if flip, then the pad.  cv2's nearest rule, restated from
 * resizeNN in its imgproc/resize.cpp (cv2 was not available to re-capture it):
 *     inv = (double)w / W0;  ifx = 1.0 / inv;  sx = min((int)floor(xs * ifx), W0 - 1)      with xs = flip ? w - 1 - x : x, likewise sy from y;
 * note 1.0 / ((double)w / W0), not (double)W0 / w.  The source pixel (sy, sx) has the column-major index k = sx * H0 + sy; its value is the
 * parity of the last run whose start is <= k (a zero-length run is never picked over the run behind it). */
typedef struct stm_data_mask_desc {
    int H0, W0;
    int flip;
    int list;
} stm_data_mask_desc;
int stm_data_masks_u8(const unsigned int* starts, const int64_t* offsets, const int* n_runs, int n_lists, const stm_data_mask_desc* desc, int n,
                      int64_t total_runs, unsigned char* out, int h, int w, int Hp, int Wp, stm_stream_t stream);

/* ---- boxes: BboxTransform.__call__ in fp32, every step rounded as numpy's float32 does (no multiply-add is contracted) --------------------
 * boxes [n, 4] fp32 (x1, y1, x2, y2 in source pixels), desc [n] in device memory (box i belongs to mask i; `list` is not read).  out [n, 4] fp32:
 *     b * [ws, hs, ws, hs]  with ws = (float)((double)w / W0), hs = (float)((double)h / H0);
 *     flip: x1' = ((float)w - x2) - 1, x2' = ((float)w - x1) - 1;
 *     x clipped to [0, w], y to [0, h];  x / (float)Wp, y / (float)Hp. */
int stm_data_boxes_f32(const float* boxes, const stm_data_mask_desc* desc, int n, float* out, int h, int w, int Hp, int Wp, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
