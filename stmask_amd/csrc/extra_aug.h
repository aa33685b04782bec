/* extra_aug.h -- ExtraAugmentation (datasets/extra_aug.py: PhotoMetricDistortion, Expand, RandomCrop) inside the training-batch kernels, gfx950
 * (MI355X).  The host draws the parameters (stmask_amd/extra_aug.py); these kernels do the per-pixel work on the way from the uint8 sources and
 * the run lists to the batch, so that nothing at source resolution is written.  INTEGRATION.md section 22 is the contract.
 *
 * Package-private: exported by libstmask_hip.so, restated in stmask_amd/_lib.py AUG_SIGNATURES and bound on first use by _lib.private_call().
 * Not part of the drop-in boundary of include/, so STM_ABI_VERSION does not count these.
 *
 * One function of the augmented image's coordinates (sy, sx) -- the image keeps its size H0 x W0 through all three transforms -- gives its bytes:
 *   1. RandomCrop: outside the patch [y0, y1) x [x0, x1) the bytes are 0 (the reference zeroes, it does not move the image);
 *   2. Expand: (sy, sx) is a pixel of the canvas (Hc, Wc) = (int(H0 * ratio), int(W0 * ratio)) resized back by cv2's nearest rule,
 *          cy = min((int)floor(sy * (1.0 / ((double)H0 / Hc))), Hc - 1) - top, likewise cx with left;
 *      off the source the value is fill[c] (mean[::-1] in the image's BGR order, not distorted); on it, the source pixel through
 *   3. PhotoMetricDistortion, in IEEE fp32, one rounding per operation, nothing contracted, when photo != 0:
 *          x = (float)byte;  x += delta;  x *= alpha_pre;  BGR -> HSV;  S *= saturation;  H += hue;  if (H > 360) H -= 360;  if (H < 0) H += 360;
 *          HSV -> BGR;  x *= alpha_post;  out[c] = x[perm[c]]
 *      with cv2.cvtColor's float32 rule, restated from OpenCV's scalar path (cv2 was not available to re-capture it):
 *          v = max(b, g, r);  d = v - min(b, g, r);  s = d / (fabsf(v) + FLT_EPSILON);  k = (float)(60.0 / (double)(d + FLT_EPSILON));
 *          h = v == r ? (g - b) * k : v == g ? (b - r) * k + 120 : (r - g) * k + 240;  if (h < 0) h += 360;
 *      and back: s == 0 gives b = g = r = v; otherwise h *= 6.f / 360.f, wrapped into [0, 6) by repeated +-6, sector = floor(h), h -= sector
 *      (a sector outside 0..5: sector = 0, h = 0), tab = {v, v * (1 - s), v * (1 - s * h), v * (1 - s * (1 - h))} and
 *      (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector];
 *   4. the cast of `imgs[i] = img` into a uint8 array: cast_clip == 0 truncates toward zero and keeps the low 8 bits (300.7 -> 44, -5.5 -> 251);
 *      cast_clip != 0 clips to [0, 255] first.
 * Identity: photo = 0, (Hc, Wc, top, left) = (H0, W0, 0, 0), patch (0, 0, W0, H0): the source's own bytes.
 *
 * The descriptors are read by the kernels from DEVICE memory (one block uploaded per batch); the entries that dereference ptr also take the same
 * descriptors in host memory and refuse, before any launch, a NULL pointer, a non-positive size, a row stride below 3 * W0, a canvas smaller than
 * the source plus its offset, and a patch outside the image.  The device copy must hold those values when the launch runs (an upload queued
 * earlier on the same stream). */
#pragma once
#include <stdint.h>

#include "../../include/stmask_hip_data.h"

#define STM_AUG_FRAMES_PER_LAUNCH 64

#ifdef __cplusplus
extern "C" {
#endif

typedef struct stm_aug_desc {
    const uint8_t* ptr;          /* uint8 HWC source, BGR; not read by stm_aug_masks_u8 */
    int64_t row_stride_bytes;
    int H0, W0;
    int flip;                    /* stm_aug_frames_u8_f32 only (the masks take stm_data_mask_desc's) */
    int photo;
    float delta, alpha_pre, saturation, hue, alpha_post;
    int perm[3];
    int Hc, Wc, top, left;
    float fill[3];
    int x0, y0, x1, y1;
    int cast_clip;
} stm_aug_desc;

/* sizeof(stm_aug_desc) as the library was compiled (which == 0); anything else 0 */
size_t stm_aug_struct_bytes(int which);

/* stm_data_frames_u8_f32 with every tap of the 8-bit bilinear resize read through the function above instead of memory; to_rgb, the
 * normalisation, the flip and the pad as there, and with identity descriptors its bits.  out [n, 3, Hp, Wp] fp32.
 * STM_AUG_FRAMES_PER_LAUNCH frames per launch. */
int stm_aug_frames_u8_f32(const stm_aug_desc* desc_host, const stm_aug_desc* desc_dev, int n, float* out, int h, int w, int Hp, int Wp,
                          const double* mean, const double* stdv, int to_rgb, stm_stream_t stream);

/* stm_data_masks_u8 with the same coordinate maps between the target pixel and the run-list lookup: zero outside the patch and zero off the
 * source inside the canvas.  frame_of [n] int32 (device): the descriptor of desc_dev [n_frames] that mask i is augmented by; an index outside
 * [0, n_frames) gives zeros.  Of a descriptor only Hc, Wc, top, left and the patch are read; the sizes and the flip are mask_desc's.  No pointer
 * of a descriptor is followed and every run-list read is clamped to the list's slot, so no descriptor value can make it read out of bounds. */
int stm_aug_masks_u8(const unsigned int* starts, const int64_t* offsets, const int* n_runs, int n_lists, const stm_data_mask_desc* mask_desc,
                     const int* frame_of, const stm_aug_desc* desc_dev, int n_frames, int n, int64_t total_runs, unsigned char* out, int h, int w,
                     int Hp, int Wp, stm_stream_t stream);

/* The augmented image itself, uint8 HWC [H0, W0, 3] contiguous: one thread per pixel writes the function's bytes.  For looking at what an
 * augmentation did, and for holding the colour function byte by byte. */
int stm_aug_source_u8(const stm_aug_desc* desc_host, const stm_aug_desc* desc_dev, unsigned char* out, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
