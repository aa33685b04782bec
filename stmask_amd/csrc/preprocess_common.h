// preprocess_common.h -- the cv2 INTER_LINEAR-on-uint8 resize and the normalisation behind it, one output pixel at a time.  Shared by the
// inference pre-processing (output.hip: stm_preprocess_u8_f32, stm_preprocess_u8_multi_f32) and the training frames (train_data.hip:
// stm_data_frames_u8_f32), so the three perform the identical integer / float / double operation sequence.  The 8-bit bilinear arithmetic is
// OpenCV's fixed-point path, restated in oracle/stm_oracle.c (orc_resize_pixel_u8) with the derivation.
#pragma once
#include "stm_common.h"

__device__ __forceinline__ void resize_coeffs(int src, int dst, int d, bool clamp_f, int& s, int& c0, int& c1)
{
    const double inv = (double)dst / (double)src;
    const double scale = 1.0 / inv;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (clamp_f) {
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= src - 1) { f = 0.0f; s = src - 1; }
    }
    int a0 = (int)rintf((1.0f - f) * 2048.0f), a1 = (int)rintf(f * 2048.0f);   // cvRound: round half to even
    c0 = min(max(a0, -32768), 32767);
    c1 = min(max(a1, -32768), 32767);
}

// cv2 resizeNN: the source index of destination index d on an axis resized from `src` to `dst` (include/stmask_hip_data.h states the rule)
__device__ __forceinline__ int resize_nearest(int d, int src, int dst)
{
    const double inv = (double)dst / (double)src;
    const double ifx = 1.0 / inv;
    return min((int)floor((double)d * ifx), src - 1);
}

// One output pixel (x, y) < (w, h) of an image whose source rows start at `img` with `row_stride` bytes between rows (3 bytes per pixel):
// the fixed-point bilinear taps, then the mode's normalisation in double.  mean / stdv are indexed by the SOURCE channel c, as o is.
__device__ __forceinline__ void preprocess_pixel(const uint8_t* __restrict__ img, int64_t row_stride, int H0, int W0, int h, int w, int x, int y,
                                                 const double (&mean)[3], const double (&stdv)[3], int mode, float (&o)[3])
{
    int sx, sy, a0, a1, b0, b1;
    resize_coeffs(W0, w, x, true, sx, a0, a1);
    resize_coeffs(H0, h, y, false, sy, b0, b1);
    const int sx1 = min(sx + 1, W0 - 1);
    const int y0 = min(max(sy, 0), H0 - 1), y1 = min(max(sy + 1, 0), H0 - 1);
    const uint8_t* r0 = img + (int64_t)y0 * row_stride;
    const uint8_t* r1 = img + (int64_t)y1 * row_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int D0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
        const int D1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
        int v = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
        double d = (double)v;
        if (mode == 1) d = (d - mean[c]) / stdv[c];
        else if (mode == 2) d = d - mean[c];
        else if (mode == 3) d = d / 255.0;
        o[c] = (float)d;
    }
}
