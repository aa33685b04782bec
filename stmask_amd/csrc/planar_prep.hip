// planar_prep.hip -- the producers of the planar activation / weight layouts that are not convolutions: entry into the planes from
// fp32 NHWC (split, bilinear resize, stem tail, stem row patches), CandidateShift's RoI features written straight into planes, and the
// weight packer of the planar convolution kernels (conv_bf16x.hip).  Layouts: include/stmask_hip.h; store_planes8: planar_common.h.
#include "planar_common.h"

namespace {

// fp32 [n pixels][C] (NHWC) -> three bf16 planes [3][C/32][n][32] (entry into the planar format from a foreign producer);
// thread = 8 channels of one pixel
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, uint8_t* __restrict__ planes, int64_t n, int C,
                                                           int fmt, int* range_flag)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c8n = C >> 3;
    if (idx >= n * c8n) return;
    const int64_t pix = idx / c8n;
    const int c8 = (int)(idx - pix * c8n);
    const float* src = x + pix * C + c8 * 8;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(src), a1 = *reinterpret_cast<const f32x4*>(src + 4);
    const size_t plane_b = (size_t)n * C * 2;
    uint8_t* dst = planes + (((size_t)(c8 >> 2) * n + pix) * 32 + (c8 & 3) * 8) * 2;
    const float v8[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    store_planes8(dst, plane_b, v8, fmt, range_flag, false);
}

// Bilinear resize (F.interpolate(mode="bilinear", align_corners=False): make_net.py's InterpolateModule between the proto-net
// convolutions) of an fp32 NHWC tensor straight into planes: thread = 8 channels of one output pixel; the fp32 upsampled
// tensor (4x the input for the proto-net's x2) is never written or re-read.  Same expression order as the ATen kernel.
__global__ __launch_bounds__(256) void resize_bilinear_planes_kernel(const float* __restrict__ x, uint8_t* __restrict__ planes, int B, int H,
                                                                    int W, int C, int Ho, int Wo, float sy, float sx, int fmt,
                                                                    int* range_flag)
{
    const int c8n = C >> 3;
    const int64_t n = (int64_t)B * Ho * Wo;
    const int64_t blk = stm_xcd_block((n * c8n + 255) >> 8);
    if (blk < 0) return;
    const int64_t idx = blk * 256 + threadIdx.x;
    if (idx >= n * c8n) return;
    const int64_t pix = idx / c8n;
    const int c8 = (int)(idx - pix * c8n);
    const int b = (int)(pix / ((int64_t)Ho * Wo));
    const int rem = (int)(pix - (int64_t)b * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    // area_pixel_compute_source_index(scale, dst, align_corners=false, cubic=false): max(0, scale * (dst + 0.5) - 0.5)
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.0f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    const float* base = x + (size_t)b * H * W * C + c8 * 8;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x0) * C + 4 * h);
        const f32x4 bq = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x1) * C + 4 * h);
        const f32x4 c = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x0) * C + 4 * h);
        const f32x4 d = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x1) * C + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * h + e] = ly0 * (lx0 * a[e] + lx1 * bq[e]) + ly1 * (lx0 * c[e] + lx1 * d[e]);
    }
    const size_t plane_b = (size_t)n * C * 2;
    uint8_t* dst = planes + (((size_t)(c8 >> 2) * n + pix) * 32 + (c8 & 3) * 8) * 2;
    store_planes8(dst, plane_b, v, fmt, range_flag, true);
}

// ResNet stem tail (backbone.py:73: relu(bn1(conv1)) -> MaxPool2d(3, 2, 1)) on the raw fp32 NHWC convolution output, written as
// planes for layer1: y = relu(max over the 3x3 window (stride 2, pad 1) + folded-BN bias).  The bias add and the ReLU are
// monotone and the bias is per channel, so they commute with the max exactly.  thread = 8 channels of one output pixel.
__global__ __launch_bounds__(256) void bias_relu_maxpool_planes_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                                      uint8_t* __restrict__ planes, int B, int H, int W, int C, int Ho, int Wo,
                                                                      int fmt, int* range_flag)
{
    const int c8n = C >> 3;
    const int64_t n = (int64_t)B * Ho * Wo;
    const int64_t blk = stm_xcd_block((n * c8n + 255) >> 8);
    if (blk < 0) return;
    const int64_t idx = blk * 256 + threadIdx.x;
    if (idx >= n * c8n) return;
    const int64_t pix = idx / c8n;
    const int c8 = (int)(idx - pix * c8n);
    const int b = (int)(pix / ((int64_t)Ho * Wo));
    const int rem = (int)(pix - (int64_t)b * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const float* base = x + (size_t)b * H * W * C + c8 * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = -__builtin_inff();
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
        if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox - 1 + dx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const f32x4 a = *reinterpret_cast<const f32x4*>(base + ((size_t)iy * W + ix) * C);
            const f32x4 c = *reinterpret_cast<const f32x4*>(base + ((size_t)iy * W + ix) * C + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = fmaxf(v[e], a[e]); v[4 + e] = fmaxf(v[4 + e], c[e]); }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t = v[e] + (bias ? bias[c8 * 8 + e] : 0.0f);
        v[e] = t > 0.0f ? t : 0.0f;
    }
    const size_t plane_b = (size_t)n * C * 2;
    uint8_t* dst = planes + (((size_t)(c8 >> 2) * n + pix) * 32 + (c8 & 3) * 8) * 2;
    store_planes8(dst, plane_b, v, fmt, range_flag, true);
}

// CandidateShift's RoI features (TF_utils.py:30-39: relu(cat(corr, T2S_prev, T2S)) -> mmcv roi_align 7x7, aligned, adaptive
// sampling grid) written straight into the planes TemporalNet's first convolution reads: no concatenated feature map, no
// fp32 RoI tensor, no pad / permute / split passes.  Channel order of the planes: [T2S_prev (C1) | T2S (C1) | corr (Cc) |
// zeros] -- the two feature maps are NHWC, so a lane's 8 channels are two 16-byte loads per corner and the lanes of a
// wave read one contiguous run; the correlation volume is NCHW (strided, 19 % of the channels).  The arithmetic is
// roi_align_avg_kernel's, operation for operation (temporal.hip), with the ReLU applied to the sampled inputs.
struct RoiPlanesArgs {
    const float* t2s_prev;   // [B][H][W][C1]
    const float* t2s;        // [B][H][W][C1]
    const float* corr;       // [B][Cc][H][W], or channels-last [B][H][W][corr_ld] when corr_ld > 0
    int corr_ld;
    const float* rois;       // [n][5] = (image, x1, y1, x2, y2) in feature-map pixels
    uint8_t* planes;         // [P][Cpad/32][n*PH*PW][32]
    int n, H, W, C1, Cc, Cpad, PH, PW, fmt;
    int* range_flag;
};

__global__ __launch_bounds__(256) void roi_align_planes_kernel(const RoiPlanesArgs a)
{
    const int gpp = a.Cpad >> 3;                                   // 8-channel groups per output pixel
    const int64_t npix = (int64_t)a.n * a.PH * a.PW;
    const int64_t blk = stm_xcd_block((npix * gpp + 255) >> 8);
    if (blk < 0) return;
    const int64_t idx = blk * 256 + threadIdx.x;
    if (idx >= npix * gpp) return;
    const int64_t pix = idx / gpp;
    const int g = (int)(idx - pix * gpp);
    const int ri = (int)(pix / (a.PH * a.PW));
    const int pp = (int)(pix - (int64_t)ri * a.PH * a.PW);
    const int py = pp / a.PW, px = pp - py * a.PW;
    const float* roi = a.rois + 5 * ri;
    const int b = (int)roi[0];
    const float sw_ = roi[1] - 0.5f, sh_ = roi[2] - 0.5f, ew_ = roi[3] - 0.5f, eh_ = roi[4] - 0.5f;   // aligned, scale 1
    const float rw = ew_ - sw_, rh = eh_ - sh_;
    const float bh = rh / (float)a.PH, bw = rw / (float)a.PW;
    const int gh = (int)ceilf(rh / (float)a.PH), gw = (int)ceilf(rw / (float)a.PW);
    const float count = (float)max(gh * gw, 1);
    const int c0 = g * 8;
    // source of this lane's 8 channels
    const bool from_prev = c0 < a.C1, from_cur = !from_prev && c0 < 2 * a.C1;
    const float* nhwc = from_prev ? a.t2s_prev + (size_t)b * a.H * a.W * a.C1 + c0
                                  : a.t2s + (size_t)b * a.H * a.W * a.C1 + (c0 - a.C1);
    const int cc0 = c0 - 2 * a.C1;                                 // first correlation channel of the lane (NCHW source)
    const float* nchw = a.corr + ((size_t)b * a.Cc + (cc0 > 0 ? cc0 : 0)) * a.H * a.W;
    const float* cl = a.corr + (size_t)b * a.H * a.W * a.corr_ld + (cc0 > 0 ? cc0 : 0);        // channels-last source of the lane's 8 channels
    const int HW = a.H * a.W;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int iy = 0; iy < gh; ++iy) {
        const float ys = sh_ + (float)py * bh + ((float)iy + 0.5f) * bh / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
            const float xs = sw_ + (float)px * bw + ((float)ix + 0.5f) * bw / (float)gw;
            float y = ys, x = xs;
            if (y < -1.0f || y > (float)a.H || x < -1.0f || x > (float)a.W) continue;     // the sample contributes 0
            if (y <= 0.0f) y = 0.0f;
            if (x <= 0.0f) x = 0.0f;
            int y_low = (int)y, x_low = (int)x, y_high, x_high;
            if (y_low >= a.H - 1) { y_high = y_low = a.H - 1; y = (float)y_low; } else y_high = y_low + 1;
            if (x_low >= a.W - 1) { x_high = x_low = a.W - 1; x = (float)x_low; } else x_high = x_low + 1;
            const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
            const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
            const int o1 = y_low * a.W + x_low, o2 = y_low * a.W + x_high, o3 = y_high * a.W + x_low, o4 = y_high * a.W + x_high;
            float v1[8], v2[8], v3[8], v4[8];
            if (from_prev || from_cur) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x4 q1 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o1 * a.C1 + 4 * h);
                    const f32x4 q2 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o2 * a.C1 + 4 * h);
                    const f32x4 q3 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o3 * a.C1 + 4 * h);
                    const f32x4 q4 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o4 * a.C1 + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v1[4 * h + e] = q1[e]; v2[4 * h + e] = q2[e]; v3[4 * h + e] = q3[e]; v4[4 * h + e] = q4[e]; }
                }
            } else if (a.corr_ld > 0) {
                // (channels past Cc of the padded row are whatever the buffer holds: masked, never used)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    // a 4-channel group that lies wholly in the zero padding past Cc is not loaded at all: its address may be
                    // beyond the padded row (Cpad rounds 2*C1 + Cc up to 32, corr_ld only Cc up to 8) or, on the last pixel, the buffer
                    const int hofs = cc0 + 4 * h < a.Cc ? 4 * h : -cc0;          // all-padding group: re-read channel 0 (masked below)
                    const f32x4 q1 = *reinterpret_cast<const f32x4*>(cl + (size_t)o1 * a.corr_ld + hofs);
                    const f32x4 q2 = *reinterpret_cast<const f32x4*>(cl + (size_t)o2 * a.corr_ld + hofs);
                    const f32x4 q3 = *reinterpret_cast<const f32x4*>(cl + (size_t)o3 * a.corr_ld + hofs);
                    const f32x4 q4 = *reinterpret_cast<const f32x4*>(cl + (size_t)o4 * a.corr_ld + hofs);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool real = cc0 + 4 * h + e < a.Cc;
                        v1[4 * h + e] = real ? q1[e] : 0.0f; v2[4 * h + e] = real ? q2[e] : 0.0f;
                        v3[4 * h + e] = real ? q3[e] : 0.0f; v4[4 * h + e] = real ? q4[e] : 0.0f;
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool real = cc0 + e < a.Cc;
                    const float* im = nchw + (size_t)(real ? e : 0) * HW;
                    v1[e] = real ? im[o1] : 0.0f; v2[e] = real ? im[o2] : 0.0f; v3[e] = real ? im[o3] : 0.0f; v4[e] = real ? im[o4] : 0.0f;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                acc[e] += w1 * fmaxf(v1[e], 0.0f) + w2 * fmaxf(v2[e], 0.0f) + w3 * fmaxf(v3[e], 0.0f) + w4 * fmaxf(v4[e], 0.0f);
        }
    }
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = acc[e] / count;
    const size_t plane_b = (size_t)npix * a.Cpad * 2;
    uint8_t* dst = a.planes + (((size_t)(g >> 2) * npix + pix) * 32 + (g & 3) * 8) * 2;
    store_planes8(dst, plane_b, v, a.fmt, a.range_flag, false);
}

// The same, laid out for the memory system (round 5; channels-last correlation volume only).  The kernel above gives a wave 64 channel groups of ONE
// pixel: its plane stores are sixteen 64-byte pieces in sixteen channel slabs per instruction, and nothing of what neighbouring bins share (the corners of
// adjacent bins of a RoI are the same feature pixels) is reused inside a workgroup.  Here a workgroup owns 16 consecutive output pixels (two to three rows
// of a 7 x 7 RoI grid) and every channel slab: lane = 4 pixel + chunk, wave w takes slabs w, w + 4, ... -- a plane store is 1 KB contiguous (16 pixels x
// 64 B), a corner read 16 full 128-byte lines, and the five slabs of a lane share its RoI arithmetic.  Same expressions per output value: bit-equal.
__global__ __launch_bounds__(256) void roi_align_planes_tiled_kernel(const RoiPlanesArgs a)
{
    const int64_t npix = (int64_t)a.n * a.PH * a.PW;
    const int64_t blk = stm_xcd_block((npix + 15) >> 4);
    if (blk < 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pix_ = blk * 16 + (lane >> 2);
    const bool live = pix_ < npix;
    const int64_t pix = live ? pix_ : npix - 1;
    const int ck = lane & 3;
    const int ri = (int)(pix / (a.PH * a.PW));
    const int pp = (int)(pix - (int64_t)ri * a.PH * a.PW);
    const int py = pp / a.PW, px = pp - py * a.PW;
    const float* roi = a.rois + 5 * ri;
    const int b = (int)roi[0];
    const float sw_ = roi[1] - 0.5f, sh_ = roi[2] - 0.5f, ew_ = roi[3] - 0.5f, eh_ = roi[4] - 0.5f;   // aligned, scale 1
    const float rw = ew_ - sw_, rh = eh_ - sh_;
    const float bh = rh / (float)a.PH, bw = rw / (float)a.PW;
    const int gh = (int)ceilf(rh / (float)a.PH), gw = (int)ceilf(rw / (float)a.PW);
    const float count = (float)max(gh * gw, 1);
    const size_t plane_b = (size_t)npix * a.Cpad * 2;
    const int nslabs = a.Cpad >> 5;
    for (int s = wave; s < nslabs; s += 4) {
        const int g = s * 4 + ck;
        const int c0 = g * 8;
        const bool from_prev = c0 < a.C1, from_cur = !from_prev && c0 < 2 * a.C1;
        const float* nhwc = from_prev ? a.t2s_prev + (size_t)b * a.H * a.W * a.C1 + c0
                                      : a.t2s + (size_t)b * a.H * a.W * a.C1 + (c0 - a.C1);
        const int cc0 = c0 - 2 * a.C1;                             // first correlation channel of the lane
        const float* cl = a.corr + (size_t)b * a.H * a.W * a.corr_ld + (cc0 > 0 ? cc0 : 0);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int iy = 0; iy < gh; ++iy) {
            const float ys = sh_ + (float)py * bh + ((float)iy + 0.5f) * bh / (float)gh;
            for (int ix = 0; ix < gw; ++ix) {
                const float xs = sw_ + (float)px * bw + ((float)ix + 0.5f) * bw / (float)gw;
                float y = ys, x = xs;
                if (y < -1.0f || y > (float)a.H || x < -1.0f || x > (float)a.W) continue;     // the sample contributes 0
                if (y <= 0.0f) y = 0.0f;
                if (x <= 0.0f) x = 0.0f;
                int y_low = (int)y, x_low = (int)x, y_high, x_high;
                if (y_low >= a.H - 1) { y_high = y_low = a.H - 1; y = (float)y_low; } else y_high = y_low + 1;
                if (x_low >= a.W - 1) { x_high = x_low = a.W - 1; x = (float)x_low; } else x_high = x_low + 1;
                const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                const int o1 = y_low * a.W + x_low, o2 = y_low * a.W + x_high, o3 = y_high * a.W + x_low, o4 = y_high * a.W + x_high;
                float v1[8], v2[8], v3[8], v4[8];
                if (from_prev || from_cur) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 q1 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o1 * a.C1 + 4 * h);
                        const f32x4 q2 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o2 * a.C1 + 4 * h);
                        const f32x4 q3 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o3 * a.C1 + 4 * h);
                        const f32x4 q4 = *reinterpret_cast<const f32x4*>(nhwc + (size_t)o4 * a.C1 + 4 * h);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v1[4 * h + e] = q1[e]; v2[4 * h + e] = q2[e]; v3[4 * h + e] = q3[e]; v4[4 * h + e] = q4[e]; }
                    }
                } else {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int hofs = cc0 + 4 * h < a.Cc ? 4 * h : -cc0;          // all-padding group: re-read channel 0 (masked below)
                        const f32x4 q1 = *reinterpret_cast<const f32x4*>(cl + (size_t)o1 * a.corr_ld + hofs);
                        const f32x4 q2 = *reinterpret_cast<const f32x4*>(cl + (size_t)o2 * a.corr_ld + hofs);
                        const f32x4 q3 = *reinterpret_cast<const f32x4*>(cl + (size_t)o3 * a.corr_ld + hofs);
                        const f32x4 q4 = *reinterpret_cast<const f32x4*>(cl + (size_t)o4 * a.corr_ld + hofs);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool real = cc0 + 4 * h + e < a.Cc;
                            v1[4 * h + e] = real ? q1[e] : 0.0f; v2[4 * h + e] = real ? q2[e] : 0.0f;
                            v3[4 * h + e] = real ? q3[e] : 0.0f; v4[4 * h + e] = real ? q4[e] : 0.0f;
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    acc[e] += w1 * fmaxf(v1[e], 0.0f) + w2 * fmaxf(v2[e], 0.0f) + w3 * fmaxf(v3[e], 0.0f) + w4 * fmaxf(v4[e], 0.0f);
            }
        }
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = acc[e] / count;
        if (live) {
            uint8_t* dst = a.planes + (((size_t)s * npix + pix) * 32 + ck * 8) * 2;
            store_planes8(dst, plane_b, v, a.fmt, a.range_flag, false);
        }
    }
}

// Stem entry (backbone.py:73, the 7x7 / stride-2 convolution on the 3-channel frame): the kw * Cin = 21 values one kernel row
// reads for output column ox are contiguous in the NHWC frame, starting at column sw*ox - pw.  This kernel lays them out as
// the 32-channel slab of a planar tensor R[b][y][ox][32] (channels >= kw*Cin zero, columns outside the frame zero), which
// turns the stem into a (kh x 1) convolution with stride (sh, 1) over R on the planar kernel: K = kh * 32 = 224 for 147
// real products, no im2col buffer, no library call.  thread = 8 channels of one R pixel.
__global__ __launch_bounds__(256) void stem_rows_planes_kernel(const float* __restrict__ x, uint8_t* __restrict__ planes, int B, int H, int W,
                                                              int Cin, int kw, int sw, int pw, int Wo, int fmt, int* range_flag)
{
    const int64_t n = (int64_t)B * H * Wo;
    const int64_t blk = stm_xcd_block((n * 4 + 255) >> 8);
    if (blk < 0) return;
    const int64_t idx = blk * 256 + threadIdx.x;
    if (idx >= n * 4) return;
    const int64_t pix = idx >> 2;
    const int g = (int)(idx & 3);
    const int ox = (int)(pix % Wo);
    const int64_t row = pix / Wo;                                   // b * H + y
    const float* src = x + row * (int64_t)W * Cin;
    const int c0 = (sw * ox - pw) * Cin;                            // first float of the patch within the frame row
    const int lim = W * Cin, real = kw * Cin;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = g * 8 + e, c = c0 + j;
        v[e] = (j < real && c >= 0 && c < lim) ? src[c] : 0.0f;
    }
    const size_t plane_b = (size_t)n * 32 * 2;
    uint8_t* dst = planes + ((size_t)pix * 32 + g * 8) * 2;
    store_planes8(dst, plane_b, v, fmt, range_flag, false);
}

// Weights [Cout][Cin][kh][kw] fp32 -> packed [n_tile][slab][plane][row 0..127][swizzled 16-B chunk][8 bf16]; rows past
// Cout are zero.  One thread per (n_tile, slab, row, chunk).
__global__ __launch_bounds__(256) void conv_pack_weights_kernel(const float* __restrict__ w, uint8_t* __restrict__ wp, int Cout,
                                                                int C, int kh, int kw, int slabs, int n_tiles, int npl, int bn, int fmt,
                                                                float wscale)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int per_tile = bn * 4;                       // (row, chunk) pairs of one slab tile
    const int64_t total = (int64_t)n_tiles * slabs * per_tile;
    if (idx >= total) return;
    const int chunk = (int)(idx & 3), row = (int)((idx >> 2) % bn);
    const int slab = (int)((idx / per_tile) % slabs), nt = (int)((idx / per_tile) / slabs);
    const int taps = kh * kw;
    const int cs = slab / taps, tap = slab - cs * taps, c0 = cs * CV_BK + chunk * 8;   // K order: channel slab outer, tap inner
    const int co = nt * bn + row;
    unsigned pl[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f32x2 v = {0.0f, 0.0f};
        if (co < Cout) {
            v.x = w[((size_t)co * C + c0 + 2 * e) * (kh * kw) + tap];
            v.y = w[((size_t)co * C + c0 + 2 * e + 1) * (kh * kw) + tap];
        }
        if (fmt >= 1) { pl[2][e] = 0; split2_f16(v * wscale, pl[0][e], pl[1][e]); }
        else split2(v, pl[0][e], pl[1][e], pl[2][e]);
    }
    const int wpl = bn * 64;
    uint8_t* dst = wp + ((size_t)nt * slabs + slab) * (npl * wpl) + lds_off(row, chunk);
    for (int p = 0; p < npl; ++p) {
        u32x4 o = {pl[p][0], pl[p][1], pl[p][2], pl[p][3]};
        *reinterpret_cast<u32x4*>(dst + p * wpl) = o;
    }
}

}  // namespace

extern "C" size_t stm_conv_packed_weight_bytes_tiled(int Cout, int Cin, int kh, int kw, int planes, int tile_n)
{
    if (Cout <= 0 || Cin <= 0 || Cin % CV_BK || kh <= 0 || kw <= 0 || (planes < 1 || planes > 3) || (tile_n != 64 && tile_n != 128))
        return 0;
    return (size_t)stm_cdiv(Cout, tile_n) * (kh * kw * (Cin / CV_BK)) * planes * (tile_n * 64);
}

extern "C" size_t stm_conv_packed_weight_bytes(int Cout, int Cin, int kh, int kw, int planes)
{
    return stm_conv_packed_weight_bytes_tiled(Cout, Cin, kh, kw, planes, CV_BN);
}

extern "C" int stm_conv_pack_weights_fmt_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int tile_n, int fmt,
                                             float wscale, stm_stream_t stream);

extern "C" int stm_conv_pack_weights_tiled_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int planes,
                                               int tile_n, stm_stream_t stream)
{
    if (planes == 3) return stm_conv_pack_weights_fmt_f32(weight, packed, Cout, Cin, kh, kw, tile_n, 0, 1.0f, stream);
    STM_REQUIRE(weight && packed, STM_ENULL, "stm_conv_pack_weights_f32: weight/packed must be non-NULL");
    STM_REQUIRE(stm_conv_packed_weight_bytes_tiled(Cout, Cin, kh, kw, planes, tile_n) > 0, STM_EINVAL,
                "stm_conv_pack_weights_f32: bad sizes Cout=%d Cin=%d (multiple of 32) k=%dx%d planes=%d tile_n=%d (64 or 128)", Cout,
                Cin, kh, kw, planes, tile_n);
    STM_REQUIRE((uintptr_t)packed % 16 == 0, STM_EINVAL, "stm_conv_pack_weights_f32: packed buffer must be 16-byte aligned");
    const int slabs = kh * kw * (Cin / CV_BK), n_tiles = stm_cdiv(Cout, tile_n);
    const int64_t total = (int64_t)n_tiles * slabs * tile_n * 4;
    hipLaunchKernelGGL(conv_pack_weights_kernel, dim3(stm_cdiv(total, 256)), dim3(256), 0, stm_hs(stream), weight,
                       static_cast<uint8_t*>(packed), Cout, Cin, kh, kw, slabs, n_tiles, planes, tile_n, 0, 1.0f);
    STM_CHECK_LAUNCH("conv_pack_weights_kernel");
    return STM_OK;
}

extern "C" int stm_conv_pack_weights_fmt_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int tile_n, int fmt,
                                             float wscale, stm_stream_t stream)
{
    STM_REQUIRE(weight && packed, STM_ENULL, "stm_conv_pack_weights_fmt_f32: weight/packed must be non-NULL");
    STM_REQUIRE(fmt >= 0 && fmt <= 2, STM_EINVAL, "stm_conv_pack_weights_fmt_f32: fmt must be 0 (bf16 x 3), 1 (fp16 x 2) or 2 (fp16 x 1)");
    const int planes = fmt == 1 ? 2 : (fmt == 2 ? 1 : 3);
    STM_REQUIRE(stm_conv_packed_weight_bytes_tiled(Cout, Cin, kh, kw, planes, tile_n) > 0, STM_EINVAL,
                "stm_conv_pack_weights_fmt_f32: bad sizes Cout=%d Cin=%d (multiple of 32) k=%dx%d tile_n=%d (64 or 128)", Cout, Cin, kh, kw,
                tile_n);
    STM_REQUIRE((uintptr_t)packed % 16 == 0, STM_EINVAL, "stm_conv_pack_weights_fmt_f32: packed buffer must be 16-byte aligned");
    STM_REQUIRE(fmt == 0 || (wscale > 0.0f && wscale < 3.0e38f), STM_EINVAL, "stm_conv_pack_weights_fmt_f32: bad weight scale");
    const int slabs = kh * kw * (Cin / CV_BK), n_tiles = stm_cdiv(Cout, tile_n);
    const int64_t total = (int64_t)n_tiles * slabs * tile_n * 4;
    hipLaunchKernelGGL(conv_pack_weights_kernel, dim3(stm_cdiv(total, 256)), dim3(256), 0, stm_hs(stream), weight,
                       static_cast<uint8_t*>(packed), Cout, Cin, kh, kw, slabs, n_tiles, planes, tile_n, fmt, fmt >= 1 ? wscale : 1.0f);
    STM_CHECK_LAUNCH("conv_pack_weights_kernel");
    return STM_OK;
}

extern "C" int stm_conv_pack_weights_f32(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int planes,
                                         stm_stream_t stream)
{
    return stm_conv_pack_weights_tiled_f32(weight, packed, Cout, Cin, kh, kw, planes, CV_BN, stream);
}

extern "C" int stm_split_planes_fmt_f32(const float* x, void* planes, int64_t n_pixels, int C, int fmt, stm_stream_t stream);
extern "C" int stm_split_bf16_planes_f32(const float* x, void* planes, int64_t n_pixels, int C, stm_stream_t stream)
{
    return stm_split_planes_fmt_f32(x, planes, n_pixels, C, 0, stream);
}

extern "C" int stm_split_planes_fmt_f32(const float* x, void* planes, int64_t n_pixels, int C, int fmt, stm_stream_t stream)
{
    STM_REQUIRE(fmt >= 0 && fmt <= 2, STM_EINVAL, "stm_split_planes_fmt_f32: fmt must be 0 (bf16 x 3), 1 (fp16 x 2) or 2 (fp16 x 1)");
    STM_REQUIRE(x && planes, STM_ENULL, "stm_split_bf16_planes_f32: x/planes must be non-NULL");
    STM_REQUIRE(n_pixels > 0 && C > 0 && C % 32 == 0, STM_EINVAL, "stm_split_bf16_planes_f32: n_pixels (%lld) > 0 and C (%d) a multiple of 32",
                (long long)n_pixels, C);
    STM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)planes % 16 == 0, STM_EINVAL, "stm_split_bf16_planes_f32: 16-byte alignment required");
    hipLaunchKernelGGL(split_planes_kernel, dim3(stm_cdiv(n_pixels * (C / 8), 256)), dim3(256), 0, stm_hs(stream), x,
                       static_cast<uint8_t*>(planes), n_pixels, C, fmt, stm_internal_range_flag());
    STM_CHECK_LAUNCH("split_planes_kernel");
    return STM_OK;
}

extern "C" int stm_resize_bilinear_planes_f32(const float* x, void* planes, int B, int H, int W, int C, int Ho, int Wo, int fmt,
                                              stm_stream_t stream)
{
    STM_REQUIRE(fmt >= 0 && fmt <= 2, STM_EINVAL, "stm_resize_bilinear_planes_f32: fmt must be 0, 1 or 2");
    STM_REQUIRE(x && planes, STM_ENULL, "stm_resize_bilinear_planes_f32: x/planes must be non-NULL");
    STM_REQUIRE(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 32 == 0, STM_EINVAL,
                "stm_resize_bilinear_planes_f32: sizes must be positive and C (%d) a multiple of 32", C);
    STM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)planes % 16 == 0, STM_EINVAL, "stm_resize_bilinear_planes_f32: 16-byte alignment required");
    const int64_t n = (int64_t)B * Ho * Wo;
    // scale as ATen computes it for align_corners=false without an explicit scale factor: input size / output size
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    hipLaunchKernelGGL(resize_bilinear_planes_kernel, dim3(8 * stm_cdiv(stm_cdiv(n * (C / 8), 256), 8)), dim3(256), 0, stm_hs(stream), x,
                       static_cast<uint8_t*>(planes), B, H, W, C, Ho, Wo, sy, sx, fmt, stm_internal_range_flag());
    STM_CHECK_LAUNCH("resize_bilinear_planes_kernel");
    return STM_OK;
}

extern "C" int stm_bias_relu_maxpool_planes_f32(const float* x, const float* bias, void* planes, int B, int H, int W, int C, int fmt,
                                                stm_stream_t stream)
{
    STM_REQUIRE(fmt >= 0 && fmt <= 2, STM_EINVAL, "stm_bias_relu_maxpool_planes_f32: fmt must be 0, 1 or 2");
    STM_REQUIRE(x && planes, STM_ENULL, "stm_bias_relu_maxpool_planes_f32: x/planes must be non-NULL");
    STM_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0, STM_EINVAL,
                "stm_bias_relu_maxpool_planes_f32: sizes must be positive and C (%d) a multiple of 32", C);
    STM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)planes % 16 == 0, STM_EINVAL, "stm_bias_relu_maxpool_planes_f32: 16-byte alignment required");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;     // MaxPool2d(kernel 3, stride 2, padding 1), floor mode
    const int64_t n = (int64_t)B * Ho * Wo;
    hipLaunchKernelGGL(bias_relu_maxpool_planes_kernel, dim3(8 * stm_cdiv(stm_cdiv(n * (C / 8), 256), 8)), dim3(256), 0, stm_hs(stream), x, bias,
                       static_cast<uint8_t*>(planes), B, H, W, C, Ho, Wo, fmt, stm_internal_range_flag());
    STM_CHECK_LAUNCH("bias_relu_maxpool_planes_kernel");
    return STM_OK;
}

extern "C" int stm_roi_align_planes_nhwc_f32(const float* t2s_prev, const float* t2s, const float* corr, int corr_ld, const float* rois,
                                             void* planes, int B, int H, int W, int C1, int Cc, int n, int PH, int PW, int fmt, stm_stream_t stream);
extern "C" int stm_roi_align_planes_f32(const float* t2s_prev, const float* t2s, const float* corr, const float* rois, void* planes, int B,
                                        int H, int W, int C1, int Cc, int n, int PH, int PW, int fmt, stm_stream_t stream)
{
    return stm_roi_align_planes_nhwc_f32(t2s_prev, t2s, corr, 0, rois, planes, B, H, W, C1, Cc, n, PH, PW, fmt, stream);
}

extern "C" int stm_roi_align_planes_nhwc_f32(const float* t2s_prev, const float* t2s, const float* corr, int corr_ld, const float* rois,
                                             void* planes, int B, int H, int W, int C1, int Cc, int n, int PH, int PW, int fmt, stm_stream_t stream)
{
    STM_REQUIRE(corr_ld == 0 || (corr_ld >= (Cc + 7) / 8 * 8 && corr_ld % 4 == 0 && (uintptr_t)corr % 16 == 0), STM_EINVAL,
                "stm_roi_align_planes_nhwc_f32: corr_ld must be 0 (NCHW) or a multiple of 4 >= Cc rounded up to 8, corr 16-byte aligned");
    STM_REQUIRE(fmt >= 0 && fmt <= 2, STM_EINVAL, "stm_roi_align_planes_f32: fmt must be 0, 1 or 2");
    STM_REQUIRE(t2s_prev && t2s && corr && rois && planes, STM_ENULL, "stm_roi_align_planes_f32: NULL argument");
    STM_REQUIRE(B > 0 && H > 0 && W > 0 && C1 > 0 && C1 % 8 == 0 && Cc > 0 && n > 0 && PH > 0 && PW > 0, STM_EINVAL,
                "stm_roi_align_planes_f32: bad sizes (C1 = %d must be a multiple of 8)", C1);
    STM_REQUIRE((uintptr_t)t2s_prev % 16 == 0 && (uintptr_t)t2s % 16 == 0 && (uintptr_t)planes % 16 == 0, STM_EINVAL,
                "stm_roi_align_planes_f32: 16-byte alignment required");
    RoiPlanesArgs a;
    a.t2s_prev = t2s_prev; a.t2s = t2s; a.corr = corr; a.corr_ld = corr_ld; a.rois = rois; a.planes = static_cast<uint8_t*>(planes);
    a.n = n; a.H = H; a.W = W; a.C1 = C1; a.Cc = Cc; a.Cpad = (2 * C1 + Cc + 31) / 32 * 32; a.PH = PH; a.PW = PW; a.fmt = fmt;
    a.range_flag = stm_internal_range_flag();
    const int64_t threads = (int64_t)n * PH * PW * (a.Cpad / 8);
    // STM_ROI_TILED: 0 the first kernel (one pixel's channel groups per wave; the only form for an NCHW correlation volume), 1 (default) the tiled
    // kernel.  (A third form with the RoI's feature patch staged in LDS was bit-equal and slower -- 399 vs 272 us at 32 clips, 149 vs 80 at 8:
    // twenty slabs of stage / barrier / gather / barrier per workgroup, 196 of 256 lanes at work -- and was removed in round 7.)
    const int roi_form = STM_ENV_INT("STM_ROI_TILED", 1);
    if (corr_ld > 0 && roi_form) {
        const int64_t tiles = ((int64_t)n * PH * PW + 15) >> 4;
        hipLaunchKernelGGL(roi_align_planes_tiled_kernel, dim3(8 * stm_cdiv(tiles, 8)), dim3(256), 0, stm_hs(stream), a);
        STM_CHECK_LAUNCH("roi_align_planes_tiled_kernel");
        return STM_OK;
    }
    hipLaunchKernelGGL(roi_align_planes_kernel, dim3(8 * stm_cdiv(stm_cdiv(threads, 256), 8)), dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("roi_align_planes_kernel");
    return STM_OK;
}

extern "C" int stm_stem_rows_planes_f32(const float* x, void* planes, int B, int H, int W, int Cin, int kw, int sw, int pw, int fmt,
                                        stm_stream_t stream)
{
    STM_REQUIRE(fmt >= 0 && fmt <= 2, STM_EINVAL, "stm_stem_rows_planes_f32: fmt must be 0, 1 or 2");
    STM_REQUIRE(x && planes, STM_ENULL, "stm_stem_rows_planes_f32: x/planes must be non-NULL");
    STM_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && kw > 0 && sw > 0 && pw >= 0 && kw * Cin <= 32, STM_EINVAL,
                "stm_stem_rows_planes_f32: sizes must be positive and kw * Cin (%d) at most 32", kw * Cin);
    STM_REQUIRE((uintptr_t)planes % 16 == 0, STM_EINVAL, "stm_stem_rows_planes_f32: 16-byte alignment required");
    const int Wo = (W + 2 * pw - kw) / sw + 1;
    STM_REQUIRE(Wo > 0 && (int64_t)H * W * Cin < ((int64_t)1 << 31), STM_EINVAL, "stm_stem_rows_planes_f32: bad geometry");
    const int64_t n = (int64_t)B * H * Wo;
    hipLaunchKernelGGL(stem_rows_planes_kernel, dim3(8 * stm_cdiv(stm_cdiv(n * 4, 256), 8)), dim3(256), 0, stm_hs(stream), x,
                       static_cast<uint8_t*>(planes), B, H, W, Cin, kw, sw, pw, Wo, fmt, stm_internal_range_flag());
    STM_CHECK_LAUNCH("stem_rows_planes_kernel");
    return STM_OK;
}

// `_f16` forms (one fp16 plane, plane format 2; see conv_bf16x.hip)
extern "C" int stm_split_planes_f16(const float* x, void* planes, int64_t n_pixels, int C, stm_stream_t stream)
{
    return stm_split_planes_fmt_f32(x, planes, n_pixels, C, 2, stream);
}

extern "C" int stm_conv_pack_weights_f16(const float* weight, void* packed, int Cout, int Cin, int kh, int kw, int tile_n, float wscale,
                                         stm_stream_t stream)
{
    return stm_conv_pack_weights_fmt_f32(weight, packed, Cout, Cin, kh, kw, tile_n, 2, wscale, stream);
}
