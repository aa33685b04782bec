// extra_aug.hip -- ExtraAugmentation inside the training-batch kernels (extra_aug.h).  Three kernels share one
// __device__ function, aug_byte: the augmented image's byte triple at augmented-image coordinates, composed of RandomCrop's zeroing, Expand's
// nearest map and fill, the photometric chain in single-rounded fp32 (-ffp-contract=off) and the uint8 cast of the reference's assignment.
//   frames  data_frames_kernel (train_data.hip) with the four taps of the 8-bit bilinear resize read through aug_byte;
//   masks   data_masks_kernel with the same coordinate maps between the target pixel and the run-list lookup;
//   source  aug_byte for every pixel of the augmented image, uint8 HWC: the tool for looking at an augmentation.
// The per-frame descriptors (112 bytes) are read from device memory at a wavefront-uniform index.  Integer arithmetic and fixed orders, no
// atomics, no LDS: the same bytes from run to run.  stmask_amd/datasets.py is the caller.
#include "stm_common.h"
#include "preprocess_common.h"
#include "extra_aug.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int AUG_MASK_ROWS = 16;      // as TD_MASK_ROWS / TD_LANE_PX of train_data.hip
constexpr int AUG_LANE_PX = 4;

__device__ __forceinline__ float sel4(int i, float t0, float t1, float t2, float t3)
{
    return i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3;
}

__device__ __forceinline__ float sel3(int i, float t0, float t1, float t2)
{
    return i == 0 ? t0 : i == 1 ? t1 : t2;
}

// PhotoMetricDistortion on one BGR pixel, every step one fp32 operation (extra_aug.h, item 3)
__device__ __forceinline__ void aug_photometric(const stm_aug_desc& d, float& b, float& g, float& r)
{
    b += d.delta;
    g += d.delta;
    r += d.delta;
    b *= d.alpha_pre;
    g *= d.alpha_pre;
    r *= d.alpha_pre;
    // BGR -> HSV
    const float v = fmaxf(fmaxf(b, g), r), vmin = fminf(fminf(b, g), r);
    const float diff = v - vmin;
    float s = diff / (fabsf(v) + FLT_EPSILON);
    const float k = (float)(60.0 / (double)(diff + FLT_EPSILON));
    float h = v == r ? (g - b) * k : v == g ? (b - r) * k + 120.0f : (r - g) * k + 240.0f;
    if (h < 0.0f) h += 360.0f;
    // saturation and hue
    s *= d.saturation;
    h += d.hue;
    if (h > 360.0f) h -= 360.0f;
    if (h < 0.0f) h += 360.0f;
    // HSV -> BGR
    if (s == 0.0f) {
        b = g = r = v;
    } else {
        h *= 6.0f / 360.0f;
        if (h < 0.0f) {
            do h += 6.0f;
            while (h < 0.0f);
        } else if (h >= 6.0f) {
            do h -= 6.0f;
            while (h >= 6.0f);
        }
        int sector = (int)floorf(h);
        h -= (float)sector;
        if ((unsigned)sector >= 6u) {
            sector = 0;
            h = 0.0f;
        }
        const float t0 = v, t1 = v * (1.0f - s), t2 = v * (1.0f - s * h), t3 = v * (1.0f - s * (1.0f - h));
        // the sector table as selects (an indexed local array would live in scratch): 2 bits per sector, sector 0 in the low bits
        //   b: 1 1 3 0 0 2    g: 3 0 0 2 1 1    r: 0 2 1 1 3 0
        const int sh = 2 * sector;
        b = sel4((0x835 >> sh) & 3, t0, t1, t2, t3);
        g = sel4((0x583 >> sh) & 3, t0, t1, t2, t3);
        r = sel4((0x358 >> sh) & 3, t0, t1, t2, t3);
    }
    b *= d.alpha_post;
    g *= d.alpha_post;
    r *= d.alpha_post;
    const float pb = sel3(d.perm[0], b, g, r), pg = sel3(d.perm[1], b, g, r), pr = sel3(d.perm[2], b, g, r);
    b = pb;
    g = pg;
    r = pr;
}

// numpy's float -> uint8 assignment for these magnitudes: truncate toward zero, keep the low 8 bits; or clip first
__device__ __forceinline__ unsigned char aug_cast(float x, int clip)
{
    if (clip) x = fminf(fmaxf(x, 0.0f), 255.0f);
    return (unsigned char)((int)x & 255);
}

// The augmented image's bytes at (sy, sx), 0 <= sy < H0, 0 <= sx < W0.  Every source read is at a pixel inside [0, H0) x [0, W0).
__device__ __forceinline__ uchar3 aug_byte(const stm_aug_desc& d, int sy, int sx)
{
    if (sx < d.x0 || sx >= d.x1 || sy < d.y0 || sy >= d.y1) return make_uchar3(0, 0, 0);
    const int cy = resize_nearest(sy, d.Hc, d.H0) - d.top, cx = resize_nearest(sx, d.Wc, d.W0) - d.left;
    float b = d.fill[0], g = d.fill[1], r = d.fill[2];
    if (cy >= 0 && cy < d.H0 && cx >= 0 && cx < d.W0) {
        const uint8_t* px = d.ptr + (int64_t)cy * d.row_stride_bytes + 3 * cx;
        b = (float)px[0];
        g = (float)px[1];
        r = (float)px[2];
        if (d.photo) aug_photometric(d, b, g, r);
    }
    return make_uchar3(aug_cast(b, d.cast_clip), aug_cast(g, d.cast_clip), aug_cast(r, d.cast_clip));
}

// One tap pair -> one channel of the cv2 8-bit bilinear resize and its normalisation: the integer and double sequence of preprocess_pixel
// (preprocess_common.h, mode 1), whose taps come from memory.
__device__ __forceinline__ float aug_channel(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1, double mean, double stdv)
{
    const int D0 = p00 * a0 + p01 * a1;
    const int D1 = p10 * a0 + p11 * a1;
    int v = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2;
    v = min(max(v, 0), 255);
    return (float)(((double)v - mean) / stdv);
}

// thread = one output pixel, three channels (the colour function needs the triple); blockIdx.z = frame within the chunk
__global__ __launch_bounds__(256) void aug_frames_kernel(const stm_aug_desc* __restrict__ desc, float* __restrict__ out, int h, int w, int Hp, int Wp,
                                                         double m0, double m1, double m2, double s0, double s1, double s2, int to_rgb)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int i = blockIdx.z;
    if (x >= Wp || y >= Hp) return;
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (y < h && x < w) {
        const stm_aug_desc d = desc[i];
        int sx, sy, a0, a1, b0, b1;
        resize_coeffs(d.W0, w, d.flip ? w - 1 - x : x, true, sx, a0, a1);
        resize_coeffs(d.H0, h, y, false, sy, b0, b1);
        const int sx1 = min(sx + 1, d.W0 - 1);
        const int y0 = min(max(sy, 0), d.H0 - 1), y1 = min(max(sy + 1, 0), d.H0 - 1);
        const uchar3 p00 = aug_byte(d, y0, sx), p01 = aug_byte(d, y0, sx1), p10 = aug_byte(d, y1, sx), p11 = aug_byte(d, y1, sx1);
        // the constants are in the output's channel order: with to_rgb source channel c lands in output channel 2 - c
        const float c0 = aug_channel(p00.x, p01.x, p10.x, p11.x, a0, a1, b0, b1, to_rgb ? m2 : m0, to_rgb ? s2 : s0);
        const float c1 = aug_channel(p00.y, p01.y, p10.y, p11.y, a0, a1, b0, b1, m1, s1);
        const float c2 = aug_channel(p00.z, p01.z, p10.z, p11.z, a0, a1, b0, b1, to_rgb ? m0 : m2, to_rgb ? s0 : s2);
        o0 = to_rgb ? c2 : c0;
        o1 = c1;
        o2 = to_rgb ? c0 : c2;
    }
    const size_t plane = (size_t)Hp * Wp, at = (size_t)i * 3 * plane + (size_t)y * Wp + x;
    out[at] = o0;
    out[at + plane] = o1;
    out[at + 2 * plane] = o2;
}

// grid (n, ceil(Hp / 16), ceil(Wp / 256)), block 64: data_masks_kernel's walk (lanes along x, four output pixels each, 16 rows; the first live
// row of a column finds its run by binary search, the rows below move a cursor) with the augmentation's maps between the target pixel and the
// lookup.  Both maps are non-decreasing in y, so for a fixed column the source index k still rises over the rows that land on the source.
__global__ __launch_bounds__(STM_WAVE) void aug_masks_kernel(const unsigned int* __restrict__ starts, const int64_t* __restrict__ off,
                                                             const int* __restrict__ n_runs, int n_lists,
                                                             const stm_data_mask_desc* __restrict__ mdesc, const int* __restrict__ frame_of,
                                                             const stm_aug_desc* __restrict__ adesc, int n_frames, int64_t total,
                                                             unsigned char* __restrict__ out, int h, int w, int Hp, int Wp)
{
    const int64_t i = blockIdx.x;
    const int y_begin = blockIdx.y * AUG_MASK_ROWS;
    const int x4 = (blockIdx.z * STM_WAVE + threadIdx.x) * AUG_LANE_PX;
    if (x4 >= Wp) return;
    const stm_data_mask_desc d = mdesc[i];
    const int fi = frame_of[i];
    const bool framed = fi >= 0 && fi < n_frames;
    const stm_aug_desc a = adesc[framed ? fi : 0];
    const bool listed = d.list >= 0 && d.list < n_lists;
    const int m = listed ? d.list : 0;
    int64_t c0, c1;
    stm_slot(off, m, total, c0, c1);
    const int nr = listed ? (int)min((int64_t)max(n_runs[m], 0), min(c1 - c0, (int64_t)INT_MAX)) : 0;
    const bool live = framed && nr > 0 && d.H0 > 0 && d.W0 > 0 && a.Hc > 0 && a.Wc > 0;
    const unsigned int* __restrict__ st = starts + c0;

    unsigned int kbase[AUG_LANE_PX];
    int cur[AUG_LANE_PX];
    bool inside[AUG_LANE_PX];
#pragma unroll
    for (int c = 0; c < AUG_LANE_PX; ++c) {
        const int x = x4 + c;
        bool ok = live && x < w;
        int cx = 0;
        if (ok) {
            const int ax = resize_nearest(d.flip ? w - 1 - x : x, d.W0, w);             // the augmented image's column
            cx = resize_nearest(ax, a.Wc, d.W0) - a.left;                               // the source's
            ok = ax >= a.x0 && ax < a.x1 && cx >= 0 && cx < d.W0;
        }
        inside[c] = ok;
        kbase[c] = ok ? (unsigned int)cx * (unsigned int)d.H0 : 0u;
        cur[c] = -1;
    }
    const int y_end = min(y_begin + AUG_MASK_ROWS, Hp);
    for (int y = y_begin; y < y_end; ++y) {
        unsigned int word = 0;
        if (live && y < h) {
            const int ay = resize_nearest(y, d.H0, h);
            const int cy = resize_nearest(ay, a.Hc, d.H0) - a.top;
            if (ay >= a.y0 && ay < a.y1 && cy >= 0 && cy < d.H0) {
#pragma unroll
                for (int c = 0; c < AUG_LANE_PX; ++c) {
                    if (!inside[c]) continue;
                    const unsigned int k = kbase[c] + (unsigned int)cy;
                    int j = cur[c];
                    if (j < 0) {                                     // the last run whose start is <= k: starts[0] = 0, so there is one
                        int lo = 0, hi = nr;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (st[mid] <= k) lo = mid + 1;
                            else hi = mid;
                        }
                        j = max(lo - 1, 0);
                    } else {
                        while (j + 1 < nr && st[j + 1] <= k) ++j;
                    }
                    cur[c] = j;
                    word |= (unsigned int)(j & 1) << (8 * c);
                }
            }
        }
        *reinterpret_cast<unsigned int*>(out + ((size_t)i * Hp + y) * Wp + x4) = word;
    }
}

// thread = one pixel of the augmented image
__global__ __launch_bounds__(256) void aug_source_kernel(const stm_aug_desc* __restrict__ desc, unsigned char* __restrict__ out)
{
    const stm_aug_desc d = desc[0];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= d.W0 || y >= d.H0) return;
    const uchar3 p = aug_byte(d, y, x);
    unsigned char* o = out + ((size_t)y * d.W0 + x) * 3;
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.z;
}

// what the kernels rely on for their source reads, checked on the host copy
int aug_check_desc(const char* who, const stm_aug_desc& d, int i)
{
    STM_REQUIRE(d.ptr, STM_ENULL, "%s: frame %d has a NULL pointer", who, i);
    STM_REQUIRE(d.H0 > 0 && d.W0 > 0 && d.row_stride_bytes >= 3 * (int64_t)d.W0, STM_EINVAL, "%s: frame %d: bad source size %dx%d (row stride %lld bytes)",
                who, i, d.H0, d.W0, (long long)d.row_stride_bytes);
    STM_REQUIRE(d.top >= 0 && d.left >= 0 && d.Hc >= d.H0 && d.Wc >= d.W0 && (int64_t)d.top + d.H0 <= d.Hc && (int64_t)d.left + d.W0 <= d.Wc, STM_EINVAL,
                "%s: frame %d: the canvas %dx%d does not hold the %dx%d source at (%d, %d)", who, i, d.Hc, d.Wc, d.H0, d.W0, d.top, d.left);
    STM_REQUIRE(0 <= d.x0 && d.x0 <= d.x1 && d.x1 <= d.W0 && 0 <= d.y0 && d.y0 <= d.y1 && d.y1 <= d.H0, STM_EINVAL,
                "%s: frame %d: the patch (%d, %d, %d, %d) is not inside the %dx%d image", who, i, d.x0, d.y0, d.x1, d.y1, d.H0, d.W0);
    for (int c = 0; c < 3; ++c)
        STM_REQUIRE(d.perm[c] >= 0 && d.perm[c] <= 2, STM_EINVAL, "%s: frame %d: perm[%d]=%d", who, i, c, d.perm[c]);
    return STM_OK;
}

}  // namespace

extern "C" size_t stm_aug_struct_bytes(int which)
{
    return which == 0 ? sizeof(stm_aug_desc) : 0;
}

extern "C" int stm_aug_frames_u8_f32(const stm_aug_desc* desc_host, const stm_aug_desc* desc_dev, int n, float* out, int h, int w, int Hp, int Wp,
                                     const double* mean, const double* stdv, int to_rgb, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL, "stm_aug_frames_u8_f32: bad sizes n=%d dst=%dx%d padded=%dx%d", n, h, w, Hp,
                Wp);
    if (n == 0) return STM_OK;
    STM_REQUIRE(desc_host && desc_dev && out && mean && stdv, STM_ENULL, "stm_aug_frames_u8_f32: desc_host/desc_dev/out/mean/stdv must be non-NULL");
    STM_REQUIRE(stm_cdiv(Hp, 4) <= 65535, STM_EINVAL, "stm_aug_frames_u8_f32: output %dx%d too large", Hp, Wp);
    for (int i = 0; i < n; ++i) {
        const int rc = aug_check_desc("stm_aug_frames_u8_f32", desc_host[i], i);
        if (rc != STM_OK) return rc;
    }
    for (int i0 = 0; i0 < n; i0 += STM_AUG_FRAMES_PER_LAUNCH) {
        const int k = min(STM_AUG_FRAMES_PER_LAUNCH, n - i0);
        const dim3 grid(stm_cdiv(Wp, 64), stm_cdiv(Hp, 4), k);
        hipLaunchKernelGGL(aug_frames_kernel, grid, dim3(256), 0, stm_hs(stream), desc_dev + i0, out + (size_t)i0 * 3 * Hp * Wp, h, w, Hp, Wp, mean[0],
                           mean[1], mean[2], stdv[0], stdv[1], stdv[2], to_rgb ? 1 : 0);
        STM_CHECK_LAUNCH("aug_frames_kernel");
    }
    return STM_OK;
}

extern "C" int stm_aug_masks_u8(const unsigned int* starts, const int64_t* offsets, const int* n_runs, int n_lists, const stm_data_mask_desc* mask_desc,
                                const int* frame_of, const stm_aug_desc* desc_dev, int n_frames, int n, int64_t total_runs, unsigned char* out, int h,
                                int w, int Hp, int Wp, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && n_lists >= 1 && n_frames >= 1 && total_runs >= 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL,
                "stm_aug_masks_u8: bad sizes n=%d n_frames=%d dst=%dx%d padded=%dx%d", n, n_frames, h, w, Hp, Wp);
    STM_REQUIRE(Wp % AUG_LANE_PX == 0, STM_EINVAL, "stm_aug_masks_u8: the padded width %d must be a multiple of %d", Wp, AUG_LANE_PX);
    if (n == 0) return STM_OK;
    STM_REQUIRE(offsets && n_runs && mask_desc && frame_of && desc_dev && out && (total_runs == 0 || starts), STM_ENULL,
                "stm_aug_masks_u8: NULL argument");
    STM_REQUIRE((uintptr_t)out % 4 == 0, STM_EINVAL, "stm_aug_masks_u8: out must be 4-byte aligned");
    const int bands = stm_cdiv(Hp, AUG_MASK_ROWS), chunks = stm_cdiv(Wp, STM_WAVE * AUG_LANE_PX);
    STM_REQUIRE(bands <= 65535 && chunks <= 65535, STM_EINVAL, "stm_aug_masks_u8: output %dx%d too large", Hp, Wp);
    hipLaunchKernelGGL(aug_masks_kernel, dim3(n, bands, chunks), dim3(STM_WAVE), 0, stm_hs(stream), starts, offsets, n_runs, n_lists, mask_desc, frame_of,
                       desc_dev, n_frames, total_runs, out, h, w, Hp, Wp);
    STM_CHECK_LAUNCH("aug_masks_kernel");
    return STM_OK;
}

extern "C" int stm_aug_source_u8(const stm_aug_desc* desc_host, const stm_aug_desc* desc_dev, unsigned char* out, stm_stream_t stream)
{
    STM_REQUIRE(desc_host && desc_dev && out, STM_ENULL, "stm_aug_source_u8: desc_host/desc_dev/out must be non-NULL");
    const int rc = aug_check_desc("stm_aug_source_u8", desc_host[0], 0);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(stm_cdiv(desc_host->H0, 4) <= 65535, STM_EINVAL, "stm_aug_source_u8: source %dx%d too large", desc_host->H0, desc_host->W0);
    hipLaunchKernelGGL(aug_source_kernel, dim3(stm_cdiv(desc_host->W0, 64), stm_cdiv(desc_host->H0, 4)), dim3(256), 0, stm_hs(stream), desc_dev, out);
    STM_CHECK_LAUNCH("aug_source_kernel");
    return STM_OK;
}
