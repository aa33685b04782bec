// output.hip -- output stage on the device: the mask leg of postprocess_ytbvis
// (layers/output_utils.py:85-106) -- un-pad, bilinear resize to the original frame size, threshold at 0.5 and
// COCO run-length encoding -- without ever materialising the full-resolution masks in host memory.
//
// The reference copies every [ori_h, ori_w] mask to the host (`.cpu()`, output_utils.py:103) and run-length encodes it
// with pycocotools: 921 KB per mask at 720p.  Here two integer/byte kernels leave only the run lengths (a few hundred
// 32-bit counts per mask) to be copied:
//   1. resize + threshold + bit-pack: lanes walk the COLUMN-major pixel order RLE needs (consecutive lanes = consecutive
//      rows of one column), a wavefront ballot turns 64 pixels into one 64-bit word;
//   2. run extraction, one workgroup per mask: transitions are the set bits of w ^ ((w << 1) | carry); per-word
//      popcounts are prefix-summed across the workgroup, every thread then emits its words' transition positions in
//      order and the counts are the first differences.
// Arithmetic follows ATen's bilinear kernel (align_corners=False) in fp32, operand order as in oracle/stm_oracle.c, so
// the bits agree with the oracle exactly (-ffp-contract=off).
#include "stm_common.h"
#include "rle_common.h"
#include "preprocess_common.h"

namespace {

__global__ __launch_bounds__(256) void resize_threshold_pack_kernel(const float* __restrict__ masks, int mh, int mw,
                                                                    int crop_h, int crop_w, int out_h, int out_w, float thr,
                                                                    unsigned long long* __restrict__ bits, int words)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int word = blockIdx.x * 4 + wave;
    const int i = blockIdx.y;
    if (word >= words) return;
    const int64_t p = (int64_t)word * 64 + lane;   // column-major pixel index: p = x * out_h + y
    bool b = false;
    if (p < (int64_t)out_h * out_w) {
        const int x = (int)(p / out_h), y = (int)(p - (int64_t)x * out_h);
        const float* m = masks + (int64_t)i * mh * mw;
        int y0, y1, x0, x1;
        float ly, hy, lx, hx;
        stm_bilinear_tap(y, (float)crop_h / (float)out_h, crop_h, y0, y1, ly, hy);
        stm_bilinear_tap(x, (float)crop_w / (float)out_w, crop_w, x0, x1, lx, hx);
        b = stm_bilinear_blend(m, mw, y0, y1, x0, x1, ly, hy, lx, hx) > thr;
    }
    const unsigned long long bal = __ballot(b);
    if (lane == 0) bits[(int64_t)i * words + word] = bal;
}

// one workgroup per mask; counts[i][0..n_runs[i]) (capacity max_runs; n_runs reports the true number): rle_common.h
__global__ __launch_bounds__(1024) void rle_runs_kernel(const unsigned long long* __restrict__ bits, int words, int64_t n_px,
                                                        unsigned int* __restrict__ counts, int max_runs, int* __restrict__ n_runs,
                                                        unsigned int* __restrict__ trans_ws)
{
    __shared__ int wave_tot[16];
    const int i = blockIdx.x;
    const int nr = stm_rle_runs_block(bits + (int64_t)i * words, words, n_px, trans_ws + (int64_t)i * max_runs, counts + (int64_t)i * max_runs,
                                      max_runs, wave_tot);
    if (threadIdx.x == 0) n_runs[i] = nr;
}

}  // namespace

extern "C" size_t stm_mask_rle_workspace_bytes(int n, int out_h, int out_w, int max_runs)
{
    size_t words = ((size_t)out_h * out_w + 63) / 64;
    return (size_t)n * words * 8 + (size_t)n * max_runs * 4 + 256;
}

extern "C" int stm_mask_resize_rle_f32(const float* masks, int n, int mh, int mw, int crop_h, int crop_w, int out_h, int out_w,
                                       float thr, uint32_t* counts, int max_runs, int* n_runs, void* workspace,
                                       size_t workspace_bytes, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0, STM_EINVAL, "stm_mask_resize_rle_f32: n=%d", n);
    if (n == 0) return STM_OK;
    STM_REQUIRE(masks && counts && n_runs, STM_ENULL, "stm_mask_resize_rle_f32: masks/counts/n_runs must be non-NULL");
    STM_REQUIRE(mh > 0 && mw > 0 && crop_h > 0 && crop_h <= mh && crop_w > 0 && crop_w <= mw && out_h > 0 && out_w > 0,
                STM_EINVAL, "stm_mask_resize_rle_f32: bad sizes");
    STM_REQUIRE((int64_t)out_h * out_w < ((int64_t)1 << 31) && max_runs > 0 && n <= 65535, STM_EINVAL,
                "stm_mask_resize_rle_f32: output too large");
    STM_REQUIRE(workspace && workspace_bytes >= stm_mask_rle_workspace_bytes(n, out_h, out_w, max_runs), STM_EWORKSPACE,
                "stm_mask_resize_rle_f32: workspace too small");
    const int64_t n_px = (int64_t)out_h * out_w;
    const int words = (int)((n_px + 63) / 64);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(workspace);
    unsigned int* trans = reinterpret_cast<unsigned int*>(bits + (size_t)n * words);
    hipLaunchKernelGGL(resize_threshold_pack_kernel, dim3(stm_cdiv(words, 4), n), dim3(256), 0, stm_hs(stream), masks, mh, mw,
                       crop_h, crop_w, out_h, out_w, thr, bits, words);
    STM_CHECK_LAUNCH("resize_threshold_pack_kernel");
    hipLaunchKernelGGL(rle_runs_kernel, dim3(n), dim3(1024), 0, stm_hs(stream), bits, words, n_px, counts, max_runs, n_runs,
                       trans);
    STM_CHECK_LAUNCH("rle_runs_kernel");
    return STM_OK;
}


// ---- frame pre-processing: eval.py:703-717 = mmcv.imresize (cv2 INTER_LINEAR on uint8) ->
// (im - MEANS) / STD in float64 -> zero pad to a multiple of 32 -> CHW fp32, as ONE pass over the output.  The 8-bit
// bilinear arithmetic is OpenCV's fixed-point path, restated in oracle/stm_oracle.c (orc_resize_pixel_u8) with the
// derivation; this kernel performs the identical integer / float / double operation sequence, so the two agree bit
// for bit.  Thread = one output pixel, three channels; HBM-bound (2.8 MB in, 2.9 MB out per 720p frame).  The per-pixel sequence itself
// (resize_coeffs, preprocess_pixel) lives in preprocess_common.h, shared with the training frames of train_data.hip.
namespace {

__global__ __launch_bounds__(256) void preprocess_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int H0, int W0,
                                                            int h, int w, int Hp, int Wp, double m0, double m1, double m2, double s0,
                                                            double s1, double s2, int mode)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int i = blockIdx.z;
    if (x >= Wp || y >= Hp) return;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (y < h && x < w) {
        const double mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
        preprocess_pixel(img + (size_t)i * H0 * W0 * 3, (int64_t)W0 * 3, H0, W0, h, w, x, y, mean, stdv, mode, o);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(((size_t)i * 3 + c) * Hp + y) * Wp + x] = o[c];
}

// Up to 64 frames of different source sizes (and tensors) per launch: the descriptors travel in the kernel argument, so a launch needs no
// host -> device copy and can be captured in a graph.  blockIdx.z = frame within the chunk.
constexpr int kMultiFrames = 64;
struct PreprocessMultiArgs {
    stm_frame_desc f[kMultiFrames];
};

__global__ __launch_bounds__(256) void preprocess_u8_multi_kernel(const PreprocessMultiArgs a, float* __restrict__ out, int h, int w, int Hp, int Wp,
                                                                  double m0, double m1, double m2, double s0, double s1, double s2, int mode)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int i = blockIdx.z;
    if (x >= Wp || y >= Hp) return;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (y < h && x < w) {
        const stm_frame_desc d = a.f[i];
        const double mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
        preprocess_pixel(d.ptr, d.row_stride_bytes, d.H0, d.W0, h, w, x, y, mean, stdv, mode, o);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(((size_t)i * 3 + c) * Hp + y) * Wp + x] = o[c];
}

}  // namespace

extern "C" int stm_preprocess_u8_f32(const uint8_t* img, float* out, int n, int H0, int W0, int h, int w, int Hp, int Wp,
                                     const double* mean, const double* stdv, int mode, stm_stream_t stream)
{
    STM_REQUIRE(img && out, STM_ENULL, "stm_preprocess_u8_f32: img/out must be non-NULL");
    STM_REQUIRE(n > 0 && n <= 65535 && H0 > 0 && W0 > 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL,
                "stm_preprocess_u8_f32: bad sizes n=%d src=%dx%d dst=%dx%d padded=%dx%d", n, H0, W0, h, w, Hp, Wp);
    STM_REQUIRE(mode >= 0 && mode <= 3, STM_EINVAL, "stm_preprocess_u8_f32: mode %d not in 0..3", mode);
    STM_REQUIRE(mode == 0 || mode == 3 || (mean && (mode == 2 || stdv)), STM_ENULL, "stm_preprocess_u8_f32: mean/std needed for mode %d", mode);
    const double m[3] = {mean ? mean[0] : 0.0, mean ? mean[1] : 0.0, mean ? mean[2] : 0.0};
    const double s[3] = {stdv ? stdv[0] : 1.0, stdv ? stdv[1] : 1.0, stdv ? stdv[2] : 1.0};
    const dim3 grid(stm_cdiv(Wp, 64), stm_cdiv(Hp, 4), n);
    hipLaunchKernelGGL(preprocess_u8_kernel, grid, dim3(256), 0, stm_hs(stream), img, out, H0, W0, h, w, Hp, Wp, m[0], m[1], m[2],
                       s[0], s[1], s[2], mode);
    STM_CHECK_LAUNCH("preprocess_u8_kernel");
    return STM_OK;
}

extern "C" int stm_preprocess_u8_multi_f32(const stm_frame_desc* frames, int n, float* out, int h, int w, int Hp, int Wp, const double* mean,
                                           const double* stdv, int mode, stm_stream_t stream)
{
    STM_REQUIRE(frames && out, STM_ENULL, "stm_preprocess_u8_multi_f32: frames/out must be non-NULL");
    STM_REQUIRE(n > 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL, "stm_preprocess_u8_multi_f32: bad sizes n=%d dst=%dx%d padded=%dx%d",
                n, h, w, Hp, Wp);
    STM_REQUIRE(mode >= 0 && mode <= 3, STM_EINVAL, "stm_preprocess_u8_multi_f32: mode %d not in 0..3", mode);
    STM_REQUIRE(mode == 0 || mode == 3 || (mean && (mode == 2 || stdv)), STM_ENULL, "stm_preprocess_u8_multi_f32: mean/std needed for mode %d", mode);
    for (int i = 0; i < n; ++i) {
        const stm_frame_desc& d = frames[i];
        STM_REQUIRE(d.ptr, STM_ENULL, "stm_preprocess_u8_multi_f32: frame %d has a NULL pointer", i);
        STM_REQUIRE(d.H0 > 0 && d.W0 > 0 && d.row_stride_bytes >= 3 * (int64_t)d.W0, STM_EINVAL,
                    "stm_preprocess_u8_multi_f32: frame %d: bad source size %dx%d (row stride %lld bytes)", i, d.H0, d.W0,
                    (long long)d.row_stride_bytes);
    }
    const double m[3] = {mean ? mean[0] : 0.0, mean ? mean[1] : 0.0, mean ? mean[2] : 0.0};
    const double s[3] = {stdv ? stdv[0] : 1.0, stdv ? stdv[1] : 1.0, stdv ? stdv[2] : 1.0};
    for (int i0 = 0; i0 < n; i0 += kMultiFrames) {
        const int k = min(kMultiFrames, n - i0);
        PreprocessMultiArgs a = {};
        for (int i = 0; i < k; ++i) a.f[i] = frames[i0 + i];
        const dim3 grid(stm_cdiv(Wp, 64), stm_cdiv(Hp, 4), k);
        hipLaunchKernelGGL(preprocess_u8_multi_kernel, grid, dim3(256), 0, stm_hs(stream), a, out + (size_t)i0 * 3 * Hp * Wp, h, w, Hp, Wp,
                           m[0], m[1], m[2], s[0], s[1], s[2], mode);
        STM_CHECK_LAUNCH("preprocess_u8_multi_kernel");
    }
    return STM_OK;
}
