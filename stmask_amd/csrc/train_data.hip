// train_data.hip -- training batches on the device (include/stmask_hip_data.h): what datasets/ytvos.py prepare_train_img and
// datasets/transforms.py do per sample on the host, for img_scale=[(w, h)] and resize_keep_ratio=False.
//   frames  uint8 HWC sources of unequal sizes -> cv2 8-bit bilinear resize, to_rgb, (v - mean) / std, flip, pad, CHW fp32 (preprocess_common.h:
//           the per-pixel sequence of the inference pre-processing, so flip = 0 / to_rgb = 0 gives its bits);
//   masks   COCO run lengths -> exclusive prefix sums ("starts", one wavefront per mask) -> the resized, flipped, padded uint8 target: every
//           output pixel looks its source pixel's column-major index up in the starts.  Nothing at source resolution is ever written;
//   boxes   BboxTransform in fp32, one rounding per step (-ffp-contract=off).
// Integer arithmetic and fixed orders, no atomics: the same bytes from run to run.  stmask_amd/datasets.py is the caller.
#include "stm_common.h"
#include "preprocess_common.h"
#include "../../include/stmask_hip_data.h"
#include <limits.h>

namespace {

constexpr int TD_THREADS = 256;
constexpr int TD_WAVES = TD_THREADS / STM_WAVE;
constexpr int TD_FRAMES = 64;          // frame descriptors per launch (2 KiB of kernel arguments)
constexpr int TD_MASK_ROWS = 16;       // output rows a wavefront of the mask kernel walks: one binary search per column, then a cursor
constexpr int TD_LANE_PX = 4;          // output pixels of a row per lane: one 4-byte store; a wavefront's 64 stores are 256 contiguous bytes

struct FrameArgs {
    stm_data_frame_desc f[TD_FRAMES];
};

// thread = one output pixel, three channels (the mapping of preprocess_u8_multi_kernel); blockIdx.z = frame within the chunk
__global__ __launch_bounds__(256) void data_frames_kernel(const FrameArgs a, float* __restrict__ out, int h, int w, int Hp, int Wp, double m0,
                                                          double m1, double m2, double s0, double s1, double s2, int to_rgb)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int i = blockIdx.z;
    if (x >= Wp || y >= Hp) return;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (y < h && x < w) {
        const stm_data_frame_desc d = a.f[i];
        // preprocess_pixel indexes its constants by the source channel: with to_rgb source channel c lands in output channel 2 - c
        const double mean[3] = {to_rgb ? m2 : m0, m1, to_rgb ? m0 : m2}, stdv[3] = {to_rgb ? s2 : s0, s1, to_rgb ? s0 : s2};
        preprocess_pixel(d.ptr, d.row_stride_bytes, d.H0, d.W0, h, w, d.flip ? w - 1 - x : x, y, mean, stdv, 1, o);
        if (to_rgb) {
            const float t = o[0];
            o[0] = o[2];
            o[2] = t;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(((size_t)i * 3 + c) * Hp + y) * Wp + x] = o[c];
}

// grid ceil(n / 4), block 256: a wavefront per mask, 64 runs per pass, the total so far carried from pass to pass
__global__ __launch_bounds__(TD_THREADS) void data_rle_starts_kernel(const unsigned int* __restrict__ runs, const int64_t* __restrict__ off,
                                                                     const int* n_runs_in, const int* status_in, const int64_t* __restrict__ hw,
                                                                     int n, int64_t total, unsigned int* __restrict__ starts, int* n_runs,
                                                                     int64_t* __restrict__ area, int* status)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * TD_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wavefront-uniform
    int64_t c0, c1;
    stm_slot(off, i, total, c0, c1);
    int st = status_in ? status_in[i] : 0;
    int64_t cnt = c1 - c0;
    if (n_runs_in) cnt = min(cnt, (int64_t)max(n_runs_in[i], 0));
    if (cnt > INT_MAX) {
        st |= STM_VIS_RLE_RANGE;
        cnt = 0;
    }
    unsigned long long carry = 0;
    long long sum_odd = 0;
    for (int64_t b = 0; b < cnt; b += 64) {
        const int64_t p = b + lane;
        const bool in = p < cnt;
        const unsigned long long v = in ? (unsigned long long)runs[c0 + p] : 0ull;
        const unsigned long long incl = stm_wave_scan_u64(v, lane);
        if (in) {
            starts[c0 + p] = (unsigned int)(carry + incl - v);
            if (p & 1) sum_odd += (long long)v;
        }
        carry += __shfl(incl, 63, STM_WAVE);
    }
    sum_odd = stm_wave_sum_i64(sum_odd);
    if (!st && carry != (unsigned long long)hw[i]) st |= STM_VIS_RLE_SUM;
    if (lane == 0) {
        n_runs[i] = st ? 0 : (int)cnt;
        area[i] = st ? 0 : sum_odd;
        status[i] = st;
    }
}

// grid (n, ceil(Hp / 16), ceil(Wp / 256)), block 64: lanes lie along x, four output pixels each, and walk 16 rows.  For a fixed output column
// the source index k = sx * H0 + sy rises with y: the first row finds its run by binary search in the mask's starts, the rows below move a
// cursor.  Every lane stores one 32-bit word per row, pad and flagged masks (zeros) included.
__global__ __launch_bounds__(STM_WAVE) void data_masks_kernel(const unsigned int* __restrict__ starts, const int64_t* __restrict__ off,
                                                              const int* __restrict__ n_runs, int n_lists,
                                                              const stm_data_mask_desc* __restrict__ desc, int64_t total,
                                                              unsigned char* __restrict__ out, int h, int w, int Hp, int Wp)
{
    const int64_t i = blockIdx.x;
    const int y_begin = blockIdx.y * TD_MASK_ROWS;
    const int x4 = (blockIdx.z * STM_WAVE + threadIdx.x) * TD_LANE_PX;
    if (x4 >= Wp) return;
    const stm_data_mask_desc d = desc[i];
    const bool listed = d.list >= 0 && d.list < n_lists;
    const int m = listed ? d.list : 0;                           // the run list this mask is drawn from
    int64_t c0, c1;
    stm_slot(off, m, total, c0, c1);
    const int nr = listed ? (int)min((int64_t)max(n_runs[m], 0), min(c1 - c0, (int64_t)INT_MAX)) : 0;
    const bool live = nr > 0 && d.H0 > 0 && d.W0 > 0;
    const unsigned int* __restrict__ st = starts + c0;

    unsigned int kbase[TD_LANE_PX];
    int cur[TD_LANE_PX];
    bool inside[TD_LANE_PX];
#pragma unroll
    for (int c = 0; c < TD_LANE_PX; ++c) {
        const int x = x4 + c;
        inside[c] = live && x < w;
        kbase[c] = inside[c] ? (unsigned int)resize_nearest(d.flip ? w - 1 - x : x, d.W0, w) * (unsigned int)d.H0 : 0u;
        cur[c] = -1;
    }
    const int y_end = min(y_begin + TD_MASK_ROWS, Hp);
    for (int y = y_begin; y < y_end; ++y) {
        unsigned int word = 0;
        if (live && y < h) {
            const unsigned int sy = (unsigned int)resize_nearest(y, d.H0, h);
#pragma unroll
            for (int c = 0; c < TD_LANE_PX; ++c) {
                if (!inside[c]) continue;
                const unsigned int k = kbase[c] + sy;
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
        *reinterpret_cast<unsigned int*>(out + ((size_t)i * Hp + y) * Wp + x4) = word;
    }
}

__global__ __launch_bounds__(TD_THREADS) void data_boxes_kernel(const float* __restrict__ boxes, const stm_data_mask_desc* __restrict__ desc, int n,
                                                                float* __restrict__ out, int h, int w, int Hp, int Wp)
{
    const int i = blockIdx.x * TD_THREADS + threadIdx.x;
    if (i >= n) return;
    const stm_data_mask_desc d = desc[i];
    const float ws = (float)((double)w / (double)d.W0), hs = (float)((double)h / (double)d.H0);
    float x1 = boxes[4 * i] * ws, y1 = boxes[4 * i + 1] * hs, x2 = boxes[4 * i + 2] * ws, y2 = boxes[4 * i + 3] * hs;
    const float wf = (float)w, hf = (float)h;
    if (d.flip) {
        const float f1 = (wf - x2) - 1.0f, f2 = (wf - x1) - 1.0f;
        x1 = f1;
        x2 = f2;
    }
    out[4 * i] = fminf(fmaxf(x1, 0.0f), wf) / (float)Wp;
    out[4 * i + 1] = fminf(fmaxf(y1, 0.0f), hf) / (float)Hp;
    out[4 * i + 2] = fminf(fmaxf(x2, 0.0f), wf) / (float)Wp;
    out[4 * i + 3] = fminf(fmaxf(y2, 0.0f), hf) / (float)Hp;
}

}  // namespace

extern "C" size_t stm_data_struct_bytes(int which)
{
    switch (which) {
        case 0: return sizeof(stm_data_frame_desc);
        case 1: return sizeof(stm_data_mask_desc);
        default: return 0;
    }
}

extern "C" int stm_data_frames_u8_f32(const stm_data_frame_desc* frames, int n, float* out, int h, int w, int Hp, int Wp, const double* mean,
                                      const double* stdv, int to_rgb, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL, "stm_data_frames_u8_f32: bad sizes n=%d dst=%dx%d padded=%dx%d", n, h, w,
                Hp, Wp);
    if (n == 0) return STM_OK;
    STM_REQUIRE(frames && out && mean && stdv, STM_ENULL, "stm_data_frames_u8_f32: frames/out/mean/stdv must be non-NULL");
    for (int i = 0; i < n; ++i) {
        const stm_data_frame_desc& d = frames[i];
        STM_REQUIRE(d.ptr, STM_ENULL, "stm_data_frames_u8_f32: frame %d has a NULL pointer", i);
        STM_REQUIRE(d.H0 > 0 && d.W0 > 0 && d.row_stride_bytes >= 3 * (int64_t)d.W0, STM_EINVAL,
                    "stm_data_frames_u8_f32: frame %d: bad source size %dx%d (row stride %lld bytes)", i, d.H0, d.W0, (long long)d.row_stride_bytes);
    }
    for (int i0 = 0; i0 < n; i0 += TD_FRAMES) {
        const int k = min(TD_FRAMES, n - i0);
        FrameArgs a = {};
        for (int i = 0; i < k; ++i) a.f[i] = frames[i0 + i];
        const dim3 grid(stm_cdiv(Wp, 64), stm_cdiv(Hp, 4), k);
        hipLaunchKernelGGL(data_frames_kernel, grid, dim3(256), 0, stm_hs(stream), a, out + (size_t)i0 * 3 * Hp * Wp, h, w, Hp, Wp, mean[0], mean[1],
                           mean[2], stdv[0], stdv[1], stdv[2], to_rgb ? 1 : 0);
        STM_CHECK_LAUNCH("data_frames_kernel");
    }
    return STM_OK;
}

extern "C" int stm_data_rle_starts(const unsigned int* runs, const int64_t* offsets, const int* n_runs_in, const int* status_in, const int64_t* hw,
                                   int n, int64_t total_runs, unsigned int* starts, int* n_runs, int64_t* area, int* status, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && total_runs >= 0, STM_EINVAL, "stm_data_rle_starts: bad sizes");
    if (n == 0) return STM_OK;
    STM_REQUIRE(offsets && hw && n_runs && area && status && (total_runs == 0 || (runs && starts)), STM_ENULL, "stm_data_rle_starts: NULL argument");
    hipLaunchKernelGGL(data_rle_starts_kernel, dim3(stm_cdiv(n, TD_WAVES)), dim3(TD_THREADS), 0, stm_hs(stream), runs, offsets, n_runs_in, status_in,
                       hw, n, total_runs, starts, n_runs, area, status);
    STM_CHECK_LAUNCH("data_rle_starts_kernel");
    return STM_OK;
}

extern "C" int stm_data_masks_u8(const unsigned int* starts, const int64_t* offsets, const int* n_runs, int n_lists, const stm_data_mask_desc* desc,
                                 int n, int64_t total_runs, unsigned char* out, int h, int w, int Hp, int Wp, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && n_lists >= 1 && total_runs >= 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL,
                "stm_data_masks_u8: bad sizes n=%d dst=%dx%d padded=%dx%d", n, h, w, Hp, Wp);
    STM_REQUIRE(Wp % TD_LANE_PX == 0, STM_EINVAL, "stm_data_masks_u8: the padded width %d must be a multiple of %d", Wp, TD_LANE_PX);
    if (n == 0) return STM_OK;
    STM_REQUIRE(offsets && n_runs && desc && out && (total_runs == 0 || starts), STM_ENULL, "stm_data_masks_u8: NULL argument");
    STM_REQUIRE((uintptr_t)out % 4 == 0, STM_EINVAL, "stm_data_masks_u8: out must be 4-byte aligned");
    const int bands = stm_cdiv(Hp, TD_MASK_ROWS), chunks = stm_cdiv(Wp, STM_WAVE * TD_LANE_PX);
    STM_REQUIRE(bands <= 65535 && chunks <= 65535, STM_EINVAL, "stm_data_masks_u8: output %dx%d too large", Hp, Wp);
    hipLaunchKernelGGL(data_masks_kernel, dim3(n, bands, chunks), dim3(STM_WAVE), 0, stm_hs(stream), starts, offsets, n_runs, n_lists, desc, total_runs, out,
                       h, w, Hp, Wp);
    STM_CHECK_LAUNCH("data_masks_kernel");
    return STM_OK;
}

extern "C" int stm_data_boxes_f32(const float* boxes, const stm_data_mask_desc* desc, int n, float* out, int h, int w, int Hp, int Wp,
                                  stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && h > 0 && w > 0 && Hp >= h && Wp >= w, STM_EINVAL, "stm_data_boxes_f32: bad sizes n=%d dst=%dx%d padded=%dx%d", n, h, w, Hp,
                Wp);
    if (n == 0) return STM_OK;
    STM_REQUIRE(boxes && desc && out, STM_ENULL, "stm_data_boxes_f32: NULL argument");
    hipLaunchKernelGGL(data_boxes_kernel, dim3(stm_cdiv(n, TD_THREADS)), dim3(TD_THREADS), 0, stm_hs(stream), boxes, desc, n, out, h, w, Hp, Wp);
    STM_CHECK_LAUNCH("data_boxes_kernel");
    return STM_OK;
}
