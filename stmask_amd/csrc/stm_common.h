// stm_common.h -- shared helpers for the gfx950 kernels behind include/stmask_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/stmask_hip.h"

#define STM_WAVE 64  // gfx950 wavefront width (hard-coded: warpSize folds to 64, no macro exists)

void stm_set_error(const char* fmt, ...);

#define STM_REQUIRE(cond, code, ...)      \
    do {                                  \
        if (!(cond)) {                    \
            stm_set_error(__VA_ARGS__);   \
            return (code);                \
        }                                 \
    } while (0)

#define STM_CHECK_LAUNCH(name)                                                       \
    do {                                                                             \
        hipError_t e_ = hipGetLastError();                                           \
        if (e_ != hipSuccess) {                                                      \
            stm_set_error("%s: launch failed: %s", (name), hipGetErrorString(e_));   \
            return STM_ELAUNCH;                                                      \
        }                                                                            \
    } while (0)

// A/B switches (STM_* environment variables) are read ONCE per process, at first use -- never per launch.
// stm_debug_reload_tunables() (tests, A/B scripts) bumps the generation so they are read again.
int stm_env_generation();
int stm_env_int_uncached(const char* name, int dflt);
#define STM_ENV_INT(name, dflt)                                                          \
    ([]() -> int {                                                                       \
        static int v_ = 0, gen_ = -1;                                                    \
        const int g_ = stm_env_generation();                                             \
        if (gen_ != g_) { v_ = stm_env_int_uncached((name), (dflt)); gen_ = g_; }        \
        return v_;                                                                       \
    }())

int* stm_internal_range_flag();                 // conv_bf16x.hip: the device flag registered with stm_planar_set_range_flag for the current device (or null)
long long stm_internal_fused_dcn_launches();   // dcn_fused.hip: launches of dcn_fused_kernel (stm_debug_launch_count(1))

const int* stm_internal_take_pixel_gate();      // capi.hip: the gate set by stm_conv_set_pixel_gate for this thread's next convolution launch (cleared)

static inline hipStream_t stm_hs(stm_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline int stm_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

static inline bool stm_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// the quiet NaN a loss and its gradients are set to when a status word is set
__device__ __forceinline__ float stm_nan_f32() { return __int_as_float(0x7FC00000); }

// ---- launch plumbing: what the host keeps per device ---------------------------------------------
constexpr int STM_MAX_DEVICES = 32;

// index of the current device, or -1 (no device, or one past the per-device tables)
static inline int stm_current_device()
{
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < STM_MAX_DEVICES) ? dev : -1;
}

// Dynamic LDS beyond the default limit must be reserved for a kernel before it is launched.  The attribute belongs to the device's
// copy of the function and is sticky, so the largest size reserved so far is remembered per kernel (one instantiation of this
// template each) and device, and the attribute is set only when a launch needs more -- setting it at each launch only costs host
// time.  Relaxed atomics: two host threads racing here both set a size that covers their own launch, and the larger request is
// simply made again by whoever finds the smaller one recorded.  Without a current device nothing is remembered.
template <auto Kernel>
int stm_reserve_lds(size_t bytes, const char* who)
{
    static std::atomic<int> reserved[STM_MAX_DEVICES];
    const int dev = stm_current_device();
    if (dev < 0 || reserved[dev].load(std::memory_order_relaxed) < (int)bytes) {
        STM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess,
                    STM_ELAUNCH, "%s: cannot reserve %zu bytes of LDS", who, bytes);
        if (dev >= 0) reserved[dev].store((int)bytes, std::memory_order_relaxed);
    }
    return STM_OK;
}

// compute units of the current device, looked up once per device (256 when it cannot be asked)
static inline int stm_cu_count()
{
    static std::atomic<int> n_cus[STM_MAX_DEVICES];
    const int dev = stm_current_device();
    int cus = dev >= 0 ? n_cus[dev].load(std::memory_order_relaxed) : 0;
    if (cus <= 0) {
        hipDeviceProp_t prop;
        cus = (dev >= 0 && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        if (dev >= 0) n_cus[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// ---- device helpers -----------------------------------------------------------------------------

// Workgroup ids are dealt round-robin to the 8 XCDs of the chip, each with its own L2.  Kernels whose neighbouring
// workgroups re-read the same lines (gathers, windows, per-image tables) launch 8 * ceil(nblocks / 8) workgroups and map
// id -> (id & 7) * per_xcd + (id >> 3): each XCD then works on a contiguous run of logical blocks and the shared lines are
// fetched through one L2 instead of eight.  Returns -1 for the padding workgroups.
__device__ __forceinline__ int64_t stm_xcd_block(int64_t nblocks)
{
    const int64_t per_xcd = (nblocks + 7) >> 3;
    const int64_t b = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    return b < nblocks ? b : -1;
}
__device__ __forceinline__ int64_t stm_xcd_block_or_plain(int xcd, int64_t nblocks) { return xcd ? stm_xcd_block(nblocks) : (int64_t)blockIdx.x; }
static inline unsigned stm_xcd_grid(int64_t nblocks) { return (unsigned)(8 * ((nblocks + 7) / 8)); }

// Bilinear sampling as ATen's upsample_bilinear2d (align_corners=False) in fp32, operand order as in oracle/stm_oracle.c.  Shared by the
// mask encoder (output.hip) and the display renderer (display.hip): the masks drawn are the masks written to the json, bit for bit.
// stm_bilinear_tap: output index o of a length-`in` axis resized with `scale` = (float)in / (float)out -> taps i0, i1 and weights h, l.
__device__ __forceinline__ void stm_bilinear_tap(int o, float scale, int in, int& i0, int& i1, float& l, float& h)
{
    float f = scale * ((float)o + 0.5f) - 0.5f;
    if (f < 0.0f) f = 0.0f;
    i0 = (int)f;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l = f - (float)i0;
    h = 1.0f - l;
}
__device__ __forceinline__ float stm_bilinear_blend(const float* __restrict__ m, int64_t ld, int y0, int y1, int x0, int x1, float ly, float hy,
                                                    float lx, float hx)
{
    return hy * (hx * m[y0 * ld + x0] + lx * m[y0 * ld + x1]) + ly * (hx * m[y1 * ld + x0] + lx * m[y1 * ld + x1]);
}

// Canonical exp (oracle/stm_oracle.c: stm_exp_f64): identical IEEE operation sequence in double, rounded
// once to fp32.  Compiled with -ffp-contract=off; every fused step is an explicit fma().
__device__ __forceinline__ double stm_exp_f64(double x)
{
    if (x > 709.0) return __longlong_as_double(0x7FF0000000000000LL);
    if (x < -745.0) return 0.0;
    const double LOG2E = 1.4426950408889634074;
    const double LN2_HI = 6.93147180369123816490e-01;
    const double LN2_LO = 1.90821492927058770002e-10;
    double kf = rint(x * LOG2E);
    double r = fma(-kf, LN2_HI, x);
    r = fma(-kf, LN2_LO, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    int k = (int)kf;
    int k1 = k / 2, k2 = k - k1;
    double s1 = __longlong_as_double((long long)(k1 + 1023) << 52);
    double s2 = __longlong_as_double((long long)(k2 + 1023) << 52);
    return p * s1 * s2;
}

__device__ __forceinline__ float stm_expf_canon(float x) { return (float)stm_exp_f64((double)x); }

// box_utils.py:37-88 in fp32, reference operand order (no contraction: -ffp-contract=off).
__device__ __forceinline__ float stm_iou(const float4 a, const float4 b)
{
    float mx = fminf(a.z, b.z) - fmaxf(a.x, b.x);
    float my = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    mx = mx < 0.0f ? 0.0f : mx;
    my = my < 0.0f ? 0.0f : my;
    float inter = mx * my;
    float area_a = (a.z - a.x) * (a.w - a.y);
    float area_b = (b.z - b.x) * (b.w - b.y);
    float uni = area_a + area_b - inter;
    return inter / uni;
}

// box_utils.py decode (use_yolo_regressors = False) in fp32, reference operand order: cx = p.x + (l.x * 0.1) * p.z, w = p.z * exp(l.z * 0.2),
// x1 = cx - w / 2, x2 = w + x1 (the reference's in-place point-form step: x2 is formed from the UPDATED x1); y alike.
__device__ __forceinline__ float4 stm_decode_one(const float4 l, const float4 p)
{
    const float v0 = 0.1f, v1 = 0.2f;
    float t0 = l.x * v0, t1 = l.y * v0;
    float cx = p.x + t0 * p.z;
    float cy = p.y + t1 * p.w;
    float w = p.z * stm_expf_canon(l.z * v1);
    float h = p.w * stm_expf_canon(l.w * v1);
    float x1 = cx - w / 2.0f;
    float y1 = cy - h / 2.0f;
    return make_float4(x1, y1, w + x1, h + y1);
}

// ... and its adjoint.  x2 = cx + w / 2, so
//     d/dcx = g_x1 + g_x2,   d/dw = (g_x2 - g_x1) / 2     [-1/2 through x1 into both outputs, +1 directly into x2]
//     grad_loc.x = d/dcx * 0.1 * p.z          grad_loc.z = d/dw * w * 0.2
//     grad_priors.x = d/dcx                   grad_priors.z = d/dcx * (l.x * 0.1) + d/dw * exp(l.z * 0.2)
__device__ __forceinline__ void stm_decode_one_adjoint(const float4 gb, const float4 l, const float4 p, float4& grad_loc, float4& grad_priors)
{
    const float v0 = 0.1f, v1 = 0.2f;
    const float gcx = gb.x + gb.z, gcy = gb.y + gb.w;
    const float gw = (gb.z - gb.x) / 2.0f, gh = (gb.w - gb.y) / 2.0f;
    const float ew = stm_expf_canon(l.z * v1), eh = stm_expf_canon(l.w * v1);
    grad_loc = make_float4(gcx * v0 * p.z, gcy * v0 * p.w, gw * (p.z * ew) * v1, gh * (p.w * eh) * v1);
    grad_priors = make_float4(gcx, gcy, gcx * (l.x * v0) + gw * ew, gcy * (l.y * v0) + gh * eh);
}

// Adjoint of stm_iou for one pair.  iou = I / U,  I = mx * my,  mx = max(0, min(a.z, b.z) - max(a.x, b.x)),  U = area_a + area_b - I:
//     dI = g (U + I) / U^2,   d area_a = d area_b = -g I / U^2
// Ties: min(a.z, b.z) and max(a.x, b.x) pass their gradient to a's coordinate when the two are equal; an overlap extent that is not
// strictly positive (the clamp at 0, including exactly 0) passes none.
__device__ __forceinline__ void stm_iou_adjoint(const float4 a, const float4 b, float g, float4& da, float4& db)
{
    const float rx = fminf(a.z, b.z) - fmaxf(a.x, b.x), ry = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    const float mx = rx < 0.0f ? 0.0f : rx, my = ry < 0.0f ? 0.0f : ry;
    const float inter = mx * my;
    const float wa = a.z - a.x, ha = a.w - a.y, wb = b.z - b.x, hb = b.w - b.y;
    const float uni = wa * ha + wb * hb - inter;
    const float gi = g * (uni + inter) / (uni * uni);
    const float ga = -(g * inter) / (uni * uni);          // d area_a = d area_b
    const float gmx = rx > 0.0f ? gi * my : 0.0f, gmy = ry > 0.0f ? gi * mx : 0.0f;
    const bool ax = a.x >= b.x, ay = a.y >= b.y, az = a.z <= b.z, aw = a.w <= b.w;
    da = make_float4((ax ? -gmx : 0.0f) - ga * ha, (ay ? -gmy : 0.0f) - ga * wa, (az ? gmx : 0.0f) + ga * ha, (aw ? gmy : 0.0f) + ga * wa);
    db = make_float4((ax ? 0.0f : -gmx) - ga * hb, (ay ? 0.0f : -gmy) - ga * wb, (az ? 0.0f : gmx) + ga * hb, (aw ? 0.0f : gmy) + ga * wb);
}

// box_utils.py:298-316 (cast=False)
__device__ __forceinline__ void stm_sanitize(float x1, float x2, int size, int padding, float& lo, float& hi)
{
    float a = x1 * (float)size, b = x2 * (float)size;
    float l = fminf(a, b), h = fmaxf(a, b);
    l = l - (float)padding;
    h = h + (float)padding;
    lo = l < 0.0f ? 0.0f : l;
    hi = h > (float)size ? (float)size : h;
}

// box_utils.py:223-233 encode (use_yolo_regressors = False): m point form, p centre-size.  Columns 0-1 in the reference's operand order; the log in
// double, rounded once.  Shared by the target assignment (match.hip) and the temporal-fusion targets (t2s_loss.hip).
__device__ __forceinline__ float4 stm_encode_one(const float4 m, const float4 p)
{
    float4 o;
    o.x = ((m.x + m.z) / 2.0f - p.x) / (0.1f * p.z);
    o.y = ((m.y + m.w) / 2.0f - p.y) / (0.1f * p.w);
    o.z = (float)log((double)((m.z - m.x) / p.z)) / 0.2f;
    o.w = (float)log((double)((m.w - m.y) / p.w)) / 0.2f;
    return o;
}

// bbox_feat_extractor's box -> RoI conversion: sanitize_coordinates_hw(box, fh, fw) with cast=False, padding 0 (box_utils.py:298-337), behind the
// clip index.  Shared by CandidateShift's RoIs (tracker.hip) and the temporal-fusion loss (t2s_loss.hip).
__device__ __forceinline__ void stm_roi_one(const float4 b, float clip, int fh, int fw, float* __restrict__ o)
{
    float x1, x2, y1, y2;
    stm_sanitize(b.x, b.z, fw, 0, x1, x2);
    stm_sanitize(b.y, b.w, fh, 0, y1, y2);
    o[0] = clip;
    o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
}

// Sum over the 16 lanes of a DPP row (lanes 16 q .. 16 q + 15): four data-parallel-primitive moves at VALU speed, every lane of the row ends with the
// row's sum -- quad_perm [1, 0, 3, 2], quad_perm [2, 3, 0, 1], row_half_mirror, row_mirror.  (__shfl_xor goes through ds_bpermute: an LDS round trip
// per step; the tail kernels that fold many small sums spent most of their time there.)  One fixed order: run-to-run identical.
// (The builtins exist only in the device pass; the host pass needs the names.)
__device__ __forceinline__ float stm_row16_sum(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false));
#endif
    return v;
}
__device__ __forceinline__ unsigned stm_row16_sum(unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);
#endif
    return v;
}
// ... and over the whole wave: the four row sums read from lanes 0, 16, 32, 48 and added in that order (wave-uniform result)
__device__ __forceinline__ float stm_wave_sum(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    v = stm_row16_sum(v);
    const int i = __builtin_bit_cast(int, v);
    v = ((__builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16))) +
         __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32))) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
#endif
    return v;
}
__device__ __forceinline__ int stm_wave_sum_rows(unsigned row_sums)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readlane((int)row_sums, 0) + __builtin_amdgcn_readlane((int)row_sums, 16) + __builtin_amdgcn_readlane((int)row_sums, 32) +
           __builtin_amdgcn_readlane((int)row_sums, 48);
#else
    return (int)row_sums;
#endif
}
// the sum of a 64-bit integer over the wave, in every lane
__device__ __forceinline__ long long stm_wave_sum_i64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, STM_WAVE);
    return v;
}
// inclusive prefix sum over the lanes of a wave (wrapping unsigned arithmetic: the sums of a run list that fails its checks are garbage, not undefined)
__device__ __forceinline__ unsigned long long stm_wave_scan_u64(unsigned long long v, int lane)
{
#pragma unroll
    for (int o = 1; o < STM_WAVE; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, STM_WAVE);
        if (lane >= o) v += u;
    }
    return v;
}
// item i's slot [c0, c1) of a buffer of `total` elements, never outside it whatever the offsets hold
__device__ __forceinline__ void stm_slot(const int64_t* off, int64_t i, int64_t total, int64_t& c0, int64_t& c1)
{
    c0 = min(max(off[i], (int64_t)0), total);
    c1 = min(max(off[i + 1], c0), total);
}

// exclusive prefix of v over the 256 threads of a workgroup in thread order, and the total; sw: 4 words of LDS.  Has barriers: call it uniformly.
__device__ __forceinline__ unsigned stm_block_excl_scan(unsigned v, unsigned* sw, unsigned& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                     // sw may still be read from an earlier call
    if (lane == 63) sw[wv] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < wv; ++i) base += sw[i];
    total = sw[0] + sw[1] + sw[2] + sw[3];
    return base + inc - v;
}

// sum of v over the 256 threads of a workgroup in one fixed order (xor butterfly inside a wave, then the waves in order); sd: 4 doubles of LDS
__device__ __forceinline__ double stm_block_sum_f64(double v, double* sd)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sd[0] + sd[1]) + sd[2]) + sd[3];
}
