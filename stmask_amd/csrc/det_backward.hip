// det_backward.hip -- the deterministic mode of the training backward for gfx950 (MI355X): det_backward.h.
//
//   stm_deform_col2im_det_f32       grad_x of the deformable im2col: the terms of stm_deform_col2im_f32 (deform_backward.hip), summed in 64-bit fixed point
//   stm_roi_align_backward_det_f32  grad_feat of RoIAlign: the terms of stm_roi_align_backward_f32 (temporal_backward.hip), likewise
//   stm_upsample_bilinear_backward_f32  the adjoint of torch's bilinear upsampling as a gather (torch's own is an atomic scatter)
//   stm_det_exponent                the exponent rule of det_accum.h on the host
// The sample position, the validity rule, the corner weights and the in-kernel sigmoid of a logit mask are those of the kernels these stand beside,
// expression for expression: what differs is the addition.  Vector code only; the one atomic is a 64-bit integer add on global memory.
#include "det_accum.h"
#include "det_backward.h"
#include "stm_common.h"

namespace {

constexpr unsigned ONE_BITS = 0x3F800000u;   // 1.0f: the second maximum when no explicit mask scales the terms

// ---------------------------------------------------------------------------------------------- pass 1: maxima as bit patterns
// max over i < n of the bits of |v[(i / inner) * bstride + i % inner]| into *word (cleared before).  The bit patterns of non-negative floats order as
// the floats do, inf above every finite value and NaN above inf, so one integer maximum also says whether anything was not finite.
__global__ __launch_bounds__(256) void det_absmax_kernel(const float* __restrict__ v, int64_t n, int64_t inner, int64_t bstride,
                                                         unsigned* __restrict__ word)
{
    unsigned m = 0;
    const int64_t step = (int64_t)gridDim.x * 256;
    if (inner == bstride) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) m = max(m, __float_as_uint(fabsf(v[i])));
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
            const int64_t b = i / inner;
            m = max(m, __float_as_uint(fabsf(v[b * bstride + (i - b * inner)])));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(word, m);
}

int launch_absmax(const float* v, int64_t n, int64_t inner, int64_t bstride, unsigned* word, stm_stream_t stream)
{
    const int blocks = (int)(n < (int64_t)2048 * 2048 ? (n + 2047) / 2048 : 2048);     // ~8 elements a thread, at most 2048 workgroups
    hipLaunchKernelGGL(det_absmax_kernel, dim3(blocks), dim3(256), 0, stm_hs(stream), v, n, inner, bstride, word);
    STM_CHECK_LAUNCH("det_absmax_kernel");
    return STM_OK;
}

// ---------------------------------------------------------------------------------------------- pass 3: accumulator -> fp32
__global__ __launch_bounds__(256) void det_finish_kernel(const long long* __restrict__ acc, const unsigned* __restrict__ words, int has_b, int q,
                                                         float* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int p;
    const int state = stm_det_state(words[0], has_b ? words[1] : ONE_BITS, q, &p);
    float r = 0.0f;
    if (state == STM_DET_NONFINITE) r = stm_nan_f32();
    else if (state == STM_DET_FINITE) r = (float)((double)acc[i] * stm_det_pow2(-p));     // int64 -> double -> one power-of-two scaling -> fp32
    out[i] = r;
}

int launch_finish(const long long* acc, const unsigned* words, int has_b, int q, float* out, int64_t n, stm_stream_t stream)
{
    hipLaunchKernelGGL(det_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stm_hs(stream), acc, words, has_b, q, out, n);
    STM_CHECK_LAUNCH("det_finish_kernel");
    return STM_OK;
}

int check_workspace(const char* who, const void* ws, size_t ws_bytes, int64_t numel)
{
    STM_REQUIRE(numel < ((int64_t)1 << 38), STM_EUNSUPPORTED, "%s: output of %lld elements", who, (long long)numel);
    STM_REQUIRE(ws, STM_EWORKSPACE, "%s: workspace is NULL", who);
    STM_REQUIRE((uintptr_t)ws % 8 == 0, STM_EWORKSPACE, "%s: workspace is not 8-byte aligned", who);
    STM_REQUIRE(ws_bytes >= stm_det_workspace_bytes(numel), STM_EWORKSPACE, "%s: workspace of %zu bytes < %zu", who, ws_bytes,
                stm_det_workspace_bytes(numel));
    return STM_OK;
}

int shape_bits(const char* who, int64_t terms_bound, int64_t mass_bound, int* q)
{
    *q = stm_det_shape_bits(terms_bound, mass_bound);
    STM_REQUIRE(*q >= STM_DET_MIN_BITS, STM_EUNSUPPORTED, "%s: %lld terms of mass %lld per destination leave %d bits below the maximum, fewer than %d",
                who, (long long)terms_bound, (long long)mass_bound, *q, STM_DET_MIN_BITS);
    return STM_OK;
}

// ---------------------------------------------------------------------------------------------- pass 2: deformable col2im
// Bounds.  A destination (b, c, y, x) receives from a tap (k, position n) through at most one of its four corners (the corners of a sample are four
// different addresses and each is guarded by its own in-range test), so at most K * Ho * Wo terms.  A term is fl(fl(fl(hh * hw) * m) * v) with hh, hw
// in [0, 1], |m| <= b, |v| <= a: at most the maximum's bound each, so the mass, in units of that bound, is K * Ho * Wo as well.
struct DetCol2imArgs {
    const float* gcols;     // [B][C*K][Ho*Wo]
    const float* off;
    const float* mask;
    long long* acc;         // [B][C][H][W]
    const unsigned* words;
    int64_t off_bs, mask_bs;
    int mask_logit, has_b, q;
    int B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo;
};

__device__ __forceinline__ float sigmoid_det_dev(float v) { return 1.0f / (1.0f + expf(-v)); }   // = deform_backward.hip's sigmoid_bwd_dev

// grid: x = ceil(HWo/256), y = dg * chunks_per_group * K, z = B  (stm_deform_col2im_f32's)
__global__ __launch_bounds__(256) void deform_col2im_det_kernel(DetCol2imArgs a, int cpb, int chunks_per_group)
{
    int p;
    if (stm_det_state(a.words[0], a.has_b ? a.words[1] : ONE_BITS, a.q, &p) != STM_DET_FINITE) return;     // uniform: zeros or NaN are pass 3's
    const double two_p = stm_det_pow2(p);
    const int K = a.kh * a.kw;
    const int HWo = a.Ho * a.Wo;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= HWo) return;
    int by = blockIdx.y;
    const int k = by % K;
    by /= K;
    const int chunk = by % chunks_per_group;
    const int g = by / chunks_per_group;
    const int b = blockIdx.z;
    const int Cg = a.C / a.dg;
    const int c0 = g * Cg + chunk * cpb;
    const int c1 = min(g * Cg + Cg, c0 + cpb);
    if (c0 >= c1) return;

    const int ho = n / a.Wo, wo = n - ho * a.Wo;
    const int i = k / a.kw, j = k - i * a.kw;
    const float* ob = a.off + (int64_t)b * a.off_bs + (int64_t)g * 2 * K * HWo;
    const float dy = ob[(int64_t)(2 * k) * HWo + n];
    const float dx = ob[(int64_t)(2 * k + 1) * HWo + n];
    float m = 1.0f;
    if (a.mask) {
        m = a.mask[(int64_t)b * a.mask_bs + (int64_t)(g * K + k) * HWo + n];
        if (a.mask_logit) m = sigmoid_det_dev(m);
    }
    const float fy = (float)(ho * a.sh - a.ph + i * a.dh) + dy;
    const float fx = (float)(wo * a.sw - a.pw + j * a.dw) + dx;
    if (!(fy > -1.0f && fx > -1.0f && fy < (float)a.H && fx < (float)a.W)) return;
    const float fl_y = floorf(fy), fl_x = floorf(fx);
    const int h_low = (int)fl_y, w_low = (int)fl_x, h_high = h_low + 1, w_high = w_low + 1;
    const float lh = fy - fl_y, lw = fx - fl_x, hh = 1.0f - lh, hw = 1.0f - lw;
    const bool t = h_low >= 0, l = w_low >= 0, bt = h_high <= a.H - 1, r = w_high <= a.W - 1;
    const float w1 = hh * hw * m, w2 = hh * lw * m, w3 = lh * hw * m, w4 = lh * lw * m;
    const int hl = max(h_low, 0), wl = max(w_low, 0), hh_i = min(h_high, a.H - 1), wh_i = min(w_high, a.W - 1);
    const int a1 = hl * a.W + wl, a2 = hl * a.W + wh_i, a3 = hh_i * a.W + wl, a4 = hh_i * a.W + wh_i;

    const int64_t HW = (int64_t)a.H * a.W;
    long long* gxb = a.acc + ((int64_t)b * a.C + c0) * HW;
    const float* gc = a.gcols + (((int64_t)b * a.C + c0) * K + k) * HWo + n;
    for (int c = c0; c < c1; ++c) {
        const float v = *gc;
        if (v != 0.0f) {
            if (t && l) stm_det_add(gxb + a1, w1 * v, two_p);
            if (t && r) stm_det_add(gxb + a2, w2 * v, two_p);
            if (bt && l) stm_det_add(gxb + a3, w3 * v, two_p);
            if (bt && r) stm_det_add(gxb + a4, w4 * v, two_p);
        }
        gxb += HW;
        gc += (int64_t)K * HWo;
    }
}

int check_geom(const stm_deform_geom* g, const char* who)     // deform_backward.hip's, word for word
{
    STM_REQUIRE(g, STM_ENULL, "%s: geometry is NULL", who);
    STM_REQUIRE(g->B > 0 && g->C > 0 && g->H > 0 && g->W > 0, STM_EINVAL, "%s: empty input %dx%dx%dx%d", who, g->B, g->C, g->H, g->W);
    STM_REQUIRE(g->kh > 0 && g->kw > 0 && g->sh > 0 && g->sw > 0 && g->dh > 0 && g->dw > 0 && g->ph >= 0 && g->pw >= 0, STM_EINVAL,
                "%s: bad kernel/stride/pad/dilation", who);
    STM_REQUIRE(g->dg > 0 && g->C % g->dg == 0, STM_EINVAL, "%s: C=%d not divisible by deform groups %d", who, g->C, g->dg);
    const int Ho = (g->H + 2 * g->ph - (g->dh * (g->kh - 1) + 1)) / g->sh + 1;
    const int Wo = (g->W + 2 * g->pw - (g->dw * (g->kw - 1) + 1)) / g->sw + 1;
    STM_REQUIRE(Ho > 0 && Wo > 0 && Ho == g->Ho && Wo == g->Wo, STM_EINVAL, "%s: output size %dx%d does not match conv arithmetic %dx%d", who,
                g->Ho, g->Wo, Ho, Wo);
    STM_REQUIRE(g->dg * g->kh * g->kw <= 65535 && g->B <= 65535, STM_EUNSUPPORTED, "%s: dg*K or B above 65535", who);
    STM_REQUIRE((int64_t)g->H * g->W < ((int64_t)1 << 31) && (int64_t)g->Ho * g->Wo < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: map too large", who);
    return STM_OK;
}

// ---------------------------------------------------------------------------------------------- pass 2: RoIAlign
// Bounds, with N = n * PH * PW bins that may reach one destination (b, c, y, x) and g = fl(grad / count) the value a bin's samples carry.
// Mass: a sample adds to one destination fl(g * w) for the corner weights w that land on it.  Away from the border that is one corner, w = fl(hy * hx)
// etc. <= 1.  Where a coordinate is clamped to the last row or column, y_low == y_high and ly = 0, hy = 1, so the two corners that share the address
// carry hx and 0 (or 1, 0, 0, 0): their sum is still <= 1.  A bin has `count` samples of |g| <= (|grad| / count)(1 + 2^-24) each, so a bin adds at
// most |grad| (1 + 2^-24) <= a (1 + 2^-24) and the destination receives at most (N + N / 2^24 + 1) a.
// Terms: a destination is reached by samples of y in a closed interval of length 2 ([y - 1, y + 1], the border rows take [-1, 1] and
// [H - 2, H]).  With sampling_ratio s > 0 a bin has s samples per axis.  With s = 0 it has ceil(r) per axis for a bin extent r, at a spacing
// r / ceil(r) > 1/2 when r > 1 (one sample when r <= 1): fewer than 5 in an interval of length 2, 5 with the rounding of the positions.  Every
// sample makes 4 adds, so terms <= 4 * s^2 * N for s > 0 and 100 * N for s = 0; zero products are not added but are counted.
__device__ __forceinline__ void roi_scatter_det(long long* __restrict__ im, int H, int W, float y, float x, float gw, double two_p)
{
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return;
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
    if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
    const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
    stm_det_add(im + y_low * W + x_low, gw * (hy * hx), two_p);
    stm_det_add(im + y_low * W + x_high, gw * (hy * lx), two_p);
    stm_det_add(im + y_high * W + x_low, gw * (ly * hx), two_p);
    stm_det_add(im + y_high * W + x_high, gw * (ly * lx), two_p);
}

// one thread per grad_out element, stm_roi_align_backward_f32's (px, py, c, roi) order
__global__ __launch_bounds__(256) void roi_align_backward_det_kernel(const float* __restrict__ gout, const float* __restrict__ rois,
                                                                     long long* __restrict__ acc, const unsigned* __restrict__ words, int q, int B,
                                                                     int C, int H, int W, int n, int PH, int PW, float scale, int sampling_ratio,
                                                                     int aligned)
{
    int p;
    if (stm_det_state(words[0], ONE_BITS, q, &p) != STM_DET_FINITE) return;
    const double two_p = stm_det_pow2(p);
    const int64_t total = (int64_t)n * C * PH * PW;
    const int64_t blk = stm_xcd_block((total + 255) / 256);
    if (blk < 0) return;
    const int64_t t = blk * 256 + threadIdx.x;
    if (t >= total) return;
    const float gv = gout[t];
    if (gv == 0.0f) return;
    const int px = t % PW;
    int64_t r = t / PW;
    const int py = r % PH; r /= PH;
    const int c = r % C;
    const int ri = (int)(r / C);
    const float* roi = rois + 5 * (int64_t)ri;
    const float bf = roi[0];
    if (!(bf >= 0.0f && bf < (float)B)) return;     // a batch index outside the map has nothing to scatter to
    const int b = (int)bf;
    const float offset = aligned ? 0.5f : 0.0f;
    const float sw_ = roi[1] * scale - offset, sh_ = roi[2] * scale - offset;
    const float ew_ = roi[3] * scale - offset, eh_ = roi[4] * scale - offset;
    float rw = ew_ - sw_, rh = eh_ - sh_;
    if (!aligned) { rw = fmaxf(rw, 1.0f); rh = fmaxf(rh, 1.0f); }
    const float bh = rh / (float)PH, bw = rw / (float)PW;
    const int gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)PH);
    const int gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)PW);
    const float count = (float)max(gh * gw, 1);
    const float g = gv / count;
    long long* im = acc + ((int64_t)b * C + c) * H * W;
    for (int iy = 0; iy < gh; ++iy) {
        const float y = sh_ + (float)py * bh + ((float)iy + 0.5f) * bh / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
            const float x = sw_ + (float)px * bw + ((float)ix + 0.5f) * bw / (float)gw;
            roi_scatter_det(im, H, W, y, x, g, two_p);
        }
    }
}

// ---------------------------------------------------------------------------------------------- bilinear upsampling, adjoint
constexpr int UP_MAX_SIZE = 1 << 20;

// outputs o of an axis that may read input i: those whose source index lies in [i - 1, i + 1), i.e. o + 0.5 in [(i - 0.5) / scale, (i + 1.5) / scale).
// Estimated in fp32 with a margin of one output each side (the estimate is off by less than 1/8 for sizes up to 2^20); the tap test decides.
__device__ __forceinline__ void up_candidates(int i, float scale, int out, int& lo, int& hi)
{
    const float lf = fmaxf(floorf(((float)i - 0.5f) / scale - 0.5f) - 1.0f, 0.0f);
    const float hf = fminf(ceilf(((float)i + 1.5f) / scale - 0.5f) + 1.0f, (float)(out - 1));
    lo = (int)lf;
    hi = lf <= hf ? (int)hf : lo - 1;
}

// weight of output o on input i, and whether o reads i at all
__device__ __forceinline__ bool up_weight(int o, float scale, int in, int i, float& w)
{
    int i0, i1;
    float l, h;
    stm_bilinear_tap(o, scale, in, i0, i1, l, h);
    w = (i0 == i ? h : 0.0f) + (i1 == i ? l : 0.0f);
    return i0 == i || i1 == i;
}

__global__ __launch_bounds__(256) void upsample_bilinear_backward_kernel(const float* __restrict__ gout, float* __restrict__ gin, int64_t total,
                                                                         int h_in, int w_in, int h_out, int w_out, float scale_h, float scale_w)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int xi = (int)(t % w_in);
    const int64_t r = t / w_in;
    const int yi = (int)(r % h_in);
    const int64_t plane = r / h_in;
    int oy0, oy1, ox0, ox1;
    up_candidates(yi, scale_h, h_out, oy0, oy1);
    up_candidates(xi, scale_w, w_out, ox0, ox1);
    const float* gp = gout + plane * ((int64_t)h_out * w_out);
    float acc = 0.0f;
    for (int oy = oy0; oy <= oy1; ++oy) {
        float wy;
        if (!up_weight(oy, scale_h, h_in, yi, wy)) continue;
        const float* row = gp + (int64_t)oy * w_out;
        float s = 0.0f;
        for (int ox = ox0; ox <= ox1; ++ox) {
            float wx;
            if (up_weight(ox, scale_w, w_in, xi, wx)) s = s + wx * row[ox];
        }
        acc = acc + wy * s;
    }
    gin[t] = acc;
}

}  // namespace

extern "C" int stm_det_exponent(int bits_a, int bits_b, int64_t terms_bound, int64_t mass_bound, int* p, int* state, int* q)
{
    STM_REQUIRE(p && state && q, STM_ENULL, "stm_det_exponent: p/state/q must be non-NULL");
    STM_REQUIRE(bits_a >= 0 && bits_b >= 0, STM_EINVAL, "stm_det_exponent: a maximum is taken of absolute values: the sign bit must be clear");
    STM_REQUIRE(terms_bound >= 0 && mass_bound >= 1, STM_EINVAL, "stm_det_exponent: terms_bound %lld < 0 or mass_bound %lld < 1",
                (long long)terms_bound, (long long)mass_bound);
    *p = 0;
    *state = 0;
    int rc = shape_bits("stm_det_exponent", terms_bound, mass_bound, q);
    if (rc) return rc;
    *state = stm_det_state((uint32_t)bits_a, (uint32_t)bits_b, *q, p);
    return STM_OK;
}

extern "C" size_t stm_det_workspace_bytes(int64_t numel) { return numel < 0 ? 0 : 8 * ((size_t)numel + 1); }

extern "C" int stm_deform_col2im_det_f32(const float* grad_cols, const float* offset, int64_t off_bstride, const float* mask, int64_t mask_bstride,
                                         int mask_is_logit, float* grad_x, const stm_deform_geom* g, void* workspace, size_t workspace_bytes,
                                         stm_stream_t stream)
{
    const char* who = "stm_deform_col2im_det_f32";
    int rc = check_geom(g, who);
    if (rc) return rc;
    STM_REQUIRE(grad_cols && offset && grad_x, STM_ENULL, "%s: grad_cols/offset/grad_x must be non-NULL", who);
    const int K = g->kh * g->kw, HWo = g->Ho * g->Wo, Cg = g->C / g->dg;
    STM_REQUIRE(off_bstride >= (int64_t)g->dg * 2 * K * HWo, STM_EINVAL, "%s: offset batch stride %lld < %lld", who, (long long)off_bstride,
                (long long)g->dg * 2 * K * HWo);
    STM_REQUIRE(!mask || mask_bstride >= (int64_t)g->dg * K * HWo, STM_EINVAL, "%s: mask batch stride too small", who);
    const int64_t numel = (int64_t)g->B * g->C * g->H * g->W;
    if ((rc = check_workspace(who, workspace, workspace_bytes, numel))) return rc;
    int q;
    if ((rc = shape_bits(who, (int64_t)K * HWo, (int64_t)K * HWo, &q))) return rc;
    // the grid of stm_deform_col2im_f32 (the result does not depend on it)
    int cpb = Cg;
    const int64_t base_blocks = (int64_t)stm_cdiv(HWo, 256) * K * g->dg * g->B;
    while (cpb > 8 && base_blocks * (Cg / cpb) < 2048 && cpb % 2 == 0) cpb /= 2;
    const int chunks = stm_cdiv(Cg, cpb);
    STM_REQUIRE((int64_t)g->dg * chunks * K <= 65535, STM_EUNSUPPORTED, "%s: grid too large", who);

    long long* acc = static_cast<long long*>(workspace);
    unsigned* words = reinterpret_cast<unsigned*>(acc + numel);
    const int has_b = (mask && !mask_is_logit) ? 1 : 0;       // a sigmoid is at most 1; an explicit mask is whatever the caller made it
    STM_REQUIRE(hipMemsetAsync(workspace, 0, stm_det_workspace_bytes(numel), stm_hs(stream)) == hipSuccess, STM_ELAUNCH,
                "%s: cannot clear the workspace", who);
    if ((rc = launch_absmax(grad_cols, (int64_t)g->B * g->C * K * HWo, 1, 1, words, stream))) return rc;
    if (has_b && (rc = launch_absmax(mask, (int64_t)g->B * g->dg * K * HWo, (int64_t)g->dg * K * HWo, mask_bstride, words + 1, stream))) return rc;

    DetCol2imArgs a;
    a.gcols = grad_cols; a.off = offset; a.mask = mask; a.acc = acc; a.words = words;
    a.off_bs = off_bstride; a.mask_bs = mask ? mask_bstride : 0;
    a.mask_logit = mask ? mask_is_logit : 0; a.has_b = has_b; a.q = q;
    a.B = g->B; a.C = g->C; a.H = g->H; a.W = g->W; a.kh = g->kh; a.kw = g->kw; a.sh = g->sh; a.sw = g->sw;
    a.ph = g->ph; a.pw = g->pw; a.dh = g->dh; a.dw = g->dw; a.dg = g->dg; a.Ho = g->Ho; a.Wo = g->Wo;
    dim3 grid(stm_cdiv(HWo, 256), g->dg * chunks * K, g->B);
    hipLaunchKernelGGL(deform_col2im_det_kernel, grid, dim3(256), 0, stm_hs(stream), a, cpb, chunks);
    STM_CHECK_LAUNCH("deform_col2im_det_kernel");
    return launch_finish(acc, words, has_b, q, grad_x, numel, stream);
}

extern "C" int stm_roi_align_backward_det_f32(const float* grad_out, const float* rois, float* grad_feat, int B, int C, int H, int W, int n, int PH,
                                              int PW, float spatial_scale, int sampling_ratio, int aligned, void* workspace,
                                              size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_roi_align_backward_det_f32";
    STM_REQUIRE(n >= 0, STM_EINVAL, "%s: n=%d", who, n);
    STM_REQUIRE(grad_feat && (n == 0 || (grad_out && rois)), STM_ENULL, "%s: grad_out/rois/grad_feat must be non-NULL", who);
    STM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0 && sampling_ratio >= 0, STM_EINVAL, "%s: bad sizes", who);
    STM_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: map too large", who);
    const int64_t numel = (int64_t)B * C * H * W;
    if (n == 0) {                                           // the output is written, not accumulated: zeros
        STM_REQUIRE(hipMemsetAsync(grad_feat, 0, (size_t)numel * sizeof(float), stm_hs(stream)) == hipSuccess, STM_ELAUNCH,
                    "%s: cannot clear grad_feat", who);
        return STM_OK;
    }
    const int64_t total = (int64_t)n * C * PH * PW;
    STM_REQUIRE(stm_cdiv(total, 256) < ((int64_t)1 << 31) / 8, STM_EUNSUPPORTED, "%s: too many outputs", who);
    int rc = check_workspace(who, workspace, workspace_bytes, numel);
    if (rc) return rc;
    const int64_t bins = (int64_t)n * PH * PW;
    STM_REQUIRE(sampling_ratio <= 4096, STM_EUNSUPPORTED, "%s: sampling_ratio %d above 4096", who, sampling_ratio);
    const int64_t per_axis = sampling_ratio > 0 ? sampling_ratio : 5;
    int q;
    if ((rc = shape_bits(who, 4 * per_axis * per_axis * bins, bins + (bins >> 24) + 1, &q))) return rc;

    long long* acc = static_cast<long long*>(workspace);
    unsigned* words = reinterpret_cast<unsigned*>(acc + numel);
    STM_REQUIRE(hipMemsetAsync(workspace, 0, stm_det_workspace_bytes(numel), stm_hs(stream)) == hipSuccess, STM_ELAUNCH,
                "%s: cannot clear the workspace", who);
    if ((rc = launch_absmax(grad_out, total, 1, 1, words, stream))) return rc;
    hipLaunchKernelGGL(roi_align_backward_det_kernel, dim3(stm_xcd_grid(stm_cdiv(total, 256))), dim3(256), 0, stm_hs(stream), grad_out, rois, acc,
                       words, q, B, C, H, W, n, PH, PW, spatial_scale, sampling_ratio, aligned);
    STM_CHECK_LAUNCH("roi_align_backward_det_kernel");
    return launch_finish(acc, words, 0, q, grad_feat, numel, stream);
}

extern "C" int stm_upsample_bilinear_backward_f32(const float* grad_out, float* grad_in, int64_t planes, int h_in, int w_in, int h_out, int w_out,
                                                  double scale_factor_h, double scale_factor_w, stm_stream_t stream)
{
    const char* who = "stm_upsample_bilinear_backward_f32";
    STM_REQUIRE(planes >= 0 && h_in > 0 && w_in > 0 && h_out > 0 && w_out > 0, STM_EINVAL, "%s: bad sizes", who);
    STM_REQUIRE(scale_factor_h >= 0.0 && scale_factor_w >= 0.0 && scale_factor_h < 1e300 && scale_factor_w < 1e300, STM_EINVAL,
                "%s: a scale factor is negative or not finite", who);
    if (planes == 0) return STM_OK;
    STM_REQUIRE(grad_out && grad_in, STM_ENULL, "%s: grad_out/grad_in must be non-NULL", who);
    STM_REQUIRE(h_in <= UP_MAX_SIZE && w_in <= UP_MAX_SIZE && h_out <= UP_MAX_SIZE && w_out <= UP_MAX_SIZE, STM_EUNSUPPORTED,
                "%s: an axis above %d elements", who, UP_MAX_SIZE);
    const float scale_h = scale_factor_h > 0.0 ? (float)(1.0 / scale_factor_h) : (float)h_in / (float)h_out;
    const float scale_w = scale_factor_w > 0.0 ? (float)(1.0 / scale_factor_w) : (float)w_in / (float)w_out;
    STM_REQUIRE(scale_h > 0.0f && scale_w > 0.0f && scale_h <= (float)UP_MAX_SIZE && scale_w <= (float)UP_MAX_SIZE, STM_EUNSUPPORTED,
                "%s: scale %g x %g outside (0, 2^20]", who, (double)scale_h, (double)scale_w);
    const int64_t total = planes * h_in * w_in;
    STM_REQUIRE(planes <= ((int64_t)1 << 40) / ((int64_t)h_in * w_in) && (total + 255) / 256 < ((int64_t)1 << 31), STM_EUNSUPPORTED,
                "%s: too many elements", who);
    hipLaunchKernelGGL(upsample_bilinear_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stm_hs(stream), grad_out, grad_in, total,
                       h_in, w_in, h_out, w_out, scale_h, scale_w);
    STM_CHECK_LAUNCH("upsample_bilinear_backward_kernel");
    return STM_OK;
}
