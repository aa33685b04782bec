// deform_backward.hip -- backward of the modulated / v1 deformable im2col for gfx950 (MI355X).
//
// The gradients dcn_v2's and mmcv's backward passes produce, for the training path of the drop-in shims (stmask_amd/autograd.py):
//   stm_deform_col2im_f32       grad_x      scattered from grad_cols to the 4 bilinear corners of every tap, times the mask.  Offsets are
//                                           arbitrary, so this is a scatter: fp32 atomic adds (last-bit run-to-run variation; the deterministic
//                                           mode takes stm_deform_col2im_det_f32 of det_backward.hip instead, which has none).
//   stm_deform_col2im_coord_f32 grad_offset / grad_mask: one reduction over the C / dg channels of a deformable group per output, in a fixed
//                                           channel order, no atomics (run-to-run identical).
// The sample position, the validity rule (-1 < h < H, -1 < w < W), the corner weights and the in-kernel sigmoid of a logit mask are the
// forward's (deform_im2col.hip, direct variant), so forward and backward agree on what a sample is.  The coordinate derivative follows
// DCNv2 / mmcv 1.x: h_low = floor(h) also at integer h; 0 outside (-1, H) x (-1, W).
#include "stm_common.h"

namespace {

struct Col2imArgs {
    const float* gcols;     // [B][C*K][Ho*Wo]
    const float* x;         // [B][C][H][W] (coord kernel only)
    const float* off;
    const float* mask;
    float* gx;              // [B][C][H][W], accumulated
    float* goff;
    float* gmask;
    int64_t off_bs, mask_bs, goff_bs, gmask_bs;
    int mask_logit;
    int B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo;
};

__device__ __forceinline__ float sigmoid_bwd_dev(float v) { return 1.0f / (1.0f + expf(-v)); }   // = deform_im2col.hip's sigmoidf_dev

// grid: x = ceil(HWo/256), y = dg * chunks_per_group * K, z = B  (the forward's direct variant)
__global__ __launch_bounds__(256) void deform_col2im_kernel(Col2imArgs a, int cpb, int chunks_per_group)
{
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
        if (a.mask_logit) m = sigmoid_bwd_dev(m);
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
    float* gxb = a.gx + ((int64_t)b * a.C + c0) * HW;
    const float* gc = a.gcols + (((int64_t)b * a.C + c0) * K + k) * HWo + n;
    for (int c = c0; c < c1; ++c) {
        const float v = *gc;
        if (v != 0.0f) {
            if (t && l) unsafeAtomicAdd(gxb + a1, w1 * v);
            if (t && r) unsafeAtomicAdd(gxb + a2, w2 * v);
            if (bt && l) unsafeAtomicAdd(gxb + a3, w3 * v);
            if (bt && r) unsafeAtomicAdd(gxb + a4, w4 * v);
        }
        gxb += HW;
        gc += (int64_t)K * HWo;
    }
}

// grid: x = ceil(HWo/256), y = dg * K, z = B.  One thread per (b, g, k, position): the sums over the group's channels in channel order.
__global__ __launch_bounds__(256) void deform_col2im_coord_kernel(Col2imArgs a)
{
    const int K = a.kh * a.kw;
    const int HWo = a.Ho * a.Wo;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= HWo) return;
    const int k = blockIdx.y % K;
    const int g = blockIdx.y / K;
    const int b = blockIdx.z;
    const int Cg = a.C / a.dg;

    const int ho = n / a.Wo, wo = n - ho * a.Wo;
    const int i = k / a.kw, j = k - i * a.kw;
    const float* ob = a.off + (int64_t)b * a.off_bs + (int64_t)g * 2 * K * HWo;
    const float dy = ob[(int64_t)(2 * k) * HWo + n];
    const float dx = ob[(int64_t)(2 * k + 1) * HWo + n];
    float m = 1.0f, s = 1.0f;
    if (a.mask) {
        m = a.mask[(int64_t)b * a.mask_bs + (int64_t)(g * K + k) * HWo + n];
        if (a.mask_logit) { s = sigmoid_bwd_dev(m); m = s; }
    }
    const float fy = (float)(ho * a.sh - a.ph + i * a.dh) + dy;
    const float fx = (float)(wo * a.sw - a.pw + j * a.dw) + dx;

    float acc_y = 0.0f, acc_x = 0.0f, acc_v = 0.0f;
    if (fy > -1.0f && fx > -1.0f && fy < (float)a.H && fx < (float)a.W) {
        const float fl_y = floorf(fy), fl_x = floorf(fx);
        const int h_low = (int)fl_y, w_low = (int)fl_x, h_high = h_low + 1, w_high = w_low + 1;
        const float lh = fy - fl_y, lw = fx - fl_x, hh = 1.0f - lh, hw = 1.0f - lw;
        const bool t = h_low >= 0, l = w_low >= 0, bt = h_high <= a.H - 1, r = w_high <= a.W - 1;
        const int hl = max(h_low, 0), wl = max(w_low, 0), hh_i = min(h_high, a.H - 1), wh_i = min(w_high, a.W - 1);
        const int a1 = hl * a.W + wl, a2 = hl * a.W + wh_i, a3 = hh_i * a.W + wl, a4 = hh_i * a.W + wh_i;
        const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
        const int64_t HW = (int64_t)a.H * a.W;
        const float* xc = a.x + ((int64_t)b * a.C + (int64_t)g * Cg) * HW;
        const float* gc = a.gcols + (((int64_t)b * a.C + (int64_t)g * Cg) * K + k) * HWo + n;
        for (int c = 0; c < Cg; ++c) {
            const float gv = *gc;
            const float v1 = (t && l) ? xc[a1] : 0.0f;
            const float v2 = (t && r) ? xc[a2] : 0.0f;
            const float v3 = (bt && l) ? xc[a3] : 0.0f;
            const float v4 = (bt && r) ? xc[a4] : 0.0f;
            const float dvdy = hw * (v3 - v1) + lw * (v4 - v2);      // d bilinear / d h, h_low = floor(h)
            const float dvdx = hh * (v2 - v1) + lh * (v4 - v3);      // d bilinear / d w
            const float v = fmaf(w4, v4, fmaf(w3, v3, fmaf(w2, v2, w1 * v1)));
            acc_y = fmaf(gv, dvdy, acc_y);
            acc_x = fmaf(gv, dvdx, acc_x);
            acc_v = fmaf(gv, v, acc_v);
            xc += HW;
            gc += (int64_t)K * HWo;
        }
    }
    if (a.goff) {
        float* go = a.goff + (int64_t)b * a.goff_bs + (int64_t)g * 2 * K * HWo;
        go[(int64_t)(2 * k) * HWo + n] = acc_y * m;
        go[(int64_t)(2 * k + 1) * HWo + n] = acc_x * m;
    }
    if (a.gmask) {
        // d/d logit = d/d m * s * (1 - s) for the forward's s = 1 / (1 + e), e = exp(-logit), evaluated as e / (1 + e)^2: 1 - s in fp32 would cancel
        // for s near 1 (a logit of 10 leaves 1 - s with 3 significant bits)
        float ds = 1.0f;
        if (a.mask_logit) {
            const float e = expf(-a.mask[(int64_t)b * a.mask_bs + (int64_t)(g * K + k) * HWo + n]);
            const float d = 1.0f + e;
            ds = e < 1e18f ? e / (d * d) : 1.0f / e;
        }
        const float gm = a.mask_logit ? acc_v * ds : acc_v;
        a.gmask[(int64_t)b * a.gmask_bs + (int64_t)(g * K + k) * HWo + n] = gm;
    }
}

int check_geom(const stm_deform_geom* g, const char* who)
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

Col2imArgs make_args(const float* gcols, const float* offset, int64_t off_bstride, const float* mask, int64_t mask_bstride, int mask_is_logit,
                     const stm_deform_geom* g)
{
    Col2imArgs a;
    a.gcols = gcols; a.x = nullptr; a.off = offset; a.mask = mask; a.gx = nullptr; a.goff = nullptr; a.gmask = nullptr;
    a.off_bs = off_bstride; a.mask_bs = mask ? mask_bstride : 0; a.goff_bs = 0; a.gmask_bs = 0;
    a.mask_logit = mask ? mask_is_logit : 0;
    a.B = g->B; a.C = g->C; a.H = g->H; a.W = g->W; a.kh = g->kh; a.kw = g->kw; a.sh = g->sh; a.sw = g->sw;
    a.ph = g->ph; a.pw = g->pw; a.dh = g->dh; a.dw = g->dw; a.dg = g->dg; a.Ho = g->Ho; a.Wo = g->Wo;
    return a;
}

}  // namespace

extern "C" int stm_deform_col2im_f32(const float* grad_cols, const float* offset, int64_t off_bstride, const float* mask, int64_t mask_bstride,
                                     int mask_is_logit, float* grad_x, const stm_deform_geom* g, stm_stream_t stream)
{
    int rc = check_geom(g, "stm_deform_col2im_f32");
    if (rc) return rc;
    STM_REQUIRE(grad_cols && offset && grad_x, STM_ENULL, "stm_deform_col2im_f32: grad_cols/offset/grad_x must be non-NULL");
    const int K = g->kh * g->kw, HWo = g->Ho * g->Wo, Cg = g->C / g->dg;
    STM_REQUIRE(off_bstride >= (int64_t)g->dg * 2 * K * HWo, STM_EINVAL, "stm_deform_col2im_f32: offset batch stride %lld < %lld",
                (long long)off_bstride, (long long)g->dg * 2 * K * HWo);
    STM_REQUIRE(!mask || mask_bstride >= (int64_t)g->dg * K * HWo, STM_EINVAL, "stm_deform_col2im_f32: mask batch stride too small");
    Col2imArgs a = make_args(grad_cols, offset, off_bstride, mask, mask_bstride, mask_is_logit, g);
    a.gx = grad_x;
    // channels per thread: the coefficients are computed once per (position, tap); keep >= ~2048 workgroups in flight
    int cpb = Cg;
    const int64_t base_blocks = (int64_t)stm_cdiv(HWo, 256) * K * g->dg * g->B;
    while (cpb > 8 && base_blocks * (Cg / cpb) < 2048 && cpb % 2 == 0) cpb /= 2;
    const int chunks = stm_cdiv(Cg, cpb);
    STM_REQUIRE((int64_t)g->dg * chunks * K <= 65535, STM_EUNSUPPORTED, "stm_deform_col2im_f32: grid too large");
    dim3 grid(stm_cdiv(HWo, 256), g->dg * chunks * K, g->B);
    hipLaunchKernelGGL(deform_col2im_kernel, grid, dim3(256), 0, stm_hs(stream), a, cpb, chunks);
    STM_CHECK_LAUNCH("deform_col2im_kernel");
    return STM_OK;
}

extern "C" int stm_deform_col2im_coord_f32(const float* grad_cols, const float* x, const float* offset, int64_t off_bstride, const float* mask,
                                           int64_t mask_bstride, int mask_is_logit, float* grad_offset, int64_t goff_bstride, float* grad_mask,
                                           int64_t gmask_bstride, const stm_deform_geom* g, stm_stream_t stream)
{
    int rc = check_geom(g, "stm_deform_col2im_coord_f32");
    if (rc) return rc;
    STM_REQUIRE(grad_cols && x && offset, STM_ENULL, "stm_deform_col2im_coord_f32: grad_cols/x/offset must be non-NULL");
    STM_REQUIRE(grad_offset || grad_mask, STM_ENULL, "stm_deform_col2im_coord_f32: neither grad_offset nor grad_mask given");
    STM_REQUIRE(!grad_mask || mask, STM_EINVAL, "stm_deform_col2im_coord_f32: grad_mask needs a mask (v1 has none)");
    const int K = g->kh * g->kw, HWo = g->Ho * g->Wo;
    STM_REQUIRE(off_bstride >= (int64_t)g->dg * 2 * K * HWo && (!grad_offset || goff_bstride >= (int64_t)g->dg * 2 * K * HWo), STM_EINVAL,
                "stm_deform_col2im_coord_f32: offset batch stride below %lld", (long long)g->dg * 2 * K * HWo);
    STM_REQUIRE((!mask || mask_bstride >= (int64_t)g->dg * K * HWo) && (!grad_mask || gmask_bstride >= (int64_t)g->dg * K * HWo), STM_EINVAL,
                "stm_deform_col2im_coord_f32: mask batch stride below %lld", (long long)g->dg * K * HWo);
    Col2imArgs a = make_args(grad_cols, offset, off_bstride, mask, mask_bstride, mask_is_logit, g);
    a.x = x; a.goff = grad_offset; a.gmask = grad_mask; a.goff_bs = grad_offset ? goff_bstride : 0; a.gmask_bs = grad_mask ? gmask_bstride : 0;
    dim3 grid(stm_cdiv(HWo, 256), g->dg * K, g->B);
    hipLaunchKernelGGL(deform_col2im_coord_kernel, grid, dim3(256), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("deform_col2im_coord_kernel");
    return STM_OK;
}
