// temporal_backward.hip -- backward of the RoIAlign and spatial-correlation drop-ins for gfx950 (MI355X).
//
//   stm_roi_align_backward_f32  grad_feat of mmcv 1.x roi_align (avg): every sample of a bin scatters grad / count times its 4 bilinear weights on
//                               the clamped coordinate (samples outside [-1, H] x [-1, W] contribute nothing) -- fp32 atomic adds.  The sample
//                               positions are computed with the forward's expressions (temporal.hip roi_align_avg_kernel).  No gradient w.r.t. rois.
//   stm_corr_backward_f32       grad_in1 / grad_in2 of spatial_correlation_sample(kernel_size=1, patch_size=P, dilation_patch=d): two gathers, one
//                               fixed-order sum per output (run-to-run identical).  A workgroup owns one row y and 64 columns of one image: the
//                               P*P rows of grad_out it needs are staged once into LDS and shared by all channels of the workgroup.
#include "stm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ RoIAlign
__device__ __forceinline__ void roi_scatter(float* __restrict__ im, int H, int W, float y, float x, float gw)
{
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return;
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
    if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
    const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
    unsafeAtomicAdd(im + y_low * W + x_low, gw * (hy * hx));
    unsafeAtomicAdd(im + y_low * W + x_high, gw * (hy * lx));
    unsafeAtomicAdd(im + y_high * W + x_low, gw * (ly * hx));
    unsafeAtomicAdd(im + y_high * W + x_high, gw * (ly * lx));
}

// one thread per grad_out element, the forward's (px, py, c, roi) order
__global__ __launch_bounds__(256) void roi_align_backward_kernel(const float* __restrict__ gout, const float* __restrict__ rois,
                                                                 float* __restrict__ gfeat, int B, int C, int H, int W, int n, int PH, int PW,
                                                                 float scale, int sampling_ratio, int aligned)
{
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
    float* im = gfeat + ((int64_t)b * C + c) * H * W;
    for (int iy = 0; iy < gh; ++iy) {
        const float y = sh_ + (float)py * bh + ((float)iy + 0.5f) * bh / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
            const float x = sw_ + (float)px * bw + ((float)ix + 0.5f) * bw / (float)gw;
            roi_scatter(im, H, W, y, x, g);
        }
    }
}

// ------------------------------------------------------------------------------------------------ correlation
// grad_out g [B][P][P][H][W]; displacement (i, j) -> (dy, dx) = ((i - P/2) * dil, (j - P/2) * dil).
//   MODE 0: grad_in1[c, y, x] = sum_{i,j} g[i, j, y, x] * in2[c, y + dy, x + dx]
//   MODE 1: grad_in2[c, y, x] = sum_{i,j} g[i, j, y - dy, x - dx] * in1[c, y - dy, x - dx]
// Workgroup = (image, row y, 64-column tile, channel chunk); 256 threads = 64 columns x 4 channel lanes.  LDS holds the grad_out values of
// the tile for every displacement: MODE 0 the row y, columns [x0, x0 + 64); MODE 1 the rows y - dy, columns [x0 - R, x0 + 64 + R) (zero outside).
// LDS = false reads the same values from global memory (patches too large for the LDS tile).
constexpr int CB_TW = 64;

template <int MODE, bool LDS>
__global__ __launch_bounds__(256) void corr_backward_kernel(const float* __restrict__ gout, const float* __restrict__ src,
                                                            float* __restrict__ dst, int C, int H, int W, int P, int dil, int cch,
                                                            int tiles_x, int chunks)
{
    extern __shared__ float gs[];
    int64_t id = blockIdx.x;
    const int chunk = id % chunks; id /= chunks;
    const int tx = id % tiles_x; id /= tiles_x;
    const int y = id % H;
    const int b = (int)(id / H);
    const int R = (P / 2) * dil;
    const int x0 = tx * CB_TW;
    const int LDW = MODE == 0 ? CB_TW : CB_TW + 2 * R;
    const int PP = P * P;
    const int64_t HW = (int64_t)H * W;
    const float* gb = gout + (int64_t)b * PP * HW;
    if (LDS) {
        for (int e = threadIdx.x; e < PP * LDW; e += 256) {
            const int ij = e / LDW, xx = e - ij * LDW;
            const int i = ij / P;
            const int yy = MODE == 0 ? y : y - (i - P / 2) * dil;
            const int xg = MODE == 0 ? x0 + xx : x0 - R + xx;
            gs[e] = (yy >= 0 && yy < H && xg >= 0 && xg < W) ? gb[(int64_t)ij * HW + (int64_t)yy * W + xg] : 0.0f;
        }
        __syncthreads();
    }
    const int xl = threadIdx.x & (CB_TW - 1);
    const int x = x0 + xl;
    if (x >= W) return;
    const int c0 = chunk * cch, c1 = min(C, c0 + cch);
    for (int c = c0 + (threadIdx.x >> 6); c < c1; c += 4) {
        const float* sc = src + ((int64_t)b * C + c) * HW;
        float acc = 0.0f;
        for (int i = 0; i < P; ++i) {
            const int dy = (i - P / 2) * dil;
            const int ys = MODE == 0 ? y + dy : y - dy;
            if (ys < 0 || ys >= H) continue;
            for (int j = 0; j < P; ++j) {
                const int dx = (j - P / 2) * dil;
                const int xs = MODE == 0 ? x + dx : x - dx;
                if (xs < 0 || xs >= W) continue;
                float gv;
                if (LDS) gv = MODE == 0 ? gs[(i * P + j) * LDW + xl] : gs[(i * P + j) * LDW + xl + R - dx];
                else gv = MODE == 0 ? gb[(int64_t)(i * P + j) * HW + (int64_t)y * W + x] : gb[(int64_t)(i * P + j) * HW + (int64_t)ys * W + xs];
                acc = fmaf(gv, sc[(int64_t)ys * W + xs], acc);
            }
        }
        dst[((int64_t)b * C + c) * HW + (int64_t)y * W + x] = acc;
    }
}

template <int MODE>
int corr_backward_launch(const float* gout, const float* src, float* dst, int B, int C, int H, int W, int P, int dil, stm_stream_t stream)
{
    const int R = (P / 2) * dil;
    const int tiles_x = stm_cdiv(W, CB_TW);
    const int64_t rows = (int64_t)B * H * tiles_x;
    int cch = 32;
    while (cch > 4 && rows * stm_cdiv(C, cch) < 2048) cch /= 2;
    const int chunks = stm_cdiv(C, cch);
    const size_t lds = (size_t)P * P * (MODE == 0 ? CB_TW : CB_TW + 2 * R) * sizeof(float);
    STM_REQUIRE(rows * chunks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "stm_corr_backward_f32: grid too large");
    const dim3 grid((unsigned)(rows * chunks));
    if (lds <= 64 * 1024) {
        hipLaunchKernelGGL((corr_backward_kernel<MODE, true>), grid, dim3(256), lds, stm_hs(stream), gout, src, dst, C, H, W, P, dil, cch, tiles_x,
                           chunks);
    } else {
        hipLaunchKernelGGL((corr_backward_kernel<MODE, false>), grid, dim3(256), 0, stm_hs(stream), gout, src, dst, C, H, W, P, dil, cch, tiles_x,
                           chunks);
    }
    STM_CHECK_LAUNCH("corr_backward_kernel");
    return STM_OK;
}

}  // namespace

extern "C" int stm_roi_align_backward_f32(const float* grad_out, const float* rois, float* grad_feat, int B, int C, int H, int W, int n, int PH,
                                          int PW, float spatial_scale, int sampling_ratio, int aligned, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0, STM_EINVAL, "stm_roi_align_backward_f32: n=%d", n);
    if (n == 0) return STM_OK;
    STM_REQUIRE(grad_out && rois && grad_feat, STM_ENULL, "stm_roi_align_backward_f32: grad_out/rois/grad_feat must be non-NULL");
    STM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0 && sampling_ratio >= 0, STM_EINVAL, "stm_roi_align_backward_f32: bad sizes");
    STM_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), STM_EUNSUPPORTED, "stm_roi_align_backward_f32: map too large");
    const int64_t total = (int64_t)n * C * PH * PW;
    STM_REQUIRE(stm_cdiv(total, 256) < ((int64_t)1 << 31) / 8, STM_EUNSUPPORTED, "stm_roi_align_backward_f32: too many outputs");
    hipLaunchKernelGGL(roi_align_backward_kernel, dim3(stm_xcd_grid(stm_cdiv(total, 256))), dim3(256), 0, stm_hs(stream), grad_out, rois, grad_feat,
                       B, C, H, W, n, PH, PW, spatial_scale, sampling_ratio, aligned);
    STM_CHECK_LAUNCH("roi_align_backward_kernel");
    return STM_OK;
}

extern "C" int stm_corr_backward_f32(const float* grad_out, const float* in1, const float* in2, float* grad_in1, float* grad_in2, int B, int C,
                                     int H, int W, int P, int dil, stm_stream_t stream)
{
    STM_REQUIRE(grad_out && in1 && in2, STM_ENULL, "stm_corr_backward_f32: grad_out/in1/in2 must be non-NULL");
    STM_REQUIRE(grad_in1 || grad_in2, STM_ENULL, "stm_corr_backward_f32: neither grad_in1 nor grad_in2 given");
    STM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, STM_EINVAL, "stm_corr_backward_f32: empty input");
    STM_REQUIRE(P > 0 && (P & 1) && dil > 0, STM_EINVAL, "stm_corr_backward_f32: patch_size must be odd, dilation > 0");
    STM_REQUIRE((int64_t)P * P * H * W < ((int64_t)1 << 31) && (int64_t)C * H * W < ((int64_t)1 << 31), STM_EUNSUPPORTED,
                "stm_corr_backward_f32: tensors too large");
    if (grad_in1) {
        int rc = corr_backward_launch<0>(grad_out, in2, grad_in1, B, C, H, W, P, dil, stream);
        if (rc) return rc;
    }
    if (grad_in2) return corr_backward_launch<1>(grad_out, in1, grad_in2, B, C, H, W, P, dil, stream);
    return STM_OK;
}
