// mask_loss.hip -- the tail of the reference's lincomb_mask_loss (layers/modules/multibox_loss.py:597-614, and :302-317 of track_to_segment_loss):
// gather one target per instance, bilinear upsampling of the soft masks to the target size, clamp to [0, 1], binary cross entropy per pixel, sum per
// instance -- as one forward and one adjoint kernel for gfx950 that materialise nothing at target resolution.
//
// Table (per axis, fp32, every operation rounded on its own: stm_bilinear_tap, -ffp-contract=off):
//     scale = (float)in / (float)out,  src = max(scale * (dst + 0.5f) - 0.5f, 0),  i0 = (int)src,  i1 = i0 + (i0 < in - 1),  l1 = src - i0,  l0 = 1 - l1
// Forward:   up = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11),  pc = clamp(up, 0, 1),
//            term = -(t max(log pc, -100) + (1 - t) max(log(1 - pc), -100)),  loss[d] = sum of term over all H * W target pixels.
// Adjoint:   grad_pred[d,y,x] = grad_loss[d] * sum over the target pixels that sample (y, x) of weight * dterm,
//            dterm = (pc - t) / max(pc (1 - pc), 1e-12) where 0 <= up <= 1, 0 elsewhere (torch's BCE backward and its inclusive clamp backward).
//
// Forward kernel: a workgroup owns a 16 x 128 target tile of one instance.  The prediction rows and columns the tile samples (at most 18 x 130, since
// h <= H and w <= W) are staged in LDS; a thread owns 4 consecutive columns of 2 rows, so the target bytes come as one dword where the address is
// 4-byte aligned and the dword lies inside the row, and as single bytes elsewhere.  A byte target of 0 or 1 needs one logarithm.  Thread sums, then
// the fixed-order wave sum (stm_wave_sum), then the 4 waves through LDS in wave order: one partial per (instance, tile) in the workspace, which
// mask_bce_reduce_kernel adds per instance (lane l adds tiles l, l + 64, ... in that order, then stm_wave_sum).
// Adjoint kernel: a gather.  One thread owns one prediction pixel; a workgroup an 8 x 32 tile whose values and one-pixel halo sit in LDS.  src is
// monotonic, so the target rows Y with i0(Y) in {y - 1, y} -- the ones that can sample row y -- are one contiguous range; its two ends are found by
// bisection on the table's own i0 (the same stm_bilinear_tap arithmetic as the forward, so both kernels use identical table values).  up is
// recomputed from the LDS tile, and the sum runs over rows, then columns, in ascending order.
// No float atomics anywhere and no host synchronisation: loss and grad_pred are bit-identical from run to run.
// An idx value outside [0, G) is data: the row's workgroups read nothing through it and write NaN.
#include "stm_common.h"

namespace {

constexpr int MF_TH = 16, MF_TW = 128;               // forward: target tile
constexpr int MF_SH = MF_TH + 2, MF_SW = MF_TW + 2;  // ... and the most prediction rows / columns it samples (scale <= 1: i0 moves by at most TH over TH - 1 steps, i1 adds one)
constexpr int MB_TH = 8, MB_TW = 32;                 // adjoint: prediction tile
constexpr int MB_SH = MB_TH + 2, MB_SW = MB_TW + 2;  // ... with its halo
constexpr int MASK_MAX_SIDE = 4096;

__device__ __forceinline__ int tap_i0(int o, float scale)
{
    float f = scale * ((float)o + 0.5f) - 0.5f;      // stm_bilinear_tap's src and i0
    if (f < 0.0f) f = 0.0f;
    return (int)f;
}

// first o in [0, out) with i0(o) >= k (out if none): i0 is non-decreasing in o
__device__ __forceinline__ int tap_lower_bound(int k, float scale, int out)
{
    int lo = 0, hi = out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tap_i0(mid, scale) >= k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ float clamp01(float up) { return up < 0.0f ? 0.0f : (up > 1.0f ? 1.0f : up); }

__device__ __forceinline__ float bce_term(float pc, float t)
{
    return -(t * fmaxf(logf(pc), -100.0f) + (1.0f - t) * fmaxf(logf(1.0f - pc), -100.0f));
}
// t = 0 or 1 exactly: the same value with one logarithm (the other product is 0 * a finite number)
__device__ __forceinline__ float bce_term_bit(float pc, bool t) { return -fmaxf(logf(t ? pc : 1.0f - pc), -100.0f); }


template <bool F32>
__global__ __launch_bounds__(256) void mask_bce_forward_kernel(const float* __restrict__ pred, const void* __restrict__ target,
                                                               const int64_t* __restrict__ idx, float* __restrict__ part, int h, int w, int G, int H,
                                                               int W, int tiles_x, float sy, float sx)
{
    __shared__ float sp[MF_SH * MF_SW];
    __shared__ float wsum[4];
    const int tid = threadIdx.x;
    const int d = blockIdx.y, tile = blockIdx.x;
    float* out = part + (int64_t)d * gridDim.x + tile;
    const int64_t g = idx ? idx[d] : (int64_t)d;
    if (g < 0 || g >= G) {                               // workgroup-uniform
        if (tid == 0) *out = stm_nan_f32();
        return;
    }
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int Y0 = tyi * MF_TH, X0 = txi * MF_TW;
    const int Yl = min(Y0 + MF_TH, H) - 1, Xl = min(X0 + MF_TW, W) - 1;   // the tile's last row and column
    int a0, a1, ys0, xs0;
    float l, hh;
    stm_bilinear_tap(Y0, sy, h, ys0, a1, l, hh);
    stm_bilinear_tap(Yl, sy, h, a0, a1, l, hh);
    const int rows = min(a1 - ys0 + 1, MF_SH);
    stm_bilinear_tap(X0, sx, w, xs0, a1, l, hh);
    stm_bilinear_tap(Xl, sx, w, a0, a1, l, hh);
    const int cols = min(a1 - xs0 + 1, MF_SW);
    const float* pd = pred + (int64_t)d * h * w;
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        sp[r * MF_SW + c] = pd[(int64_t)(ys0 + r) * w + xs0 + c];
    }
    __syncthreads();

    const int tx = tid & 31, ty = tid >> 5;
    const int X = X0 + 4 * tx;
    int c0[4], c1[4];
    float lx[4], hx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c0[j] = c1[j] = 0;
        lx[j] = hx[j] = 0.0f;
        if (X + j < W) {
            stm_bilinear_tap(X + j, sx, w, a0, a1, lx[j], hx[j]);
            c0[j] = min(a0 - xs0, MF_SW - 1);
            c1[j] = min(a1 - xs0, MF_SW - 1);
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < MF_TH / 8; ++k) {
        const int Y = Y0 + ty + 8 * k;
        if (Y >= H || X >= W) continue;
        float ly, hy;
        stm_bilinear_tap(Y, sy, h, a0, a1, ly, hy);
        const float* r0 = sp + min(a0 - ys0, MF_SH - 1) * MF_SW;
        const float* r1 = sp + min(a1 - ys0, MF_SH - 1) * MF_SW;
        const int64_t off = ((int64_t)g * H + Y) * W + X;
        float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        unsigned bits = 0;                               // byte targets: the four bytes
        if (F32) {
            const float* tp = reinterpret_cast<const float*>(target) + off;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (X + j < W) t[j] = tp[j];
        } else {
            const uint8_t* tp = reinterpret_cast<const uint8_t*>(target) + off;
            if (X + 3 < W && ((uintptr_t)tp & 3) == 0) {
                bits = *reinterpret_cast<const uint32_t*>(tp);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (X + j < W) bits |= (unsigned)tp[j] << (8 * j);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (X + j >= W) continue;
            const float up = hy * (hx[j] * r0[c0[j]] + lx[j] * r0[c1[j]]) + ly * (hx[j] * r1[c0[j]] + lx[j] * r1[c1[j]]);
            const float pc = clamp01(up);
            float term;
            if (F32) {
                term = bce_term(pc, t[j]);
            } else {
                const unsigned b = (bits >> (8 * j)) & 0xFFu;
                term = b <= 1u ? bce_term_bit(pc, b == 1u) : bce_term(pc, (float)b);
            }
            acc += term;
        }
    }
    acc = stm_wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) *out = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// loss[d] = the instance's tile partials added in one fixed order: one wave per instance
__global__ __launch_bounds__(256) void mask_bce_reduce_kernel(const float* __restrict__ part, float* __restrict__ loss, int n, int tiles)
{
    const int lane = threadIdx.x & 63;
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= n) return;                                  // wave-uniform
    const float* p = part + (int64_t)d * tiles;
    float s = 0.0f;
    for (int t = lane; t < tiles; t += 64) s += p[t];
    s = stm_wave_sum(s);
    if (lane == 0) loss[d] = s;
}

template <bool F32>
__global__ __launch_bounds__(256) void mask_bce_backward_kernel(const float* __restrict__ grad_loss, const float* __restrict__ pred,
                                                                const void* __restrict__ target, const int64_t* __restrict__ idx,
                                                                float* __restrict__ grad_pred, int h, int w, int G, int H, int W, int tiles_x,
                                                                float sy, float sx)
{
    __shared__ float sp[MB_SH * MB_SW];
    const int tid = threadIdx.x;
    const int d = blockIdx.y, tile = blockIdx.x;
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int y0 = tyi * MB_TH, x0 = txi * MB_TW;
    const int y = y0 + (tid >> 5), x = x0 + (tid & 31);
    const bool live = y < h && x < w;
    float* out = grad_pred + ((int64_t)d * h + y) * w + x;
    const int64_t g = idx ? idx[d] : (int64_t)d;
    if (g < 0 || g >= G) {                               // workgroup-uniform
        if (live) *out = stm_nan_f32();
        return;
    }
    const float* pd = pred + (int64_t)d * h * w;
    for (int i = tid; i < MB_SH * MB_SW; i += 256) {
        const int r = i / MB_SW, c = i - r * MB_SW;
        const int yy = y0 - 1 + r, xx = x0 - 1 + c;
        sp[i] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? pd[(int64_t)yy * w + xx] : 0.0f;
    }
    __syncthreads();
    if (!live) return;

    // the target rows with i0 in {y - 1, y} and the columns with i0 in {x - 1, x}: [Ya, Yb) x [Xa, Xb)
    const int Ya = tap_lower_bound(y - 1, sy, H), Yb = tap_lower_bound(y + 1, sy, H);
    const int Xa = tap_lower_bound(x - 1, sx, W), Xb = tap_lower_bound(x + 1, sx, W);
    float acc = 0.0f;
    for (int Y = Ya; Y < Yb; ++Y) {
        int i0, i1;
        float ly, hy;
        stm_bilinear_tap(Y, sy, h, i0, i1, ly, hy);
        const float wy = (i0 == y ? hy : 0.0f) + (i1 == y ? ly : 0.0f);
        const float* r0 = sp + (i0 - y0 + 1) * MB_SW;    // i0 >= y - 1 >= y0 - 1 and i1 <= y + 1 <= y0 + MB_TH: inside the halo
        const float* r1 = sp + (i1 - y0 + 1) * MB_SW;
        const int64_t off = ((int64_t)g * H + Y) * W;
        float racc = 0.0f;
        for (int X = Xa; X < Xb; ++X) {
            int j0, j1;
            float lx, hx;
            stm_bilinear_tap(X, sx, w, j0, j1, lx, hx);
            const float wx = (j0 == x ? hx : 0.0f) + (j1 == x ? lx : 0.0f);
            const int q0 = j0 - x0 + 1, q1 = j1 - x0 + 1;
            const float up = hy * (hx * r0[q0] + lx * r0[q1]) + ly * (hx * r1[q0] + lx * r1[q1]);
            const float t = F32 ? reinterpret_cast<const float*>(target)[off + X] : (float)reinterpret_cast<const uint8_t*>(target)[off + X];
            float dterm = 0.0f;
            if (!(up < 0.0f) && !(up > 1.0f)) dterm = (up - t) / fmaxf(up * (1.0f - up), 1e-12f);
            racc += wx * dterm;
        }
        acc += wy * racc;
    }
    *out = grad_loss[d] * acc;
}

int mask_bce_check(const char* who, int n, int h, int w, int G, int H, int W, const void* idx)
{
    STM_REQUIRE(n >= 0 && G >= 0, STM_EINVAL, "%s: n=%d G=%d", who, n, G);
    STM_REQUIRE(h >= 1 && w >= 1 && h <= H && w <= W && H <= MASK_MAX_SIDE && W <= MASK_MAX_SIDE, STM_EUNSUPPORTED,
                "%s: %dx%d -> %dx%d is not an upsampling to at most %dx%d", who, h, w, H, W, MASK_MAX_SIDE, MASK_MAX_SIDE);
    STM_REQUIRE(n <= 65535, STM_EUNSUPPORTED, "%s: n=%d > 65535", who, n);
    STM_REQUIRE(idx || G == n || n == 0, STM_EINVAL, "%s: without idx row i uses target i, so G (%d) must equal n (%d)", who, G, n);
    return STM_OK;
}

int mask_bce_tiles(int H, int W) { return stm_cdiv(H, MF_TH) * stm_cdiv(W, MF_TW); }

}  // namespace

extern "C" size_t stm_mask_bce_workspace_bytes(int n, int H, int W)
{
    if (n <= 0 || H <= 0 || W <= 0) return 64;
    return (size_t)n * (size_t)mask_bce_tiles(H, W) * sizeof(float) + 64;
}

extern "C" int stm_mask_bce_upsampled_f32(const float* pred, const void* target, int target_is_f32, const int64_t* idx, float* loss, int n, int h,
                                          int w, int G, int H, int W, void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const int rc = mask_bce_check("stm_mask_bce_upsampled_f32", n, h, w, G, H, W, idx);
    if (rc != STM_OK) return rc;
    if (n == 0) return STM_OK;
    STM_REQUIRE(pred && target && loss, STM_ENULL, "stm_mask_bce_upsampled_f32: pred/target/loss must be non-NULL");
    STM_REQUIRE(workspace && workspace_bytes >= stm_mask_bce_workspace_bytes(n, H, W), STM_EWORKSPACE,
                "stm_mask_bce_upsampled_f32: workspace too small");
    STM_REQUIRE((uintptr_t)workspace % 4 == 0 && (!target_is_f32 || (uintptr_t)target % 4 == 0), STM_EINVAL,
                "stm_mask_bce_upsampled_f32: the workspace and an fp32 target must be 4-byte aligned");
    const int tiles_x = stm_cdiv(W, MF_TW), tiles = mask_bce_tiles(H, W);
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    float* part = reinterpret_cast<float*>(workspace);
    hipStream_t st = stm_hs(stream);
    const dim3 grid(tiles, n);
    if (target_is_f32)
        hipLaunchKernelGGL(mask_bce_forward_kernel<true>, grid, dim3(256), 0, st, pred, target, idx, part, h, w, G, H, W, tiles_x, sy, sx);
    else
        hipLaunchKernelGGL(mask_bce_forward_kernel<false>, grid, dim3(256), 0, st, pred, target, idx, part, h, w, G, H, W, tiles_x, sy, sx);
    STM_CHECK_LAUNCH("mask_bce_forward_kernel");
    hipLaunchKernelGGL(mask_bce_reduce_kernel, dim3(stm_cdiv(n, 4)), dim3(256), 0, st, part, loss, n, tiles);
    STM_CHECK_LAUNCH("mask_bce_reduce_kernel");
    return STM_OK;
}

extern "C" int stm_mask_bce_upsampled_backward_f32(const float* grad_loss, const float* pred, const void* target, int target_is_f32,
                                                   const int64_t* idx, float* grad_pred, int n, int h, int w, int G, int H, int W,
                                                   stm_stream_t stream)
{
    const int rc = mask_bce_check("stm_mask_bce_upsampled_backward_f32", n, h, w, G, H, W, idx);
    if (rc != STM_OK) return rc;
    if (n == 0) return STM_OK;
    STM_REQUIRE(grad_loss && pred && target && grad_pred, STM_ENULL,
                "stm_mask_bce_upsampled_backward_f32: grad_loss/pred/target/grad_pred must be non-NULL");
    STM_REQUIRE(!target_is_f32 || (uintptr_t)target % 4 == 0, STM_EINVAL, "stm_mask_bce_upsampled_backward_f32: an fp32 target must be 4-byte aligned");
    const int tiles_x = stm_cdiv(w, MB_TW), tiles = stm_cdiv(h, MB_TH) * tiles_x;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipStream_t st = stm_hs(stream);
    const dim3 grid(tiles, n);
    if (target_is_f32)
        hipLaunchKernelGGL(mask_bce_backward_kernel<true>, grid, dim3(256), 0, st, grad_loss, pred, target, idx, grad_pred, h, w, G, H, W, tiles_x, sy, sx);
    else
        hipLaunchKernelGGL(mask_bce_backward_kernel<false>, grid, dim3(256), 0, st, grad_loss, pred, target, idx, grad_pred, h, w, G, H, W, tiles_x, sy, sx);
    STM_CHECK_LAUNCH("mask_bce_backward_kernel");
    return STM_OK;
}
