// display.hip -- display mode (reference eval.py:143-318 prep_display, masks and box outlines): tracked instances drawn onto their
// frames.  The reference builds the overlay with broadcast torch arithmetic over an [n, H, W, 3] fp32 tensor per frame (221 MB of
// temporaries at 720p with 20 instances); here one launch per 64 frames reads the soft masks at prototype resolution and the base
// image, and writes each uint8 output pixel once.
//
//   1. cull_rect_kernel (one workgroup per instance): the bounding rectangle of the instance's texels above kCullThr inside its crop.
//   2. render_kernel (one workgroup per 64 x 16 output tile): the tile's texel window is computed with the sampler's own tap function
//      (monotone in the output index), the instances whose rectangle meets it are compacted into LDS in row order, and each lane
//      composites 4 consecutive pixels of one row over that list, then paints the box outlines and stores 12 bytes.
//
// Compositing reproduces prep_display's fp32 operation order, compiled with -ffp-contract=off:
//   inv_j = m_j * (-a) + 1,  mc_j = (m_j * c_j) * a,  P = prod_j inv_j (sequential),  cp = cumprod(inv[:n-1]),
//   T = sum_{j>=1} mc_j * cp_{j-1},  S = mc_0 + T,  out = img * P + S,  byte = (uint8)(out * 255) truncated.
// T is grouped as ATen's CPU sum over dim 0 groups it (cascade_sum, SumKernel.cpp multi_row_sum): terms k = j - 1 in blocks of 16; each
// full block is summed from zero and added to a running block total in order; the terms after the last full block are summed on their
// own and added to that total last.  With m_j in {0, 1} an uncovered row contributes inv = 1 and a +0 term, so skipping it (culling)
// changes no bit; a row's block is set by its index, not by how many rows cover the pixel.
#include "stm_common.h"

namespace {

constexpr int kRenderFrames = 64;
constexpr int kNormSets = 4;           // distinct (mean, stdv) sets of base_fmt 1 frames per launch
constexpr int kTileW = 64, kTileH = 16, kPx = 4;
// Texels at or below 0.5 can still blend to a value a rounding step above 0.5; a rectangle of texels above 0.49 is a safe superset.
constexpr float kCullThr = 0.49f;

// compact per-frame descriptor of the kernel argument (56 bytes: 64 of them and the constants stay under 4 KB)
struct DevFrame {
    const void* base;
    uint8_t* out;
    int base_stride, out_stride;           // bytes (fmt 0) / bytes
    int inst_begin, n_inst;
    unsigned short base_h, base_w, base_ch, base_cw, out_h, out_w, crop_h, crop_w;
    unsigned char fmt, norm, aligned_in, aligned_out, pad[4];
};
static_assert(sizeof(DevFrame) == 56, "DevFrame layout");

struct RenderArgs {
    DevFrame f[kRenderFrames];
    double norm[kNormSets][6];             // mean[3], stdv[3]
};

__global__ __launch_bounds__(256) void cull_rect_kernel(const RenderArgs a, const float* __restrict__ masks, int mh, int mw,
                                                        int4* __restrict__ rects)
{
    __shared__ int r[4];
    const DevFrame& d = a.f[blockIdx.y];
    const int i = blockIdx.x;
    if (i >= d.n_inst) return;
    if (threadIdx.x == 0) { r[0] = 0x7fffffff; r[1] = -1; r[2] = 0x7fffffff; r[3] = -1; }
    __syncthreads();
    const float* m = masks + (int64_t)(d.inst_begin + i) * mh * mw;
    const int ch = d.crop_h, cw = d.crop_w;
    int y_lo = 0x7fffffff, y_hi = -1, x_lo = 0x7fffffff, x_hi = -1;
    for (int t = threadIdx.x; t < ch * cw; t += 256) {
        const int y = t / cw, x = t - y * cw;
        if (m[(int64_t)y * mw + x] > kCullThr) {
            y_lo = min(y_lo, y); y_hi = max(y_hi, y);
            x_lo = min(x_lo, x); x_hi = max(x_hi, x);
        }
    }
    if (y_hi >= 0) {
        atomicMin(&r[0], y_lo); atomicMax(&r[1], y_hi);
        atomicMin(&r[2], x_lo); atomicMax(&r[3], x_hi);
    }
    __syncthreads();
    if (threadIdx.x == 0) rects[d.inst_begin + i] = make_int4(r[0], r[1], r[2], r[3]);
}

// one step of the per-pixel composite for a covering row j (k = j - 1 of the n - 1 summed terms; `full` = 16 * floor((n - 1) / 16))
struct PixelState {
    float P, mc0[3], acc0[3], acc1[3];
    int blk;
};

__device__ __forceinline__ void composite_row(PixelState& s, int j, int full, const float (&mc)[3], float q)
{
    if (j == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s.mc0[c] = mc[c];
    } else {
        const int k = j - 1;
        const int b = k < full ? (k >> 4) : -1;
        if (b != s.blk) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { s.acc1[c] = s.acc1[c] + s.acc0[c]; s.acc0[c] = 0.0f; }
            s.blk = b;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s.acc0[c] = s.acc0[c] + mc[c] * s.P;
    }
    s.P = s.P * q;
}

__global__ __launch_bounds__(256) void render_kernel(const RenderArgs a, const float* __restrict__ masks, int mh, int mw,
                                                     const float* __restrict__ colors, const int* __restrict__ boxes, float alpha,
                                                     const int4* __restrict__ rects)
{
    __shared__ int list[256];
    __shared__ int wave_cnt[4];
    const DevFrame& d = a.f[blockIdx.z];
    const int out_h = d.out_h, out_w = d.out_w;
    const int X0 = blockIdx.x * kTileW, Y0 = blockIdx.y * kTileH;
    if (X0 >= out_w || Y0 >= out_h) return;                       // uniform over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = X0 + (threadIdx.x & 15) * kPx, y = Y0 + (threadIdx.x >> 4);
    const bool row_ok = y < out_h;
    const int n = d.n_inst;
    const int full = n > 1 ? 16 * ((n - 1) / 16) : 0;

    // ---- sampler taps of this lane's row and pixels (mask crop -> output)
    const float sy = (float)d.crop_h / (float)out_h, sx = (float)d.crop_w / (float)out_w;
    int my0, my1, mx0[kPx], mx1[kPx];
    float mly, mhy, mlx[kPx], mhx[kPx];
    stm_bilinear_tap(min(y, out_h - 1), sy, d.crop_h, my0, my1, mly, mhy);
#pragma unroll
    for (int p = 0; p < kPx; ++p) stm_bilinear_tap(min(x + p, out_w - 1), sx, d.crop_w, mx0[p], mx1[p], mlx[p], mhx[p]);

    // ---- texel window of the tile: taps are monotone in the output index
    int ty_lo, ty_hi, tx_lo, tx_hi;
    {
        int i0, i1;
        float l, h;
        stm_bilinear_tap(Y0, sy, d.crop_h, ty_lo, i1, l, h);
        stm_bilinear_tap(min(Y0 + kTileH, out_h) - 1, sy, d.crop_h, i0, ty_hi, l, h);
        stm_bilinear_tap(X0, sx, d.crop_w, tx_lo, i1, l, h);
        stm_bilinear_tap(min(X0 + kTileW, out_w) - 1, sx, d.crop_w, i0, tx_hi, l, h);
    }

    // ---- base image
    float img[kPx][3];
    if (d.fmt == 0) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(d.base) + (int64_t)min(y, out_h - 1) * d.base_stride;
        uint8_t b[kPx * 3];
        if (d.aligned_in && row_ok && x + kPx <= out_w) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + x * 3);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const uint32_t v = s4[w];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[w * 4 + q] = (uint8_t)(v >> (8 * q));
            }
        } else {
#pragma unroll
            for (int p = 0; p < kPx; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) b[p * 3 + c] = (row_ok && x + p < out_w) ? src[(x + p) * 3 + c] : (uint8_t)0;
        }
#pragma unroll
        for (int p = 0; p < kPx; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) img[p][c] = (float)b[p * 3 + c] / 255.0f;
    } else {
        // reference eval.py undo_image_transformation: crop, bilinear resize (fp32), then (v * std + mean) / 255 in double, clip
        const float* src = reinterpret_cast<const float*>(d.base);
        const int64_t plane = (int64_t)d.base_h * d.base_w;
        const double* nm = a.norm[d.norm];
        int by0, by1;
        float bly, bhy;
        stm_bilinear_tap(min(y, out_h - 1), (float)d.base_ch / (float)out_h, d.base_ch, by0, by1, bly, bhy);
#pragma unroll
        for (int p = 0; p < kPx; ++p) {
            int bx0, bx1;
            float blx, bhx;
            stm_bilinear_tap(min(x + p, out_w - 1), (float)d.base_cw / (float)out_w, d.base_cw, bx0, bx1, blx, bhx);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = stm_bilinear_blend(src + c * plane, d.base_w, by0, by1, bx0, bx1, bly, bhy, blx, bhx);
                double e = (double)v * nm[3 + c] + nm[c];
                e = e / 255.0;
                e = e < 0.0 ? 0.0 : (e > 1.0 ? 1.0 : e);
                img[p][c] = (float)e;
            }
        }
    }

    // ---- composite over the rows that can touch the tile, in row order, 256 candidates at a time
    PixelState st[kPx];
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
        st[p].P = 1.0f;
        st[p].blk = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) { st[p].mc0[c] = 0.0f; st[p].acc0[c] = 0.0f; st[p].acc1[c] = 0.0f; }
    }
    const float q = 1.0f + (-alpha);
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int j = c0 + (int)threadIdx.x;
        bool hit = false;
        if (j < n) {
            const int4 r = rects[d.inst_begin + j];
            hit = r.y >= 0 && r.x <= ty_hi && r.y >= ty_lo && r.z <= tx_hi && r.w >= tx_lo;
        }
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int base = 0, cnt = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            base += w < wave ? wave_cnt[w] : 0;
            cnt += wave_cnt[w];
        }
        if (hit) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = j;
        __syncthreads();
        for (int e = 0; e < cnt; ++e) {
            const int jr = list[e];
            const int row = d.inst_begin + jr;
            const float* m = masks + (int64_t)row * mh * mw;
            float mc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) mc[c] = colors[row * 3 + c] * alpha;      // (m * c) * a with m = 1
            if (row_ok) {
#pragma unroll
                for (int p = 0; p < kPx; ++p) {
                    if (x + p < out_w && stm_bilinear_blend(m, mw, my0, my1, mx0[p], mx1[p], mly, mhy, mlx[p], mhx[p]) > 0.5f)
                        composite_row(st[p], jr, full, mc, q);
                }
            }
        }
        __syncthreads();                                           // list / wave_cnt are rewritten by the next chunk
    }

    uint8_t o[kPx * 3];
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
        if (st[p].blk >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { st[p].acc1[c] = st[p].acc1[c] + st[p].acc0[c]; st[p].acc0[c] = 0.0f; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float T = st[p].acc0[c] + st[p].acc1[c];
            const float S = st[p].mc0[c] + T;
            const float v = (img[p][c] * st[p].P + S) * 255.0f;
            o[p * 3 + c] = (uint8_t)(int)v;
        }
    }

    // ---- box outlines: the 3-pixel band centred on each edge, opaque, row 0 on top (first hit in row order wins)
    if (boxes) {
        bool painted[kPx] = {false, false, false, false};
        for (int j = 0; j < n; ++j) {
            const int* bx = boxes + (int64_t)(d.inst_begin + j) * 4;
            const int x1 = min(bx[0], bx[2]), x2 = max(bx[0], bx[2]), y1 = min(bx[1], bx[3]), y2 = max(bx[1], bx[3]);
            if (x1 - 1 > X0 + kTileW - 1 || x2 + 1 < X0 || y1 - 1 > Y0 + kTileH - 1 || y2 + 1 < Y0) continue;   // uniform
            const int row = d.inst_begin + j;
            uint8_t col[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c] = (uint8_t)(int)rintf(colors[row * 3 + c] * 255.0f);
            const bool in_y = y >= y1 - 1 && y <= y2 + 1;
            const bool on_h = abs(y - y1) <= 1 || abs(y - y2) <= 1;
#pragma unroll
            for (int p = 0; p < kPx; ++p) {
                const int xp = x + p;
                const bool on = (in_y && (abs(xp - x1) <= 1 || abs(xp - x2) <= 1)) || (on_h && xp >= x1 - 1 && xp <= x2 + 1);
                if (on && !painted[p]) {
                    painted[p] = true;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[p * 3 + c] = col[c];
                }
            }
        }
    }

    // ---- store: 12 bytes per lane (three dwords) when the rows are 4-byte aligned, else byte by byte
    if (!row_ok) return;
    uint8_t* dst = d.out + (int64_t)y * d.out_stride + x * 3;
    if (d.aligned_out && x + kPx <= out_w) {
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            d4[w] = (uint32_t)o[w * 4] | ((uint32_t)o[w * 4 + 1] << 8) | ((uint32_t)o[w * 4 + 2] << 16) | ((uint32_t)o[w * 4 + 3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < kPx; ++p)
            if (x + p < out_w)
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[p * 3 + c] = o[p * 3 + c];
    }
}

}  // namespace

extern "C" size_t stm_render_workspace_bytes(int n_masks) { return (size_t)(n_masks > 0 ? n_masks : 0) * sizeof(int4) + 256; }

extern "C" int stm_render_overlay_u8(const stm_render_frame* frames, int n_frames, const float* masks, int n_masks, int mh, int mw,
                                     const float* colors, const int* boxes, float alpha, void* workspace, size_t workspace_bytes,
                                     stm_stream_t stream)
{
    STM_REQUIRE(n_frames >= 0 && n_masks >= 0, STM_EINVAL, "stm_render_overlay_u8: negative count (n_frames=%d n_masks=%d)", n_frames, n_masks);
    if (n_frames == 0) return STM_OK;
    STM_REQUIRE(frames, STM_ENULL, "stm_render_overlay_u8: frames must be non-NULL");
    STM_REQUIRE(n_masks == 0 || (masks && colors), STM_ENULL, "stm_render_overlay_u8: masks/colors must be non-NULL");
    STM_REQUIRE(n_masks == 0 || (mh > 0 && mw > 0 && mh <= 32767 && mw <= 32767), STM_EINVAL, "stm_render_overlay_u8: bad mask size %dx%d", mh, mw);
    STM_REQUIRE(alpha == alpha, STM_EINVAL, "stm_render_overlay_u8: alpha is NaN");
    STM_REQUIRE(n_masks == 0 || (workspace && workspace_bytes >= stm_render_workspace_bytes(n_masks)), STM_EWORKSPACE,
                "stm_render_overlay_u8: workspace too small");
    for (int i = 0; i < n_frames; ++i) {
        const stm_render_frame& f = frames[i];
        STM_REQUIRE(f.base && f.out, STM_ENULL, "stm_render_overlay_u8: frame %d has a NULL base or output", i);
        STM_REQUIRE(f.n_inst >= 0 && f.inst_begin >= 0 && (int64_t)f.inst_begin + f.n_inst <= n_masks, STM_EINVAL,
                    "stm_render_overlay_u8: frame %d: rows [%d, %d + %d) outside the %d masks", i, f.inst_begin, f.inst_begin, f.n_inst, n_masks);
        STM_REQUIRE(f.out_h > 0 && f.out_w > 0 && f.out_h <= 32767 && f.out_w <= 32767 && f.out_row_stride >= 3 * (int64_t)f.out_w &&
                    f.out_row_stride < ((int64_t)1 << 31), STM_EINVAL, "stm_render_overlay_u8: frame %d: bad output %dx%d (row stride %lld)", i,
                    f.out_h, f.out_w, (long long)f.out_row_stride);
        STM_REQUIRE(f.n_inst == 0 || (f.crop_h > 0 && f.crop_h <= mh && f.crop_w > 0 && f.crop_w <= mw), STM_EINVAL,
                    "stm_render_overlay_u8: frame %d: mask crop %dx%d outside the %dx%d masks", i, f.crop_h, f.crop_w, mh, mw);
        STM_REQUIRE(f.base_fmt == 0 || f.base_fmt == 1, STM_EINVAL, "stm_render_overlay_u8: frame %d: base_fmt %d not in 0..1", i, f.base_fmt);
        if (f.base_fmt == 0)
            STM_REQUIRE(f.base_h == f.out_h && f.base_w == f.out_w && f.base_row_stride >= 3 * (int64_t)f.base_w &&
                        f.base_row_stride < ((int64_t)1 << 31), STM_EINVAL,
                        "stm_render_overlay_u8: frame %d: uint8 base %dx%d (row stride %lld) must match the %dx%d output", i, f.base_h, f.base_w,
                        (long long)f.base_row_stride, f.out_h, f.out_w);
        else
            STM_REQUIRE(f.base_h > 0 && f.base_w > 0 && f.base_h <= 32767 && f.base_w <= 32767 && f.base_crop_h > 0 && f.base_crop_h <= f.base_h &&
                        f.base_crop_w > 0 && f.base_crop_w <= f.base_w, STM_EINVAL,
                        "stm_render_overlay_u8: frame %d: planar base %dx%d, crop %dx%d", i, f.base_h, f.base_w, f.base_crop_h, f.base_crop_w);
    }
    int4* rects = reinterpret_cast<int4*>(workspace);
    int i0 = 0;
    while (i0 < n_frames) {
        RenderArgs a;
        memset(&a, 0, sizeof(a));
        int k = 0, n_norm = 0, max_inst = 0, max_h = 0, max_w = 0;
        for (; k < kRenderFrames && i0 + k < n_frames; ++k) {
            const stm_render_frame& f = frames[i0 + k];
            int norm = 0;
            if (f.base_fmt == 1) {
                double nv[6] = {f.mean[0], f.mean[1], f.mean[2], f.stdv[0], f.stdv[1], f.stdv[2]};
                for (norm = 0; norm < n_norm && memcmp(a.norm[norm], nv, sizeof(nv)) != 0; ++norm) {}
                if (norm == n_norm) {
                    if (n_norm == kNormSets) break;                // a fifth set of constants: next launch
                    memcpy(a.norm[n_norm++], nv, sizeof(nv));
                }
            }
            DevFrame& d = a.f[k];
            d.base = f.base;
            d.out = f.out;
            d.base_stride = (int)f.base_row_stride;
            d.out_stride = (int)f.out_row_stride;
            d.inst_begin = f.inst_begin;
            d.n_inst = f.n_inst;
            d.base_h = (unsigned short)f.base_h; d.base_w = (unsigned short)f.base_w;
            d.base_ch = (unsigned short)f.base_crop_h; d.base_cw = (unsigned short)f.base_crop_w;
            d.out_h = (unsigned short)f.out_h; d.out_w = (unsigned short)f.out_w;
            d.crop_h = (unsigned short)(f.n_inst ? f.crop_h : 1); d.crop_w = (unsigned short)(f.n_inst ? f.crop_w : 1);
            d.fmt = (unsigned char)f.base_fmt;
            d.norm = (unsigned char)norm;
            d.aligned_in = f.base_fmt == 0 && ((uintptr_t)f.base & 3) == 0 && (f.base_row_stride & 3) == 0;
            d.aligned_out = ((uintptr_t)f.out & 3) == 0 && (f.out_row_stride & 3) == 0;
            max_inst = max(max_inst, f.n_inst);
            max_h = max(max_h, f.out_h);
            max_w = max(max_w, f.out_w);
        }
        if (max_inst > 0) {
            hipLaunchKernelGGL(cull_rect_kernel, dim3(max_inst, k), dim3(256), 0, stm_hs(stream), a, masks, mh, mw, rects);
            STM_CHECK_LAUNCH("cull_rect_kernel");
        }
        hipLaunchKernelGGL(render_kernel, dim3(stm_cdiv(max_w, kTileW), stm_cdiv(max_h, kTileH), k), dim3(256), 0, stm_hs(stream), a, masks,
                           mh, mw, colors, boxes, alpha, rects);
        STM_CHECK_LAUNCH("render_kernel");
        i0 += k;
    }
    return STM_OK;
}
