// t2s_feat.hip -- T2S_concat_feat (reference STMask.py:291-296) and its adjoint for gfx950 (MI355X), include/stmask_hip_t2s_feat.h.
//
// The two frames of a clip lie interleaved in the batch (image 2 b: reference frame, 2 b + 1: next frame); every kernel here reads its half in place
// through the batch stride, so none of the four .contiguous() copies, the cat and the two activations of the torch form is launched.
//
//   stm_t2s_feat_forward_f32   launch 1: the P*P correlation channels.  A workgroup owns (clip, row y, 64 columns, 4 displacement rows); a wave one
//                              displacement row i, a thread one column and the P displacements j of that row in registers.  A chunk of 16 channels of
//                              the 4 next-frame rows y + i - R, columns [x0 - R, x0 + 64 + R), is staged in LDS (zero outside the map) and shared by
//                              the 64 columns; the sum runs in channel order through one fmaf chain, then * 1/C and the clamp at 0.
//                              launch 2: the 2 Cu copied channels, max(0, t2s), a contiguous block per clip.
//   stm_t2s_feat_backward_f32  grad_fpn: the layout of corr_backward_kernel (temporal_backward.hip) -- a workgroup per (clip, row, 64-column tile,
//                              channel chunk), the P*P rows of grad_out for the tile staged in LDS -- with the gate [out > 0] and the 1/C applied
//                              once while staging and the two halves addressed through the batch stride; one launch per half.
//                              grad_t2s: grad_out's two blocks gated by t2s > 0, one launch.
#include "stm_common.h"
#include "../../include/stmask_hip_t2s_feat.h"

namespace {

constexpr int TF_TW = 64;      // columns of a workgroup's tile
constexpr int TF_CC = 16;      // channels staged per pass of the forward
constexpr int TF_ROWS = 4;     // displacement rows of a workgroup (one per wave)

// ------------------------------------------------------------------------------------------------ forward, correlation channels
template <int PT>
__global__ __launch_bounds__(256) void t2s_corr_forward_kernel(const float* __restrict__ fpn, float* __restrict__ out, int C, int H, int W, int Ctot,
                                                               int tiles_x, int igroups, float inv_c)
{
    constexpr int R = PT / 2, LDW = TF_TW + 2 * R;
    __shared__ float ns[TF_CC * TF_ROWS * LDW];
    int64_t id = blockIdx.x;
    const int ig = id % igroups; id /= igroups;
    const int tx = id % tiles_x; id /= tiles_x;
    const int y = id % H;
    const int b = (int)(id / H);
    const int64_t HW = (int64_t)H * W;
    const float* ref = fpn + (int64_t)(2 * b) * C * HW;
    const float* nxt = ref + (int64_t)C * HW;
    const int x0 = tx * TF_TW;
    const int xl = threadIdx.x & (TF_TW - 1), wv = threadIdx.x >> 6;
    const int i = ig * TF_ROWS + wv, x = x0 + xl;
    const bool live = i < PT && x < W;
    float acc[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) acc[j] = 0.0f;
    for (int c0 = 0; c0 < C; c0 += TF_CC) {
        __syncthreads();                                     // the previous chunk has been read
        for (int e = threadIdx.x; e < TF_CC * TF_ROWS * LDW; e += 256) {
            const int cc = e / (TF_ROWS * LDW), rem = e - cc * (TF_ROWS * LDW);
            const int r = rem / LDW, xx = rem - r * LDW;
            const int ii = ig * TF_ROWS + r, yy = y + ii - R, xg = x0 - R + xx, c = c0 + cc;
            ns[e] = (c < C && ii < PT && yy >= 0 && yy < H && xg >= 0 && xg < W) ? nxt[(int64_t)c * HW + (int64_t)yy * W + xg] : 0.0f;
        }
        __syncthreads();
        if (live) {
            const int ncc = min(TF_CC, C - c0);
            for (int cc = 0; cc < ncc; ++cc) {
                const float a = ref[(int64_t)(c0 + cc) * HW + (int64_t)y * W + x];
                const float* row = ns + (cc * TF_ROWS + wv) * LDW + xl;
#pragma unroll
                for (int j = 0; j < PT; ++j) acc[j] = fmaf(a, row[j], acc[j]);
            }
        }
    }
    if (live) {
        float* ob = out + ((int64_t)b * Ctot + (int64_t)i * PT) * HW + (int64_t)y * W + x;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const float v = acc[j] * inv_c;
            ob[(int64_t)j * HW] = v < 0.0f ? 0.0f : v;
        }
    }
}

// any odd P: one thread per output, the same channel-order fmaf chain read from global memory
__global__ __launch_bounds__(256) void t2s_corr_forward_any_kernel(const float* __restrict__ fpn, float* __restrict__ out, int bs, int C, int H, int W,
                                                                   int P, int Ctot, float inv_c)
{
    const int64_t HW = (int64_t)H * W, PP = (int64_t)P * P;
    const int64_t total = (int64_t)bs * PP * HW;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int x = t % W;
    int64_t r = t / W;
    const int y = r % H; r /= H;
    const int ij = r % PP;
    const int b = (int)(r / PP);
    const int i = ij / P, j = ij - i * P, R = P / 2;
    const int yy = y + i - R, xx = x + j - R;
    float acc = 0.0f;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const float* ref = fpn + (int64_t)(2 * b) * C * HW + (int64_t)y * W + x;
        const float* nxt = fpn + (int64_t)(2 * b + 1) * C * HW + (int64_t)yy * W + xx;
        for (int c = 0; c < C; ++c) acc = fmaf(ref[(int64_t)c * HW], nxt[(int64_t)c * HW], acc);
    }
    const float v = acc * inv_c;
    out[((int64_t)b * Ctot + ij) * HW + (int64_t)y * W + x] = v < 0.0f ? 0.0f : v;
}

// ------------------------------------------------------------------------------------------------ the copied channels and their adjoint
// t2s is [2 bs][Cu][HW] contiguous, so clip b's two maps are one run of n_clip = 2 Cu HW floats, and so are their channels of out / grad_out
// (at clip stride Ctot HW, offset P*P HW).  BACK = false: out = max(0, t2s);  BACK = true: grad_t2s = t2s > 0 ? grad_out : 0 (`io` is grad_t2s).
// VEC = 4 needs HW % 4 == 0 and 16-byte aligned pointers.
template <bool BACK, int VEC>
__global__ __launch_bounds__(256) void t2s_copy_kernel(const float* __restrict__ t2s, const float* __restrict__ gout, float* __restrict__ io,
                                                       int64_t n_clip, int64_t clip_stride, int64_t offset, int64_t total)
{
    const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (t >= total) return;
    const int64_t b = t / n_clip;
    const int64_t o = b * clip_stride + offset + (t - b * n_clip);
    if (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(t2s + t);
        if (BACK) {
            const float4 g = *reinterpret_cast<const float4*>(gout + o);
            *reinterpret_cast<float4*>(io + t) = make_float4(v.x > 0.0f ? g.x : 0.0f, v.y > 0.0f ? g.y : 0.0f, v.z > 0.0f ? g.z : 0.0f,
                                                             v.w > 0.0f ? g.w : 0.0f);
        } else {
            *reinterpret_cast<float4*>(io + o) = make_float4(v.x < 0.0f ? 0.0f : v.x, v.y < 0.0f ? 0.0f : v.y, v.z < 0.0f ? 0.0f : v.z,
                                                             v.w < 0.0f ? 0.0f : v.w);
        }
    } else {
        const float v = t2s[t];
        if (BACK) io[t] = v > 0.0f ? gout[o] : 0.0f;
        else io[o] = v < 0.0f ? 0.0f : v;
    }
}

template <bool BACK>
int t2s_copy_launch(const float* t2s, const float* gout, float* io, int bs, int Cu, int64_t HW, int64_t PP, int Ctot, stm_stream_t stream)
{
    const int64_t n_clip = 2 * (int64_t)Cu * HW, total = (int64_t)bs * n_clip;
    const bool vec = HW % 4 == 0 && stm_aligned16(t2s) && stm_aligned16(io) && (!BACK || stm_aligned16(gout));
    const int64_t blocks = (total / (vec ? 4 : 1) + 255) / 256;
    STM_REQUIRE(blocks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "stm_t2s_feat: grid too large");
    if (vec) hipLaunchKernelGGL((t2s_copy_kernel<BACK, 4>), dim3((unsigned)blocks), dim3(256), 0, stm_hs(stream), t2s, gout, io, n_clip,
                                (int64_t)Ctot * HW, PP * HW, total);
    else hipLaunchKernelGGL((t2s_copy_kernel<BACK, 1>), dim3((unsigned)blocks), dim3(256), 0, stm_hs(stream), t2s, gout, io, n_clip,
                            (int64_t)Ctot * HW, PP * HW, total);
    STM_CHECK_LAUNCH("t2s_copy_kernel");
    return STM_OK;
}

// ------------------------------------------------------------------------------------------------ backward, correlation channels
// g~[ij] = grad_out[ij] * [out[ij] > 0] * (1 / C); displacement (i, j) -> (dy, dx) = (i - P/2, j - P/2).
//   MODE 0: grad_fpn[2b][c, y, x]   = sum_{i,j} g~[i, j, y, x] * fpn[2b+1][c, y + dy, x + dx]
//   MODE 1: grad_fpn[2b+1][c, y, x] = sum_{i,j} g~[i, j, y - dy, x - dx] * fpn[2b][c, y - dy, x - dx]
// Workgroup = (clip, row y, 64-column tile, channel chunk); 256 threads = 64 columns x 4 channel lanes.  LDS holds g~ of the tile for every
// displacement: MODE 0 the row y, columns [x0, x0 + 64); MODE 1 the rows y - dy, columns [x0 - R, x0 + 64 + R) (zero outside).
// LDS = false forms the same values from global memory (patches too large for the LDS tile).
__device__ __forceinline__ float t2s_gated(const float* __restrict__ g, const float* __restrict__ o, int64_t idx, float inv_c)
{
    return o[idx] > 0.0f ? g[idx] * inv_c : 0.0f;
}

template <int MODE, bool LDS>
__global__ __launch_bounds__(256) void t2s_corr_backward_kernel(const float* __restrict__ gout, const float* __restrict__ outp,
                                                                const float* __restrict__ fpn, float* __restrict__ gfpn, int C, int H, int W, int P,
                                                                int Ctot, int cch, int tiles_x, int chunks, float inv_c)
{
    extern __shared__ float gs[];
    int64_t id = blockIdx.x;
    const int chunk = id % chunks; id /= chunks;
    const int tx = id % tiles_x; id /= tiles_x;
    const int y = id % H;
    const int b = (int)(id / H);
    const int R = P / 2;
    const int x0 = tx * TF_TW;
    const int LDW = MODE == 0 ? TF_TW : TF_TW + 2 * R;
    const int PP = P * P;
    const int64_t HW = (int64_t)H * W;
    const float* gb = gout + (int64_t)b * Ctot * HW;
    const float* ob = outp + (int64_t)b * Ctot * HW;
    const float* src = fpn + (int64_t)(2 * b + (MODE == 0 ? 1 : 0)) * C * HW;
    float* dst = gfpn + (int64_t)(2 * b + (MODE == 0 ? 0 : 1)) * C * HW;
    if (LDS) {
        for (int e = threadIdx.x; e < PP * LDW; e += 256) {
            const int ij = e / LDW, xx = e - ij * LDW;
            const int i = ij / P;
            const int yy = MODE == 0 ? y : y - (i - R);
            const int xg = MODE == 0 ? x0 + xx : x0 - R + xx;
            gs[e] = (yy >= 0 && yy < H && xg >= 0 && xg < W) ? t2s_gated(gb, ob, (int64_t)ij * HW + (int64_t)yy * W + xg, inv_c) : 0.0f;
        }
        __syncthreads();
    }
    const int xl = threadIdx.x & (TF_TW - 1);
    const int x = x0 + xl;
    if (x >= W) return;
    const int c0 = chunk * cch, c1 = min(C, c0 + cch);
    for (int c = c0 + (threadIdx.x >> 6); c < c1; c += 4) {
        const float* sc = src + (int64_t)c * HW;
        float acc = 0.0f;
        for (int i = 0; i < P; ++i) {
            const int dy = i - R;
            const int ys = MODE == 0 ? y + dy : y - dy;
            if (ys < 0 || ys >= H) continue;
            for (int j = 0; j < P; ++j) {
                const int dx = j - R;
                const int xs = MODE == 0 ? x + dx : x - dx;
                if (xs < 0 || xs >= W) continue;
                float gv;
                if (LDS) gv = MODE == 0 ? gs[(i * P + j) * LDW + xl] : gs[(i * P + j) * LDW + xl + R - dx];
                else gv = t2s_gated(gb, ob, (int64_t)(i * P + j) * HW + (MODE == 0 ? (int64_t)y * W + x : (int64_t)ys * W + xs), inv_c);
                acc = fmaf(gv, sc[(int64_t)ys * W + xs], acc);
            }
        }
        dst[(int64_t)c * HW + (int64_t)y * W + x] = acc;
    }
}

template <int MODE>
int t2s_corr_backward_launch(const float* gout, const float* outp, const float* fpn, float* gfpn, int bs, int C, int H, int W, int P, int Ctot,
                             stm_stream_t stream)
{
    const int R = P / 2;
    const int tiles_x = stm_cdiv(W, TF_TW);
    const int64_t rows = (int64_t)bs * H * tiles_x;
    int cch = 32;
    while (cch > 4 && rows * stm_cdiv(C, cch) < 2048) cch /= 2;
    const int chunks = stm_cdiv(C, cch);
    const size_t lds = (size_t)P * P * (MODE == 0 ? TF_TW : TF_TW + 2 * R) * sizeof(float);
    STM_REQUIRE(rows * chunks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "stm_t2s_feat_backward_f32: grid too large");
    const dim3 grid((unsigned)(rows * chunks));
    const float inv_c = 1.0f / (float)C;
    if (lds <= 48 * 1024) {
        hipLaunchKernelGGL((t2s_corr_backward_kernel<MODE, true>), grid, dim3(256), lds, stm_hs(stream), gout, outp, fpn, gfpn, C, H, W, P, Ctot, cch,
                           tiles_x, chunks, inv_c);
    } else {
        hipLaunchKernelGGL((t2s_corr_backward_kernel<MODE, false>), grid, dim3(256), 0, stm_hs(stream), gout, outp, fpn, gfpn, C, H, W, P, Ctot, cch,
                           tiles_x, chunks, inv_c);
    }
    STM_CHECK_LAUNCH("t2s_corr_backward_kernel");
    return STM_OK;
}

int t2s_check_shapes(const char* who, int bs, int C, int Cu, int H, int W, int P)
{
    STM_REQUIRE(bs > 0 && C > 0 && Cu > 0 && H > 0 && W > 0, STM_EINVAL, "%s: bs=%d C=%d Cu=%d H=%d W=%d", who, bs, C, Cu, H, W);
    STM_REQUIRE(P > 0 && (P & 1), STM_EINVAL, "%s: patch size %d must be odd and positive", who, P);
    const int64_t lim = (int64_t)1 << 31, HW = (int64_t)H * W;
    STM_REQUIRE(P < 46341 && (int64_t)P * P * HW < lim && (int64_t)C * HW < lim && (int64_t)Cu * HW < lim, STM_EUNSUPPORTED,
                "%s: P*P*H*W, C*H*W and Cu*H*W must stay below 2^31", who);
    return STM_OK;
}

}  // namespace

extern "C" int stm_t2s_feat_forward_f32(const float* fpn, const float* t2s, float* out, int bs, int C, int Cu, int H, int W, int P,
                                        stm_stream_t stream)
{
    const char* who = "stm_t2s_feat_forward_f32";
    int rc = t2s_check_shapes(who, bs, C, Cu, H, W, P);
    if (rc) return rc;
    STM_REQUIRE(fpn && t2s && out, STM_ENULL, "%s: fpn/t2s/out must be non-NULL", who);
    const int64_t HW = (int64_t)H * W, PP = (int64_t)P * P;
    const int Ctot = (int)PP + 2 * Cu;
    const float inv_c = 1.0f / (float)C;
    if (P == 11) {
        const int tiles_x = stm_cdiv(W, TF_TW), igroups = stm_cdiv(P, TF_ROWS);
        const int64_t blocks = (int64_t)bs * H * tiles_x * igroups;
        STM_REQUIRE(blocks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: grid too large", who);
        hipLaunchKernelGGL((t2s_corr_forward_kernel<11>), dim3((unsigned)blocks), dim3(256), 0, stm_hs(stream), fpn, out, C, H, W, Ctot, tiles_x,
                           igroups, inv_c);
    } else {
        const int64_t blocks = ((int64_t)bs * PP * HW + 255) / 256;
        STM_REQUIRE(blocks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: grid too large", who);
        hipLaunchKernelGGL(t2s_corr_forward_any_kernel, dim3((unsigned)blocks), dim3(256), 0, stm_hs(stream), fpn, out, bs, C, H, W, P, Ctot, inv_c);
    }
    STM_CHECK_LAUNCH("t2s_corr_forward_kernel");
    return t2s_copy_launch<false>(t2s, nullptr, out, bs, Cu, HW, PP, Ctot, stream);
}

extern "C" int stm_t2s_feat_backward_f32(const float* grad_out, const float* out, const float* fpn, const float* t2s, float* grad_fpn,
                                         float* grad_t2s, int bs, int C, int Cu, int H, int W, int P, stm_stream_t stream)
{
    const char* who = "stm_t2s_feat_backward_f32";
    int rc = t2s_check_shapes(who, bs, C, Cu, H, W, P);
    if (rc) return rc;
    STM_REQUIRE(grad_fpn || grad_t2s, STM_ENULL, "%s: neither grad_fpn nor grad_t2s given (NULL)", who);
    STM_REQUIRE(grad_out && (!grad_fpn || (out && fpn)) && (!grad_t2s || t2s), STM_ENULL, "%s: grad_out and the saved tensors of the gradients asked "
                "for must be non-NULL", who);
    const int64_t HW = (int64_t)H * W, PP = (int64_t)P * P;
    const int Ctot = (int)PP + 2 * Cu;
    if (grad_fpn) {
        rc = t2s_corr_backward_launch<0>(grad_out, out, fpn, grad_fpn, bs, C, H, W, P, Ctot, stream);
        if (rc) return rc;
        rc = t2s_corr_backward_launch<1>(grad_out, out, fpn, grad_fpn, bs, C, H, W, P, Ctot, stream);
        if (rc) return rc;
    }
    if (grad_t2s) return t2s_copy_launch<true>(t2s, grad_out, grad_t2s, bs, Cu, HW, PP, Ctot, stream);
    return STM_OK;
}
