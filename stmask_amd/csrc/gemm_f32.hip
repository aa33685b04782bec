// gemm_f32.hip -- fp32 GEMM on the gfx950 matrix pipe (v_mfma_f32_32x32x2_f32) with fused bias / ReLU.
//
// The GEMM half of the deformable convolution: y[b] = W[O, C*K] x cols[b][C*K, Ho*Wo] + bias
// (dcn_v2 / mmcv call cuBLAS sgemm here; backbone.py:45, Featurealign.py:72).  fp32-in / fp32-accumulate
// MFMA is an exact k-ordered fmaf chain (MI355X guide §3), so results are deterministic and independent of
// the tiling.  MFMA-bound: 157 TFLOP/s dense fp32 peak.
//
// Tiling: workgroup 256 threads = 4 waves (2x2); block tile BM x BN, wave tile (BM/2) x (BN/2) made of 32x32
// MFMA tiles; BK = 16.  A (weights, [M][K] row-major) is transposed on the way into LDS (As[BK][BM+2]: the +2
// pad makes the transposing ds_write_b32 conflict-free), B (columns, [K][N] row-major) is copied as is
// (Bs[BK][BN]).  Operand fetch is one conflict-free ds_read_b32 per 32x32x2 MFMA operand.  The next K-slab is
// prefetched global->registers while the current one is multiplied.
#include "stm_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int BK = 16;

template <int BM, int BN>
__global__ __launch_bounds__(256) void gemm_bias_f32_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                            const float* __restrict__ bias, float* __restrict__ Cm,
                                                            int M, int N, int Kd, int64_t b_bs, int64_t c_bs,
                                                            int relu, int n_tiles)
{
    constexpr int TM = BM / 64;       // 32x32 tiles per wave along M
    constexpr int TN = BN / 64;       // along N
    constexpr int LDA = BM + 2;       // padded leading dimension of As
    constexpr int A_F4 = BM * BK / 4 / 256;  // float4 loads per thread for the A slab
    constexpr int B_F4 = BN * BK / 4 / 256;  // for the B slab
    static_assert(A_F4 >= 1 && B_F4 >= 1, "tile too small for 256 threads");

    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * BN];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_n = blockIdx.x % n_tiles, tile_m = blockIdx.x / n_tiles;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int batch = blockIdx.y;
    const float* Bp = Bm + (int64_t)batch * b_bs;
    float* Cp = Cm + (int64_t)batch * c_bs;

    const bool n_vec = (N % 4 == 0);  // rows of B are 16-byte aligned
    const bool k_vec = (Kd % 4 == 0);

    float4 ra[A_F4], rb[B_F4];

    auto load_slab = [&](int k0) {
#pragma unroll
        for (int t = 0; t < A_F4; ++t) {
            int f = tid + t * 256;          // float4 index in the [BM][BK/4] slab
            int row = f / (BK / 4), kq = f % (BK / 4);
            int gm = m0 + row, gk = k0 + kq * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gm < M) {
                const float* p = A + (int64_t)gm * Kd + gk;
                if (k_vec && gk + 3 < Kd) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    if (gk < Kd) v.x = p[0];
                    if (gk + 1 < Kd) v.y = p[1];
                    if (gk + 2 < Kd) v.z = p[2];
                    if (gk + 3 < Kd) v.w = p[3];
                }
            }
            ra[t] = v;
        }
#pragma unroll
        for (int t = 0; t < B_F4; ++t) {
            int f = tid + t * 256;          // float4 index in the [BK][BN/4] slab
            int kr = f / (BN / 4), nq = f % (BN / 4);
            int gk = k0 + kr, gn = n0 + nq * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gk < Kd) {
                const float* p = Bp + (int64_t)gk * N + gn;
                if (n_vec && gn + 3 < N) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    if (gn < N) v.x = p[0];
                    if (gn + 1 < N) v.y = p[1];
                    if (gn + 2 < N) v.z = p[2];
                    if (gn + 3 < N) v.w = p[3];
                }
            }
            rb[t] = v;
        }
    };

    auto store_slab = [&]() {
#pragma unroll
        for (int t = 0; t < A_F4; ++t) {
            int f = tid + t * 256;
            int row = f / (BK / 4), kq = f % (BK / 4);
            As[(kq * 4 + 0) * LDA + row] = ra[t].x;
            As[(kq * 4 + 1) * LDA + row] = ra[t].y;
            As[(kq * 4 + 2) * LDA + row] = ra[t].z;
            As[(kq * 4 + 3) * LDA + row] = ra[t].w;
        }
#pragma unroll
        for (int t = 0; t < B_F4; ++t) {
            int f = tid + t * 256;
            int kr = f / (BN / 4), nq = f % (BN / 4);
            *reinterpret_cast<float4*>(&Bs[kr * BN + nq * 4]) = rb[t];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int lrow = lane & 31, lk = lane >> 5;
    const int a_base = wm * (BM / 2) + lrow;
    const int b_base = wn * (BN / 2) + lrow;

    load_slab(0);
    for (int k0 = 0; k0 < Kd; k0 += BK) {
        __syncthreads();  // previous slab fully consumed
        store_slab();
        __syncthreads();
        if (k0 + BK < Kd) load_slab(k0 + BK);  // prefetch the next slab behind the MFMAs
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[(kk + lk) * LDA + a_base + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[(kk + lk) * BN + b_base + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int gn = n0 + wn * (BN / 2) + j * 32 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int gm = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (gm < M && gn < N) {
                    float v = acc[i][j][r];
                    if (bias) v = v + bias[gm];
                    if (relu) v = v > 0.0f ? v : 0.0f;
                    Cp[(int64_t)gm * N + gn] = v;
                }
            }
        }
}

}  // namespace


// ------------------------------------------------------------------------------------------------------------------
// 128 x 128 x 32 tile, double-buffered LDS, one barrier per K-slab, optional split-K (deterministic two-pass reduce).
//
// Why a second kernel: at 1-2 waves per SIMD the instruction stream, not the MFMA pipe, sets the pace (same finding
// as for the im2col kernel).  This one keeps the per-wave stream lean: A stays [m][k] in LDS (no transposing stores)
// and each lane fetches its 16 k-values of a slab with 4 ds_read_b128 thanks to a K permutation -- MFMA step s of
// lane-half h uses k = 16h + s for BOTH operands, which is legal because a GEMM is invariant under any permutation of
// K applied to A and B alike; the next slab's global loads are issued before the 64 MFMAs of the current one and land
// in the other LDS buffer afterwards.  A row = 36 floats (144 B): the 16 rows of a ds_read_b128 group fall on 16
// distinct 16-byte bank groups.  Small grids (M x N / 128^2 x batch < 256 workgroups) are split along K.
namespace {

constexpr int G2_BM = 128, G2_BN = 128, G2_BK = 32, G2_LDA = G2_BK + 4;

__global__ __launch_bounds__(256) void gemm128_f32_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                          const float* __restrict__ bias, float* __restrict__ Cm, int M,
                                                          int N, int Kd, int64_t b_bs, int64_t c_bs, int relu, int n_tiles,
                                                          int splitk, int k_per_split, float* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float As[2][G2_BM * G2_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][G2_BK * G2_BN];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_n = blockIdx.x % n_tiles, tile_m = blockIdx.x / n_tiles;
    const int m0 = tile_m * G2_BM, n0 = tile_n * G2_BN;
    const int batch = blockIdx.y, ks = blockIdx.z;
    const int k_begin = ks * k_per_split, k_end = min(Kd, k_begin + k_per_split);
    const float* Bp = Bm + (int64_t)batch * b_bs;

    // global -> register staging: A: 128 rows x 8 float4 (row = tid/8 + 32 i, kq = tid%8); B: 32 rows x 32 float4.
    // No bounds tests in the loop: M % 128 == 0 and K % 32 == 0 are launch conditions, and B columns beyond N are read
    // from a clamped (valid) address -- they only feed output columns that are never stored.
    const int a_row = tid >> 3, a_kq = tid & 7;
    const int b_row = tid >> 5, b_nq = tid & 31;
    const float* ap0 = A + (int64_t)(m0 + a_row) * Kd + k_begin + a_kq * 4;
    const float* bp0 = Bp + (int64_t)(k_begin + b_row) * N + min(n0 + b_nq * 4, N - 4);
    const int64_t a_step = (int64_t)32 * Kd, b_step = (int64_t)8 * N;
    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;   // named scalars: an array captured by a lambda went to scratch
#define G2_LOAD_SLAB(slab)                                                            \
    {                                                                                 \
        const float* ap_ = ap0 + (int64_t)(slab) * G2_BK;                             \
        const float* bp_ = bp0 + (int64_t)(slab) * G2_BK * N;                         \
        ra0 = *reinterpret_cast<const float4*>(ap_);                                  \
        ra1 = *reinterpret_cast<const float4*>(ap_ + a_step);                         \
        ra2 = *reinterpret_cast<const float4*>(ap_ + 2 * a_step);                     \
        ra3 = *reinterpret_cast<const float4*>(ap_ + 3 * a_step);                     \
        rb0 = *reinterpret_cast<const float4*>(bp_);                                  \
        rb1 = *reinterpret_cast<const float4*>(bp_ + b_step);                         \
        rb2 = *reinterpret_cast<const float4*>(bp_ + 2 * b_step);                     \
        rb3 = *reinterpret_cast<const float4*>(bp_ + 3 * b_step);                     \
    }
#define G2_STORE_SLAB(buf_)                                                                            \
    {                                                                                                  \
        float* as_ = &As[buf_][a_row * G2_LDA + a_kq * 4];                                             \
        float* bs_ = &Bs[buf_][b_row * G2_BN + b_nq * 4];                                              \
        *reinterpret_cast<float4*>(as_) = ra0;                                                         \
        *reinterpret_cast<float4*>(as_ + 32 * G2_LDA) = ra1;                                           \
        *reinterpret_cast<float4*>(as_ + 64 * G2_LDA) = ra2;                                           \
        *reinterpret_cast<float4*>(as_ + 96 * G2_LDA) = ra3;                                           \
        *reinterpret_cast<float4*>(bs_) = rb0;                                                         \
        *reinterpret_cast<float4*>(bs_ + 8 * G2_BN) = rb1;                                             \
        *reinterpret_cast<float4*>(bs_ + 16 * G2_BN) = rb2;                                            \
        *reinterpret_cast<float4*>(bs_ + 24 * G2_BN) = rb3;                                            \
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int lrow = lane & 31, lh = lane >> 5;
    const int n_slabs = (k_end - k_begin) / G2_BK;
    G2_LOAD_SLAB(0);
    G2_STORE_SLAB(0);
    __syncthreads();
    int buf = 0;
    for (int sl = 0; sl < n_slabs; ++sl) {
        // next slab in flight behind the MFMAs below (the last iteration re-reads its own slab: no branch)
        G2_LOAD_SLAB(min(sl + 1, n_slabs - 1));
        // all fragments of this slab first (8 ds_read_b128 + 32 ds_read_b32), then 64 back-to-back MFMAs: left to
        // itself the compiler fetched each B fragment right before its MFMA group and stalled on LDS latency 16 times
        float af[2][16], bf[2][16];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float* ap = &As[buf][(wm * 64 + i * 32 + lrow) * G2_LDA + lh * 16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(ap + 4 * q);
                af[i][4 * q] = v.x; af[i][4 * q + 1] = v.y; af[i][4 * q + 2] = v.z; af[i][4 * q + 3] = v.w;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* bp = &Bs[buf][(lh * 16) * G2_BN + wn * 64 + j * 32 + lrow];
#pragma unroll
            for (int s_ = 0; s_ < 16; ++s_) bf[j][s_] = bp[s_ * G2_BN];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s_], bf[j][s_], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        G2_STORE_SLAB(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // epilogue (C/D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
    float* Cp = (splitk > 1) ? partial + ((int64_t)ks * gridDim.y + batch) * (int64_t)M * N : Cm + (int64_t)batch * c_bs;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gn = n0 + wn * 64 + j * 32 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (gm < M && gn < N) {
                    float v = acc[i][j][r];
                    if (splitk == 1) {
                        if (bias) v = v + bias[gm];
                        if (relu) v = v > 0.0f ? v : 0.0f;
                    }
                    Cp[(int64_t)gm * N + gn] = v;
                }
            }
        }
}

// sums the split-K partials in a fixed order (deterministic), adds bias, applies ReLU
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                                            float* __restrict__ Cm, int M, int N, int batch, int64_t c_bs,
                                                            int splitk, int relu)
{
    const int64_t mn4 = (int64_t)M * N / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= mn4) return;
    const int64_t stride = (int64_t)batch * M * N;
    const float* p = partial + (int64_t)b * M * N + t * 4;
    float4 v = *reinterpret_cast<const float4*>(p);
    for (int s_ = 1; s_ < splitk; ++s_) {
        const float4 u = *reinterpret_cast<const float4*>(p + s_ * stride);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    if (bias) {
        const float bb = bias[(t * 4) / N];   // N % 4 == 0: the 4 elements share a row
        v.x += bb; v.y += bb; v.z += bb; v.w += bb;
    }
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    *reinterpret_cast<float4*>(Cm + (int64_t)b * c_bs + t * 4) = v;
}

}  // namespace

// internal entry with workspace for split-K partials (ws may be NULL: then no split)
static int gemm_dispatch(const float* A, const float* Bmat, const float* bias, float* Cmat, int M, int N, int K, int batch,
                         int64_t b_bstride, int64_t c_bstride, int relu, void* ws, size_t ws_bytes, stm_stream_t stream);


extern "C" int stm_gemm_bias_f32(const float* A, const float* Bmat, const float* bias, float* Cmat, int M, int N, int K,
                                 int batch, int64_t b_bstride, int64_t c_bstride, int relu, stm_stream_t stream)
{
    return gemm_dispatch(A, Bmat, bias, Cmat, M, N, K, batch, b_bstride, c_bstride, relu, nullptr, 0, stream);
}

extern "C" size_t stm_gemm_workspace_bytes(int M, int N, int batch)
{
    size_t b = (size_t)8 * batch * M * N * sizeof(float);
    return b > ((size_t)64 << 20) ? ((size_t)64 << 20) : b;
}

extern "C" int stm_gemm_bias_ws_f32(const float* A, const float* Bmat, const float* bias, float* Cmat, int M, int N, int K,
                                    int batch, int64_t b_bstride, int64_t c_bstride, int relu, void* workspace,
                                    size_t workspace_bytes, stm_stream_t stream)
{
    return gemm_dispatch(A, Bmat, bias, Cmat, M, N, K, batch, b_bstride, c_bstride, relu, workspace, workspace_bytes, stream);
}

static int gemm_dispatch(const float* A, const float* Bmat, const float* bias, float* Cmat, int M, int N, int K, int batch,
                         int64_t b_bstride, int64_t c_bstride, int relu, void* ws, size_t ws_bytes, stm_stream_t stream)
{
    STM_REQUIRE(A && Bmat && Cmat, STM_ENULL, "stm_gemm_bias_f32: A/B/C must be non-NULL");
    STM_REQUIRE(M > 0 && N > 0 && K > 0 && batch > 0, STM_EINVAL, "stm_gemm_bias_f32: bad sizes M=%d N=%d K=%d batch=%d",
                M, N, K, batch);
    STM_REQUIRE(batch <= 65535, STM_EINVAL, "stm_gemm_bias_f32: batch %d > 65535", batch);
    STM_REQUIRE(((uintptr_t)A % 16 == 0) && ((uintptr_t)Bmat % 16 == 0) && (b_bstride % 4 == 0 || N % 4 != 0),
                STM_EINVAL, "stm_gemm_bias_f32: A and B must be 16-byte aligned");
    // 128^2 double-buffered kernel: needs whole 128-row tiles, float4-loadable A and B rows
    const bool ok128 = (M % 128 == 0) && (K % 32 == 0) && (N % 4 == 0) && (N >= 4) && (c_bstride % 4 == 0) && ((uintptr_t)Cmat % 16 == 0);
    if (ok128) {
        const int nt = stm_cdiv(N, G2_BN);
        const int64_t blocks = (int64_t)nt * (M / G2_BM) * batch;
        int splitk = 1;
        while (splitk < 8 && blocks * splitk < 224 && K / (splitk * 2) >= 256) splitk *= 2;
        if (splitk > 1 && (!ws || ws_bytes < (size_t)splitk * batch * M * N * sizeof(float))) splitk = 1;
        int kps = stm_cdiv(stm_cdiv(K, splitk), G2_BK) * G2_BK;
        splitk = stm_cdiv(K, kps);
        dim3 grid(nt * (M / G2_BM), batch, splitk);
        hipLaunchKernelGGL(gemm128_f32_kernel, grid, dim3(256), 0, stm_hs(stream), A, Bmat, bias, Cmat, M, N, K, b_bstride,
                           c_bstride, relu, nt, splitk, kps, static_cast<float*>(ws));
        STM_CHECK_LAUNCH("gemm128_f32_kernel");
        if (splitk > 1) {
            hipLaunchKernelGGL(splitk_reduce_kernel, dim3(stm_cdiv((int64_t)M * N / 4, 256), batch), dim3(256), 0, stm_hs(stream),
                               static_cast<const float*>(ws), bias, Cmat, M, N, batch, c_bstride, splitk, relu);
            STM_CHECK_LAUNCH("splitk_reduce_kernel");
        }
        return STM_OK;
    }
    // general shapes: 64x64 (or 128x128 single-buffered) tiles with full edge handling
    int64_t big = (int64_t)stm_cdiv(M, 128) * stm_cdiv(N, 128) * batch;
    const int tile = (big >= 512 && M >= 128) ? 128 : 64;
    if (tile == 128) {
        int nt = stm_cdiv(N, 128);
        dim3 grid(nt * stm_cdiv(M, 128), batch);
        hipLaunchKernelGGL((gemm_bias_f32_kernel<128, 128>), grid, dim3(256), 0, stm_hs(stream), A, Bmat, bias, Cmat, M,
                           N, K, b_bstride, c_bstride, relu, nt);
    } else {
        int nt = stm_cdiv(N, 64);
        dim3 grid(nt * stm_cdiv(M, 64), batch);
        hipLaunchKernelGGL((gemm_bias_f32_kernel<64, 64>), grid, dim3(256), 0, stm_hs(stream), A, Bmat, bias, Cmat, M, N,
                           K, b_bstride, c_bstride, relu, nt);
    }
    STM_CHECK_LAUNCH("gemm_bias_f32_kernel");
    return STM_OK;
}

extern "C" size_t stm_deform_conv_workspace_bytes(const stm_deform_geom* g)
{
    if (!g) return 0;
    // column buffer + room for the split-K partial outputs (up to 8 x [B, O, Ho*Wo], O <= 4*C; capped at 64 MB)
    size_t cols = (size_t)g->B * g->C * g->kh * g->kw * g->Ho * g->Wo * sizeof(float);
    size_t part = (size_t)8 * g->B * (4 * (size_t)g->C) * g->Ho * g->Wo * sizeof(float);
    if (part > ((size_t)64 << 20)) part = (size_t)64 << 20;  // split-K only runs on small outputs (grid < 224 tiles)
    return cols + part + 256;
}

extern "C" int stm_deform_conv_fwd_f32(const float* x, const float* offset, int64_t off_bstride, const float* mask,
                                       int64_t mask_bstride, int mask_is_logit, const float* weight, const float* bias,
                                       float* y, int O, int relu, const stm_deform_geom* g, void* workspace,
                                       size_t workspace_bytes, stm_stream_t stream)
{
    STM_REQUIRE(g, STM_ENULL, "stm_deform_conv_fwd_f32: geometry is NULL");
    STM_REQUIRE(weight && y, STM_ENULL, "stm_deform_conv_fwd_f32: weight/y must be non-NULL");
    STM_REQUIRE(O > 0, STM_EINVAL, "stm_deform_conv_fwd_f32: O=%d", O);
    size_t need = stm_deform_conv_workspace_bytes(g);
    STM_REQUIRE(workspace && workspace_bytes >= need, STM_EWORKSPACE,
                "stm_deform_conv_fwd_f32: workspace %zu bytes < required %zu", workspace_bytes, need);
    float* cols = static_cast<float*>(workspace);
    int rc = stm_deform_im2col_f32(x, offset, off_bstride, mask, mask_bstride, mask_is_logit, cols, g, 0, stream);
    if (rc) return rc;
    const int CK = g->C * g->kh * g->kw, HWo = g->Ho * g->Wo;
    const size_t cols_bytes = (((size_t)g->B * CK * HWo * sizeof(float)) + 255) / 256 * 256;
    void* part = static_cast<char*>(workspace) + cols_bytes;
    const size_t part_bytes = workspace_bytes > cols_bytes ? workspace_bytes - cols_bytes : 0;
    return gemm_dispatch(weight, cols, bias, y, O, HWo, CK, g->B, (int64_t)CK * HWo, (int64_t)O * HWo, relu, part, part_bytes,
                         stream);
}
