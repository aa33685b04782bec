// pos_index.h -- the ordered list of the positive priors of a batch, shared by pos_loss.hip (track loss: positive iff conf_t > 0), t2s_loss.hip
// (temporal-fusion loss: positive iff pos_t > 0) and mbox_loss.hip (mask term: positive iff conf_t > 0).  Three steps over tiles of 256 consecutive priors of ONE image (tiles do not straddle images):
//   count   positives per tile (t2s_loss.hip's target kernel writes these counts itself and skips this launch)
//   scan    one workgroup: the tiles' exclusive prefix, n, npos_b, the track loss's W; optionally the [B + 1] prefix of the per-image counts and
//           the status word n > cap
//   index   the flattened rows of the positives in order, and their weights 1 / max(npos_b, 1)
// Integer sums only: the list is the same from run to run.  The workspace layout (pos_layout), the shape check (pos_check) and the launch
// sequence (pos_list) of the three users are here too.
#pragma once
#include "stm_common.h"

namespace {

constexpr int PL_TILE = 256;
constexpr int PL_MAX_N = 1 << 22;

enum { TM_N = 0, TM_STATUS = 1, TM_W = 2, TM_WORDS = 4 };   // meta: n, the status word (1: n exceeds the caller's cap), then W as a double at word 2

// the list's workspace, in 32-bit words; `extra` is the user's own block (the track loss's partial doubles), 8-byte aligned behind the 4 meta words
struct PosLayout {
    size_t meta, extra, tilecnt, tilepre, npos, idx, wts, words;
};

PosLayout pos_layout(int B, int P, size_t extra_words = 0)
{
    const size_t nT = (size_t)B * stm_cdiv(P, PL_TILE), N = (size_t)B * P;
    PosLayout L;
    size_t o = 0;
    L.meta = o;    o += TM_WORDS;
    L.extra = o;   o += extra_words;
    L.tilecnt = o; o += nT;
    L.tilepre = o; o += nT;
    L.npos = o;    o += (size_t)B;
    L.idx = o;     o += N;
    L.wts = o;     o += N;
    L.words = o;
    return L;
}

int pos_check(const char* who, int B, int P)
{
    STM_REQUIRE(B >= 1 && P >= 1, STM_EINVAL, "%s: B=%d P=%d", who, B, P);
    STM_REQUIRE((int64_t)B * P <= PL_MAX_N, STM_EUNSUPPORTED, "%s: B*P=%lld > %d rows", who, (long long)B * P, PL_MAX_N);
    return STM_OK;
}

__device__ __forceinline__ float pl_weight(unsigned npos) { return (float)(1.0 / (double)(npos > 1u ? npos : 1u)); }

// the tile's image, its first row in the flattened [B * P] order and how many of its 256 threads have a row
__device__ __forceinline__ void pl_tile(int tpi, int P, int& img, int64_t& row0, int& rows)
{
    img = blockIdx.x / tpi;
    const int p0 = (blockIdx.x - img * tpi) * PL_TILE;
    row0 = (int64_t)img * P + p0;
    rows = min(PL_TILE, P - p0);
}

__global__ __launch_bounds__(256) void pos_count_kernel(const int64_t* __restrict__ conf_t, unsigned* __restrict__ tilecnt, int P, int tpi)
{
    __shared__ unsigned sc[4];
    int img, rows;
    int64_t row0;
    pl_tile(tpi, P, img, row0, rows);
    const int tid = threadIdx.x;
    const bool pos = tid < rows && conf_t[row0 + tid] > 0;
    const unsigned long long m = __ballot(pos);
    if ((tid & 63) == 0) sc[tid >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (tid == 0) tilecnt[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

// prefix: null, or [B + 1] ints: the exclusive prefix of npos over the images, prefix[B] = n.  cap: the most rows the caller has room for.
__global__ __launch_bounds__(256) void pos_scan_kernel(const unsigned* __restrict__ tilecnt, unsigned* tilepre, unsigned* __restrict__ npos,
                                                       unsigned* __restrict__ meta, int* __restrict__ prefix, unsigned cap, int nT, int B, int tpi)
{
    __shared__ unsigned sw[4];
    __shared__ double sd[4];
    const int tid = threadIdx.x;
    const int chunk = (nT + 255) / 256;
    const int lo = min(nT, tid * chunk), hi = min(nT, lo + chunk);
    unsigned s = 0, total;
    for (int i = lo; i < hi; ++i) s += tilecnt[i];
    unsigned a = stm_block_excl_scan(s, sw, total);
    for (int i = lo; i < hi; ++i) {
        tilepre[i] = a;
        a += tilecnt[i];
    }
    double s1 = 0.0, s2 = 0.0;
    for (int b = tid; b < B; b += 256) {
        unsigned cnt = 0;
        for (int t = 0; t < tpi; ++t) cnt += tilecnt[(size_t)b * tpi + t];
        npos[b] = cnt;
        const double w = (double)pl_weight(cnt);
        s1 += (double)cnt * w;
        s2 += (double)cnt * w * w;
    }
    s1 = stm_block_sum_f64(s1, sd);                              // (its barriers publish tilepre to the workgroup)
    s2 = stm_block_sum_f64(s2, sd);
    if (prefix) {
        for (int b = tid; b < B; b += 256) prefix[b] = (int)tilepre[(size_t)b * tpi];   // an image's first tile
        if (tid == 0) prefix[B] = (int)total;
    }
    if (tid == 0) {
        meta[TM_N] = total;
        meta[TM_STATUS] = total > cap ? 1u : 0u;
        *reinterpret_cast<double*>(meta + TM_W) = total >= 2u ? (s1 * s1 - s2) / 2.0 : 0.0;
    }
}

__global__ __launch_bounds__(256) void pos_index_kernel(const int64_t* __restrict__ conf_t, const unsigned* __restrict__ tilepre,
                                                        const unsigned* __restrict__ npos, int* __restrict__ idx, float* __restrict__ wts, int P,
                                                        int tpi)
{
    __shared__ unsigned sw[4];
    int img, rows;
    int64_t row0;
    pl_tile(tpi, P, img, row0, rows);
    const int tid = threadIdx.x;
    const bool pos = tid < rows && conf_t[row0 + tid] > 0;
    unsigned total;
    const unsigned rank = tilepre[blockIdx.x] + stm_block_excl_scan(pos ? 1u : 0u, sw, total);
    if (pos) {
        idx[rank] = (int)(row0 + tid);
        wts[rank] = pl_weight(npos[img]);
    }
}

// The launches count (unless the caller's own kernel wrote the tiles' counts), scan, index over a workspace laid out by pos_layout(B, P, ...).
// flag: a prior is listed iff flag > 0.  prefix: null or [B + 1] ints.  max_rows: the caller's cap behind the status word, 0 for none.
int pos_list(const int64_t* flag, bool count, int* prefix, int max_rows, int B, int P, unsigned* ws, const PosLayout& L, hipStream_t st)
{
    const int tpi = stm_cdiv(P, PL_TILE), nT = B * tpi;
    if (count) {
        hipLaunchKernelGGL(pos_count_kernel, dim3(nT), dim3(256), 0, st, flag, ws + L.tilecnt, P, tpi);
        STM_CHECK_LAUNCH("pos_count_kernel");
    }
    hipLaunchKernelGGL(pos_scan_kernel, dim3(1), dim3(256), 0, st, ws + L.tilecnt, ws + L.tilepre, ws + L.npos, ws + L.meta, prefix,
                       max_rows > 0 ? (unsigned)max_rows : 0xFFFFFFFFu, nT, B, tpi);
    STM_CHECK_LAUNCH("pos_scan_kernel");
    hipLaunchKernelGGL(pos_index_kernel, dim3(nT), dim3(256), 0, st, flag, ws + L.tilepre, ws + L.npos, reinterpret_cast<int*>(ws + L.idx),
                       reinterpret_cast<float*>(ws + L.wts), P, tpi);
    STM_CHECK_LAUNCH("pos_index_kernel");
    return STM_OK;
}

}  // namespace
