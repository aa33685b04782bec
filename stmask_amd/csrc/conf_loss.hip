// conf_loss.hip -- the class-confidence loss with online hard example mining of the reference's MultiBoxLoss (layers/modules/multibox_loss.py:402-448:
// select_neg_bboxes and ohem_conf_loss, ohem_use_most_confident = False) as a fixed sequence of launches for gfx950: no sort, no gather, no host
// synchronisation, no float atomics.  With N = B * P, x = conf_data [N, C], t = conf_t [N] (conventions: include/stmask_hip.h):
//     lse_i = m_i + log(sum_c exp(x_ic - m_i)) with the row's own maximum m_i, evaluated in double and rounded once to fp32;
//     score_i = fp32(lse_i - x_i0) where t_i == 0, exactly +0 elsewhere, so score_i >= 0 and its bit pattern orders like an unsigned integer;
//     k = min(ratio * #(t > 0), N - 1); a row is a selected negative iff t_i == 0 and it is among the k largest scores of all N rows under
//     (score descending, index ascending); kept rows = positives + selected negatives; C = alpha * sum_i w_i (lse_i - x_{i,t_i}) / (ratio + 1).
//
// Launches (8 for the loss, 7 for the selection alone; every grid depends on (B, P, C) only):
//   1 zero          the counters and the three radix histograms
//   2 score         a workgroup owns 256 consecutive rows: their contiguous floats come into LDS with aligned 16-byte loads (a row of 41 floats is
//                   not 16-byte aligned, a run of 64 rows is), the row stride is made odd so that one thread per row reads without bank conflicts;
//                   writes lse, the score bits and ce_i = lse_i - x_{i,t_i}, counts the positives per image and builds the histogram of score
//                   bits 31..21 (LDS histogram, then one integer add per non-empty bin and workgroup)
//   3 hist<1>       every workgroup finds the bin of the k-th largest score in histogram 0 (radix_pick: 2048 words, cheaper than a launch of its
//                   own), then counts bits 20..10 of the scores inside that bin
//   4 hist<2>       the same one level down: bits 9..0 of the scores that match the first 22 bits
//   5 tile counts   the last pick gives the cut value T and how many scores equal to T are taken (in index order); per 256-row tile the counts of
//                   scores == T, of true negatives with score == T, of scores > T and of positives
//   6 scan          one workgroup: prefix sums over the tiles of the scores == T (ties resolved by index) and of the kept rows (the rank of every
//                   kept row, for the reference's positional weights), the number of selected negatives, the prefix of positives per image
//   7 weights       w_i per row (both weight modes), the 0 / 1 selection on request, and the tile's sum of w_i * ce_i in double, fixed order
//   8 reduce        one workgroup adds the tile sums in a fixed order and scales
// Adjoint: one launch over the same 256-row tiles; rows with w_i = 0 are written as zeros without reading x (16-byte stores), the others read x
// and lse: grad_x[i,c] = g * alpha / (ratio + 1) * w_i * (exp(x_ic - lse_i) - [c == t_i]).
// A label >= C is data: nothing is read through it, that row's term and gradient row are NaN.
#include "stm_common.h"

namespace {

constexpr int CL_TILE = 256;           // rows per workgroup (score, tile counts, weights, adjoint)
constexpr int CL_HT = 1024;            // rows per workgroup of the histogram passes
constexpr int CL_LDS_FLOATS = 12288;   // 48 KiB of staged logits
constexpr int CL_MAX_C = 128;
constexpr int CL_MAX_N = 1 << 22;
constexpr int NB0 = 2048, NB1 = 2048, NB2 = 1024;   // score bits 31..21, 20..10, 9..0

enum { ST_NUM_POS = 0, ST_K, ST_BIN0, ST_KREM0, ST_BIN1, ST_KREM1, ST_T, ST_KREM, ST_NUM_NEG, ST_WORDS = 16 };

// workspace, in 32-bit words; [0, zero_words) is cleared by the first launch
struct ConfLayout {
    size_t st, hist0, hist1, hist2, npos, zero_words, cum, tilecnt, eqpre, keeppre, bits, ce, lse, w, part, words;
};

ConfLayout conf_layout(int B, int N)
{
    const size_t nT = (size_t)stm_cdiv(N, CL_TILE);
    ConfLayout L;
    size_t o = 0;
    L.st = o;      o += ST_WORDS;
    L.hist0 = o;   o += NB0;
    L.hist1 = o;   o += NB1;
    L.hist2 = o;   o += NB2;
    L.npos = o;    o += (size_t)B;
    L.zero_words = o;
    L.cum = o;     o += (size_t)B + 1;
    L.tilecnt = o; o += 4 * nT;
    L.eqpre = o;   o += nT;
    L.keeppre = o; o += nT;
    L.bits = o;    o += (size_t)N;
    L.ce = o;      o += (size_t)N;
    L.lse = o;     o += (size_t)N;
    L.w = o;       o += (size_t)N;
    o = (o + 1) & ~(size_t)1;          // the tile sums are doubles
    L.part = o;    o += 2 * nT;
    L.words = o;
    return L;
}


// (stm_block_excl_scan, stm_block_sum_f64: stm_common.h)

// The bin that holds the k-th largest key, walking the NB bins of hist from the top: `bin`, and krem = k minus the keys in higher bins (>= 1).
// k == 0 gives the top bin and krem = 0, which selects nothing further down.  Every workgroup that needs the answer computes it.
template <int NB>
__device__ __forceinline__ void radix_pick(const unsigned* __restrict__ hist, unsigned k, unsigned* sw, unsigned* sres, unsigned& bin, unsigned& krem)
{
    constexpr int PER = NB / 256;
    const int top = NB - 1 - (int)threadIdx.x * PER;
    unsigned c[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] = hist[top - j];
        s += c[j];
    }
    unsigned total;
    const unsigned above = stm_block_excl_scan(s, sw, total);
    if (threadIdx.x == 0) {
        sres[0] = NB - 1;
        sres[1] = 0;
    }
    __syncthreads();
    if (k >= 1 && above < k && k <= above + s) {         // one thread at most
        unsigned a = above;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (k <= a + c[j]) {
                sres[0] = (unsigned)(top - j);
                sres[1] = k - a;
                break;
            }
            a += c[j];
        }
    }
    __syncthreads();
    bin = sres[0];
    krem = sres[1];
}

__global__ __launch_bounds__(256) void ohem_zero_kernel(unsigned* __restrict__ p, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// stride: C made odd; R: rows staged at a time (a multiple of 64, R * stride <= CL_LDS_FLOATS)
__global__ __launch_bounds__(256) void ohem_score_kernel(const float* __restrict__ x, const int64_t* __restrict__ t, unsigned* __restrict__ bits,
                                                         float* __restrict__ ce, float* __restrict__ lse, unsigned* __restrict__ st,
                                                         unsigned* __restrict__ hist0, unsigned* __restrict__ npos, int N, int P, int C, int stride,
                                                         int R)
{
    __shared__ float sx[CL_LDS_FLOATS];
    __shared__ unsigned sh[NB0];
    const int tid = threadIdx.x;
    for (int i = tid; i < NB0; i += 256) sh[i] = 0u;
    const int row0 = blockIdx.x * CL_TILE;
    const int rows = min(CL_TILE, N - row0);
    for (int r0 = 0; r0 < rows; r0 += R) {
        const int nr = min(R, rows - r0);
        const int nelem = nr * C;
        const float* src = x + (int64_t)(row0 + r0) * C;     // 16-byte aligned: row0 + r0 is a multiple of 64
        __syncthreads();                                     // the previous rows are done with sx (and sh is cleared)
        for (int e = 4 * tid; e < nelem; e += 4 * 256) {
            int r = e / C, c = e - r * C;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (e + 3 < nelem) {
                const float4 q = *reinterpret_cast<const float4*>(src + e);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
                for (int j = 0; e + j < nelem; ++j) v[j] = src[e + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e + j < nelem) sx[r * stride + c] = v[j];
                if (++c == C) c = 0, ++r;
            }
        }
        __syncthreads();
        if (tid < nr) {
            const int row = row0 + r0 + tid;
            const float* p = sx + tid * stride;
            float m = p[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += exp((double)p[c] - (double)m);
            const double l = (double)m + log(s);
            const int64_t ti = t[row];
            float sc = 0.0f, cev = 0.0f;
            if (ti == 0) {
                sc = fmaxf((float)(l - (double)p[0]), 0.0f);
                cev = sc;
            } else if (ti > 0) {
                cev = ti < C ? (float)(l - (double)p[(int)ti]) : stm_nan_f32();
                atomicAdd(&npos[row / P], 1u);
                atomicAdd(&st[ST_NUM_POS], 1u);
            }
            const unsigned b = __builtin_bit_cast(unsigned, sc);
            lse[row] = (float)l;
            ce[row] = cev;
            bits[row] = b;
            atomicAdd(&sh[b >> 21], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < NB0; i += 256)
        if (sh[i]) atomicAdd(&hist0[i], sh[i]);
}

template <int LEVEL>
__global__ __launch_bounds__(256) void ohem_hist_kernel(const unsigned* __restrict__ bits, unsigned* __restrict__ st,
                                                        const unsigned* __restrict__ hprev, unsigned* __restrict__ hcur, int N, int ratio)
{
    __shared__ unsigned sh[2048];
    __shared__ unsigned sw[4], sres[2];
    const int tid = threadIdx.x;
    for (int i = tid; i < 2048; i += 256) sh[i] = 0u;
    unsigned k, bin, krem, pref;
    if (LEVEL == 1) {
        const unsigned long long kk = (unsigned long long)ratio * st[ST_NUM_POS];
        k = (unsigned)(kk < (unsigned long long)(N - 1) ? kk : (unsigned long long)(N - 1));
    } else {
        k = st[ST_KREM0];
    }
    radix_pick<2048>(hprev, k, sw, sres, bin, krem);         // (its barriers also publish the cleared sh)
    if (LEVEL == 1) {
        pref = bin;
        if (blockIdx.x == 0 && tid == 0) st[ST_K] = k, st[ST_BIN0] = bin, st[ST_KREM0] = krem;
    } else {
        pref = (st[ST_BIN0] << 11) | bin;
        if (blockIdx.x == 0 && tid == 0) st[ST_BIN1] = bin, st[ST_KREM1] = krem;
    }
    const int shift = LEVEL == 1 ? 21 : 10;
    const int end = min(N, (int)(blockIdx.x + 1) * CL_HT);
    for (int i = blockIdx.x * CL_HT + tid; i < end; i += 256) {
        const unsigned b = bits[i];
        if ((b >> shift) == pref) atomicAdd(&sh[LEVEL == 1 ? ((b >> 10) & 2047u) : (b & 1023u)], 1u);
    }
    __syncthreads();
    for (int i = tid; i < 2048; i += 256)
        if (sh[i]) atomicAdd(&hcur[i], sh[i]);
}

// per tile: {scores == T, true negatives with score == T, scores > T (all of them true negatives: a score above 0 has t == 0), positives}
__global__ __launch_bounds__(256) void ohem_tile_count_kernel(const unsigned* __restrict__ bits, const int64_t* __restrict__ t,
                                                              unsigned* __restrict__ st, const unsigned* __restrict__ hist2,
                                                              unsigned* __restrict__ tilecnt, int N)
{
    __shared__ unsigned sw[4], sres[2], sc[4][4];
    const int tid = threadIdx.x;
    unsigned bin, krem;
    radix_pick<NB2>(hist2, st[ST_KREM1], sw, sres, bin, krem);
    const unsigned T = (st[ST_BIN0] << 21) | (st[ST_BIN1] << 10) | bin;
    if (blockIdx.x == 0 && tid == 0) st[ST_T] = T, st[ST_KREM] = krem;
    const int row = blockIdx.x * CL_TILE + tid;
    const bool live = row < N;
    const unsigned b = live ? bits[row] : 0u;
    const int64_t ti = live ? t[row] : -1;
    const bool eq = live && b == T;
    const unsigned long long m0 = __ballot(eq), m1 = __ballot(eq && ti == 0), m2 = __ballot(live && b > T), m3 = __ballot(live && ti > 0);
    if ((tid & 63) == 0) {
        unsigned* d = sc[tid >> 6];
        d[0] = __popcll(m0), d[1] = __popcll(m1), d[2] = __popcll(m2), d[3] = __popcll(m3);
    }
    __syncthreads();
    if (tid < 4) tilecnt[(size_t)blockIdx.x * 4 + tid] = sc[0][tid] + sc[1][tid] + sc[2][tid] + sc[3][tid];
}

// one workgroup.  eqpre[i]: scores == T in the tiles before i; keeppre[i]: kept rows in the tiles before i; cum[b]: positives in the images before b.
__global__ __launch_bounds__(256) void ohem_scan_kernel(const unsigned* __restrict__ tilecnt, unsigned* __restrict__ eqpre,
                                                        unsigned* __restrict__ keeppre, const unsigned* __restrict__ npos,
                                                        unsigned* __restrict__ cum, unsigned* __restrict__ st, const unsigned* __restrict__ bits,
                                                        const int64_t* __restrict__ t, int N, int nT, int B)
{
    __shared__ unsigned sw[4], sres[2];
    const int tid = threadIdx.x;
    const unsigned T = st[ST_T], krem = st[ST_KREM];
    const int chunk = (nT + 255) / 256;
    const int lo = min(nT, tid * chunk), hi = min(nT, lo + chunk);
    unsigned s = 0, total;
    for (int i = lo; i < hi; ++i) s += tilecnt[4 * (size_t)i];
    const unsigned eq0 = stm_block_excl_scan(s, sw, total);
    if (tid == 0) sres[0] = 0xFFFFFFFFu, sres[1] = 0u;
    __syncthreads();
    unsigned a = eq0;
    for (int i = lo; i < hi; ++i) {
        const unsigned ceq = tilecnt[4 * (size_t)i];
        eqpre[i] = a;
        if (a < krem && a + ceq > krem) sres[0] = (unsigned)i, sres[1] = a;   // the one tile that is cut: some of its ties are taken, some are not
        a += ceq;
    }
    __syncthreads();
    const unsigned cut = sres[0], cut_pre = sres[1];
    unsigned cut_taken = 0;                                  // true negatives taken among the ties of the cut tile
    if (cut != 0xFFFFFFFFu) {                                // uniform
        const int row = (int)cut * CL_TILE + tid;
        const bool live = row < N;
        const bool eq = live && bits[row] == T;
        unsigned tot;
        const unsigned rank = cut_pre + stm_block_excl_scan(eq ? 1u : 0u, sw, tot);
        (void)stm_block_excl_scan((eq && rank < krem && t[row] == 0) ? 1u : 0u, sw, cut_taken);
    }
    s = 0;
    a = eq0;
    for (int i = lo; i < hi; ++i) {
        const unsigned* c = tilecnt + 4 * (size_t)i;
        s += c[3] + c[2] + (a + c[0] <= krem ? c[1] : (a >= krem ? 0u : cut_taken));
        a += c[0];
    }
    unsigned kept;
    unsigned kp = stm_block_excl_scan(s, sw, kept);
    a = eq0;
    for (int i = lo; i < hi; ++i) {
        const unsigned* c = tilecnt + 4 * (size_t)i;
        keeppre[i] = kp;
        kp += c[3] + c[2] + (a + c[0] <= krem ? c[1] : (a >= krem ? 0u : cut_taken));
        a += c[0];
    }
    if (tid == 0) st[ST_NUM_NEG] = kept - st[ST_NUM_POS];
    const int chb = (B + 255) / 256;
    const int blo = min(B, tid * chb), bhi = min(B, blo + chb);
    s = 0;
    for (int i = blo; i < bhi; ++i) s += npos[i];
    unsigned cp = stm_block_excl_scan(s, sw, total);
    for (int i = blo; i < bhi; ++i) {
        cum[i] = cp;
        cp += npos[i];
    }
    if (tid == 0) cum[B] = total;
}

// mode 0: the reference's positional weights; 1: aligned (every positive its own image's weight)
__global__ __launch_bounds__(256) void ohem_weights_kernel(const unsigned* __restrict__ bits, const int64_t* __restrict__ t,
                                                           const float* __restrict__ ce, const unsigned* __restrict__ st,
                                                           const unsigned* __restrict__ eqpre, const unsigned* __restrict__ keeppre,
                                                           const unsigned* __restrict__ npos, const unsigned* __restrict__ cum,
                                                           float* __restrict__ w, float* __restrict__ neg_out, double* __restrict__ part, int N,
                                                           int P, int B, int ratio, int mode)
{
    __shared__ unsigned sw[4];
    __shared__ double sd[4];
    const int tid = threadIdx.x;
    const int row = blockIdx.x * CL_TILE + tid;
    const bool live = row < N;
    const unsigned T = st[ST_T], krem = st[ST_KREM], num_pos = st[ST_NUM_POS], num_neg = st[ST_NUM_NEG];
    const unsigned b = live ? bits[row] : 0u;
    const int64_t ti = live ? t[row] : -1;
    const bool eq = live && b == T;
    unsigned tot;
    const unsigned er = eqpre[blockIdx.x] + stm_block_excl_scan(eq ? 1u : 0u, sw, tot);
    const bool pos = live && ti > 0;
    const bool neg = live && ti == 0 && (b > T || (eq && er < krem));
    const bool keep = pos || neg;
    const unsigned kr = keeppre[blockIdx.x] + stm_block_excl_scan(keep ? 1u : 0u, sw, tot);
    float wv = 0.0f;
    if (keep) {
        int img = -1;                                        // the image whose positive weight this row gets; -1: the negatives' weight
        if (mode == 1) {
            if (pos) img = row / P;
        } else if (kr < num_pos) {                           // the kr-th positive's image: cum[img] <= kr < cum[img + 1]
            int lo = 0, hi = B;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (cum[mid] <= kr) lo = mid;
                else hi = mid;
            }
            img = lo;
        }
        wv = img >= 0 ? (float)(1.0 / (double)max(npos[img], 1u)) : (float)((double)ratio * (double)B / (double)num_neg);
    }
    if (live) {
        w[row] = wv;
        if (neg_out) neg_out[row] = neg ? 1.0f : 0.0f;
    }
    const double term = keep ? (double)wv * (double)ce[row] : 0.0;
    const double sum = stm_block_sum_f64(term, sd);
    if (tid == 0) part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void ohem_reduce_kernel(const double* __restrict__ part, float* __restrict__ loss, int nT, double alpha, int ratio)
{
    __shared__ double sd[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nT; i += 256) s += part[i];
    s = stm_block_sum_f64(s, sd);
    if (threadIdx.x == 0) *loss = (float)(alpha * s / (double)(ratio + 1));
}

__global__ __launch_bounds__(256) void ohem_backward_kernel(const float* __restrict__ g, const float* __restrict__ x, const int64_t* __restrict__ t,
                                                            const float* __restrict__ lse, const float* __restrict__ w, float* __restrict__ gx,
                                                            int N, int C, float scale)
{
    __shared__ float s_w[CL_TILE], s_l[CL_TILE];
    __shared__ int s_t[CL_TILE];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * CL_TILE;
    const int rows = min(CL_TILE, N - row0);
    if (tid < rows) {
        const float wi = w[row0 + tid];
        s_w[tid] = wi;
        s_l[tid] = lse[row0 + tid];
        const int64_t ti = t[row0 + tid];
        s_t[tid] = (wi != 0.0f && ti < C) ? (int)ti : C;     // (a kept row has t >= 0); C marks a label that no class has
    }
    __syncthreads();
    const float gs = g[0] * scale;
    const int nelem = rows * C;
    const float* src = x + (int64_t)row0 * C;
    float* dst = gx + (int64_t)row0 * C;                     // 16-byte aligned: row0 is a multiple of 256
    for (int e = 4 * tid; e < nelem; e += 4 * 256) {
        int r = e / C, c = e - r * C;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0.0f;
            if (e + j < nelem) {
                const float wi = s_w[r];
                if (wi != 0.0f) {
                    const int ti = s_t[r];
                    v[j] = ti >= C ? stm_nan_f32() : gs * wi * (expf(src[e + j] - s_l[r]) - (c == ti ? 1.0f : 0.0f));
                }
            }
            if (++c == C) c = 0, ++r;
        }
        if (e + 3 < nelem) {
            *reinterpret_cast<float4*>(dst + e) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; e + j < nelem; ++j) dst[e + j] = v[j];
        }
    }
}

int conf_check(const char* who, int B, int P, int C, int ratio)
{
    STM_REQUIRE(B >= 1 && P >= 1 && ratio >= 1, STM_EINVAL, "%s: B=%d P=%d negpos_ratio=%d", who, B, P, ratio);
    STM_REQUIRE(C >= 2 && C <= CL_MAX_C, STM_EUNSUPPORTED, "%s: C=%d is outside [2, %d]", who, C, CL_MAX_C);
    STM_REQUIRE((int64_t)B * P <= CL_MAX_N, STM_EUNSUPPORTED, "%s: B*P=%lld > %d rows", who, (long long)B * P, CL_MAX_N);
    return STM_OK;
}

// launches 1-7; lse / w: where those two vectors go (the caller's tensors, or the workspace's own)
int conf_select(const char* who, const float* x, const int64_t* t, int B, int P, int C, int ratio, int mode, float* lse, float* w, float* neg_out,
                unsigned* ws, const ConfLayout& L, hipStream_t st)
{
    const int N = B * P, nT = stm_cdiv(N, CL_TILE), nH = stm_cdiv(N, CL_HT);
    const int stride = C | 1;
    const int fit = (CL_LDS_FLOATS / stride) & ~63;          // >= 64 for every C <= 128
    const int R = fit < CL_TILE ? fit : CL_TILE;
    unsigned* bits = ws + L.bits;
    float* ce = reinterpret_cast<float*>(ws + L.ce);
    hipLaunchKernelGGL(ohem_zero_kernel, dim3(stm_cdiv(L.zero_words, 256)), dim3(256), 0, st, ws, (int)L.zero_words);
    STM_CHECK_LAUNCH("ohem_zero_kernel");
    hipLaunchKernelGGL(ohem_score_kernel, dim3(nT), dim3(256), 0, st, x, t, bits, ce, lse, ws + L.st, ws + L.hist0, ws + L.npos, N, P, C, stride, R);
    STM_CHECK_LAUNCH("ohem_score_kernel");
    hipLaunchKernelGGL(ohem_hist_kernel<1>, dim3(nH), dim3(256), 0, st, bits, ws + L.st, ws + L.hist0, ws + L.hist1, N, ratio);
    STM_CHECK_LAUNCH("ohem_hist_kernel<1>");
    hipLaunchKernelGGL(ohem_hist_kernel<2>, dim3(nH), dim3(256), 0, st, bits, ws + L.st, ws + L.hist1, ws + L.hist2, N, ratio);
    STM_CHECK_LAUNCH("ohem_hist_kernel<2>");
    hipLaunchKernelGGL(ohem_tile_count_kernel, dim3(nT), dim3(256), 0, st, bits, t, ws + L.st, ws + L.hist2, ws + L.tilecnt, N);
    STM_CHECK_LAUNCH("ohem_tile_count_kernel");
    hipLaunchKernelGGL(ohem_scan_kernel, dim3(1), dim3(256), 0, st, ws + L.tilecnt, ws + L.eqpre, ws + L.keeppre, ws + L.npos, ws + L.cum,
                       ws + L.st, bits, t, N, nT, B);
    STM_CHECK_LAUNCH("ohem_scan_kernel");
    hipLaunchKernelGGL(ohem_weights_kernel, dim3(nT), dim3(256), 0, st, bits, t, ce, ws + L.st, ws + L.eqpre, ws + L.keeppre, ws + L.npos,
                       ws + L.cum, w, neg_out, reinterpret_cast<double*>(ws + L.part), N, P, B, ratio, mode);
    STM_CHECK_LAUNCH("ohem_weights_kernel");
    (void)who;
    return STM_OK;
}

}  // namespace

extern "C" size_t stm_ohem_conf_workspace_bytes(int B, int P, int C)
{
    (void)C;
    if (B <= 0 || P <= 0 || (int64_t)B * P > CL_MAX_N) return 64;
    return conf_layout(B, B * P).words * sizeof(unsigned) + 64;
}

extern "C" int stm_ohem_select_neg_f32(const float* conf, const int64_t* conf_t, float* neg, int B, int P, int C, int negpos_ratio, void* workspace,
                                       size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_ohem_select_neg_f32";
    const int rc = conf_check(who, B, P, C, negpos_ratio);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(conf && conf_t && neg, STM_ENULL, "%s: conf/conf_t/neg must be non-NULL", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_ohem_conf_workspace_bytes(B, P, C), STM_EWORKSPACE, "%s: workspace too small", who);
    STM_REQUIRE((uintptr_t)conf % 16 == 0 && (uintptr_t)workspace % 8 == 0, STM_EINVAL,
                "%s: conf must be 16-byte and the workspace 8-byte aligned", who);
    const ConfLayout L = conf_layout(B, B * P);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    return conf_select(who, conf, conf_t, B, P, C, negpos_ratio, 1, reinterpret_cast<float*>(ws + L.lse), reinterpret_cast<float*>(ws + L.w), neg, ws,
                       L, stm_hs(stream));
}

extern "C" int stm_ohem_conf_loss_f32(const float* conf, const int64_t* conf_t, float* loss, float* lse, float* w, int B, int P, int C,
                                      int negpos_ratio, double conf_alpha, int aligned_weights, void* workspace, size_t workspace_bytes,
                                      stm_stream_t stream)
{
    const char* who = "stm_ohem_conf_loss_f32";
    const int rc = conf_check(who, B, P, C, negpos_ratio);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(aligned_weights == 0 || aligned_weights == 1, STM_EINVAL, "%s: aligned_weights=%d", who, aligned_weights);
    STM_REQUIRE(conf && conf_t && loss && lse && w, STM_ENULL, "%s: conf/conf_t/loss/lse/w must be non-NULL", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_ohem_conf_workspace_bytes(B, P, C), STM_EWORKSPACE, "%s: workspace too small", who);
    STM_REQUIRE((uintptr_t)conf % 16 == 0 && (uintptr_t)workspace % 8 == 0, STM_EINVAL,
                "%s: conf must be 16-byte and the workspace 8-byte aligned", who);
    const int N = B * P;
    const ConfLayout L = conf_layout(B, N);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    hipStream_t st = stm_hs(stream);
    const int rs = conf_select(who, conf, conf_t, B, P, C, negpos_ratio, aligned_weights, lse, w, nullptr, ws, L, st);
    if (rs != STM_OK) return rs;
    hipLaunchKernelGGL(ohem_reduce_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const double*>(ws + L.part), loss, stm_cdiv(N, CL_TILE),
                       conf_alpha, negpos_ratio);
    STM_CHECK_LAUNCH("ohem_reduce_kernel");
    return STM_OK;
}

extern "C" int stm_ohem_conf_loss_backward_f32(const float* grad_loss, const float* conf, const int64_t* conf_t, const float* lse, const float* w,
                                               float* grad_conf, int B, int P, int C, int negpos_ratio, double conf_alpha, stm_stream_t stream)
{
    const char* who = "stm_ohem_conf_loss_backward_f32";
    const int rc = conf_check(who, B, P, C, negpos_ratio);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(grad_loss && conf && conf_t && lse && w && grad_conf, STM_ENULL, "%s: grad_loss/conf/conf_t/lse/w/grad_conf must be non-NULL", who);
    STM_REQUIRE((uintptr_t)grad_conf % 16 == 0, STM_EINVAL, "%s: grad_conf must be 16-byte aligned", who);
    const int N = B * P;
    hipLaunchKernelGGL(ohem_backward_kernel, dim3(stm_cdiv(N, CL_TILE)), dim3(256), 0, stm_hs(stream), grad_loss, conf, conf_t, lse, w, grad_conf, N,
                       C, (float)(conf_alpha / (double)(negpos_ratio + 1)));
    STM_CHECK_LAUNCH("ohem_backward_kernel");
    return STM_OK;
}
