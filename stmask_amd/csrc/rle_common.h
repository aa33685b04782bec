// rle_common.h -- the run-length arithmetic the two output stages share (output.hip: one frame size per call; output_batch.hip: every row with
// its own frame's size): run extraction from column-major bit words, and pycocotools' rleToString character rule.
#pragma once
#include "stm_common.h"

// bits of word w that are real pixels (the last word is zero-padded: a 1 -> padding "transition" is not a run boundary)
__device__ __forceinline__ unsigned long long stm_rle_valid_bits(int w, int64_t n_px)
{
    const int64_t rem = n_px - (int64_t)w * 64;
    return rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
}

// One workgroup of 1024 threads, one mask: bw[0..words) bit words of n_px pixels -> cnt[0..min(runs, max_runs)) run lengths, T scratch of
// max_runs transition positions; returns the true number of runs (every thread gets it).  Transitions are the set bits of
// w ^ ((w << 1) | carry); per-word popcounts are prefix-summed across the workgroup, every thread then emits its words' transition positions
// in order and the counts are the first differences.  wave_tot: 16 ints of LDS.  Has barriers: call it uniformly.
__device__ __forceinline__ int stm_rle_runs_block(const unsigned long long* __restrict__ bw, int words, int64_t n_px, unsigned int* __restrict__ T,
                                                  unsigned int* __restrict__ cnt, int max_runs, int* wave_tot)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int per = (words + 1023) / 1024;                // consecutive words per thread
    const int w0 = min(words, tid * per), w1 = min(words, w0 + per);
    // pass 1: transitions in my words
    int mine = 0;
    for (int w = w0; w < w1; ++w) {
        const unsigned long long cur = bw[w];
        const unsigned long long prev = w ? (bw[w - 1] >> 63) : 0ull;
        mine += __popcll((cur ^ ((cur << 1) | prev)) & stm_rle_valid_bits(w, n_px));
    }
    // exclusive scan over the 1024 threads (wave scan + wave totals)
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) base += wave_tot[w];
        total += wave_tot[w];
    }
    int pos = base + incl - mine;
    // pass 2: emit transition positions in order
    for (int w = w0; w < w1; ++w) {
        const unsigned long long cur = bw[w];
        const unsigned long long prev = w ? (bw[w - 1] >> 63) : 0ull;
        unsigned long long d = (cur ^ ((cur << 1) | prev)) & stm_rle_valid_bits(w, n_px);
        while (d) {
            const int b = __ffsll((long long)d) - 1;
            if (pos < max_runs) T[pos] = (unsigned int)(w * 64 + b);
            ++pos;
            d &= d - 1;
        }
    }
    __threadfence_block();
    __syncthreads();
    // counts[j] = T[j] - T[j-1] (T[-1] = 0); last count = n_px - T[last]
    const int nr = total + 1;
    for (int j = tid; j < min(nr, max_runs); j += 1024) {
        const unsigned int hi = (j < total) ? T[j] : (unsigned int)n_px;
        const unsigned int lo = j ? T[j - 1] : 0u;
        cnt[j] = hi - lo;
    }
    return nr;
}

// pycocotools maskApi.c rleToString, one run: the value written for run j is c[j] - (j > 2 ? c[j - 2] : 0) ...
__device__ __forceinline__ long long stm_rle_value(const unsigned int* __restrict__ c, int j)
{
    long long x = (long long)c[j];
    if (j > 2) x -= (long long)c[j - 2];
    return x;
}

// ... as 5-bit groups, low group first, bit 5 = "more follows", the last group carrying the sign in its bit 4; + 48 makes them printable.
// |x| < 2^32 takes at most 7 groups.  Writes the characters to `out` when it is non-null; returns how many there are.
__device__ __forceinline__ int stm_rle_chars(long long x, unsigned char* out)
{
    int n = 0;
    bool more = true;
#pragma unroll 1
    for (int k = 0; k < 13 && more; ++k) {               // 13 groups cover 64 bits: the loop is bounded whatever x is
        int ch = (int)(x & 0x1f);
        x >>= 5;
        more = (ch & 0x10) ? x != -1 : x != 0;
        if (more) ch |= 0x20;
        if (out) out[n] = (unsigned char)(ch + 48);
        ++n;
    }
    return n;
}
