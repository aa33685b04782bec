// det_accum.h -- order-independent accumulation for the scatters of the deterministic backward (det_backward.hip), gfx950 (MI355X).
//
// A scatter whose destinations collide cannot fix the order in which its terms arrive, so the sum itself is made associative: every fp32 term
// t_i is rounded once to a multiple of 2^-p and added as a 64-bit integer,
//     grad = fp32( (sum_i rint(t_i * 2^p)) / 2^p ).
// Integer addition is exact, so the result does not depend on arrival order, grid shape or channel chunking.  What has to hold is that no
// destination's integer sum leaves int64, and every thread must derive the same p:
//
//   * M is a power of two that no |t_i| exceeds: 2^E with E = ceil(log2 a) + ceil(log2 b), a = max |gradient| and b = max |mask| (1 where the
//     mask is a sigmoid or absent), both taken as bit patterns by a pass over the inputs.  A term is fl(w * fl(m * v))-like with a weight
//     w <= 1: rounding is monotone, so |t_i| <= fl(a * b) <= 2^E also after every rounding; an a * b that overflows fp32 counts as not finite.
//   * mass_bound bounds, from the shapes alone, sum_i |t_i| / M over the terms of one destination; terms_bound their number.  Then
//         |sum_i rint(t_i 2^p)| <= sum_i (|t_i| 2^p + 1/2) <= mass_bound * 2^(E + p) + terms_bound / 2,
//     and q = E + p is the largest integer with  mass_bound * 2^q + terms_bound / 2 < 2^62:  2^(q+1) <= (2^63 - 1 - terms_bound) / mass_bound.
//     q depends on the shapes only -- it is the number of bits between the bound of the maximum and the fixed-point unit -- so the host computes
//     it, refuses q < STM_DET_MIN_BITS before any launch, and hands it to the kernels; p = q - E is derived on the device from the two words.
//
// Error: each term is off by at most 2^-(p+1) = M * 2^-(q+1), a destination of L terms by L times that, plus the one final rounding to fp32.
// Everything here is plain C++ shared by host and device; the host half is what stm_det_exponent (det_backward.h) exports.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STM_DET_HD __host__ __device__ __forceinline__
#else
#define STM_DET_HD static inline
#endif

#define STM_DET_MIN_BITS 36

// what the two words say about the scatter's inputs
#define STM_DET_FINITE 0     // accumulate with the exponent p
#define STM_DET_ZERO 1       // a maximum of zero: every term is zero, the output is exact zeros
#define STM_DET_NONFINITE 2  // an inf or NaN among the inputs, or maxima whose product overflows fp32: the whole output is NaN

// ceil(log2 v) of the positive finite fp32 value with these bits (sign bit clear): 2^result >= v, with equality for a power of two
STM_DET_HD int stm_det_ceil_log2(uint32_t bits)
{
    const int e = (int)(bits >> 23);
    const uint32_t m = bits & 0x7FFFFFu;
    if (e == 0) {                                   // subnormal: v = m * 2^-149, m >= 1
        int top = 0;
        while ((m >> top) > 1u) ++top;              // floor(log2 m)
        return top + ((m & (m - 1u)) ? 1 : 0) - 149;
    }
    return e - 127 + (m ? 1 : 0);
}

// q of the header comment, or -1 when the bounds are not usable (mass_bound < 1, terms_bound < 0) or leave no exponent at all
STM_DET_HD int stm_det_shape_bits(int64_t terms_bound, int64_t mass_bound)
{
    if (mass_bound < 1 || terms_bound < 0) return -1;
    const uint64_t lim = (uint64_t)(INT64_MAX - terms_bound) / (uint64_t)mass_bound;   // 2^(q+1) <= lim
    if (lim < 2) return -1;
    int top = 0;
    while ((lim >> top) > 1u) ++top;                // floor(log2 lim)
    return top - 1;
}

// state of the two words, and p = q - E for STM_DET_FINITE
STM_DET_HD int stm_det_state(uint32_t bits_a, uint32_t bits_b, int q, int* p)
{
    *p = 0;
    if (bits_a >= 0x7F800000u || bits_b >= 0x7F800000u) return STM_DET_NONFINITE;
    if (bits_a == 0u || bits_b == 0u) return STM_DET_ZERO;
    float a, b;
    memcpy(&a, &bits_a, 4);
    memcpy(&b, &bits_b, 4);
    const float ab = a * b;                         // the largest product a term can be: one IEEE multiplication, the same on host and device
    if (!(ab <= 3.402823466e+38f)) return STM_DET_NONFINITE;
    *p = q - (stm_det_ceil_log2(bits_a) + stm_det_ceil_log2(bits_b));
    return STM_DET_FINITE;
}

#if defined(__HIPCC__)
// 2^p as a double, -1022 <= p <= 1023 (q <= 62 and -298 <= E <= 129 keep p inside [36 - 129, 62 + 298])
__device__ __forceinline__ double stm_det_pow2(int p) { return __longlong_as_double((long long)(p + 1023) << 52); }

// rint(t * 2^p): the scaling is exact in double, the rounding is to nearest even, and |result| <= 2^q
__device__ __forceinline__ long long stm_det_fix(float t, double two_p) { return (long long)rint((double)t * two_p); }

__device__ __forceinline__ void stm_det_add(long long* acc, float t, double two_p)
{
    const long long v = stm_det_fix(t, two_p);
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);   // two's complement: the unsigned add is the signed one
}
#endif
