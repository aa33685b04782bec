/* chunk_table.h -- rows of unequal length cut into chunks, one workgroup per chunk (internal: optim.hip and fold.hip; optim.h, dp_step.h and
 * fold.h take their constants from here).  A launch's table of at most STM_CHUNK_MAX_ROWS rows travels by value in the kernel arguments; beside
 * what the kernel needs of a row it holds `n[i]`, the row's element count, `first[i]`, the index of the row's first chunk among the chunks of the
 * launch, and `count`, the number of rows.  Workgroup b finds its row by a binary search over `first` (wave-uniform: scalar loads from the kernel
 * arguments). */
#pragma once

#define STM_CHUNK_ELEMS 4096    /* elements of a chunk */
#define STM_CHUNK_MAX_ROWS 64   /* rows of a table */

#ifdef __HIPCC__
#include "stm_common.h"

__device__ __forceinline__ bool stm_nonfinite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// the row of chunk b: the last i with first[i] <= b (rows without elements share their first chunk with the next one and are passed over)
template <class Table>
__device__ __forceinline__ int stm_chunk_find(const Table& t, int b)
{
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// chunk b -> its row (returned), the index `base` of the chunk's first element in the row and the chunk's element count.  Index: int where a row
// holds fewer than 2^31 elements, int64_t otherwise.
template <class Table, class Index>
__device__ __forceinline__ int stm_chunk_of(const Table& t, int b, Index& base, int& cnt)
{
    const int ti = stm_chunk_find(t, b);
    base = (Index)(b - t.first[ti]) * STM_CHUNK_ELEMS;
    const Index left = t.n[ti] - base;
    cnt = left < STM_CHUNK_ELEMS ? (int)left : STM_CHUNK_ELEMS;
    return ti;
}

// host: row k of n elements starts at the chunk count so far, which then grows by the row's chunks
inline int stm_chunk_append(const char* who, int* first, int k, int64_t n, int64_t& chunks)
{
    first[k] = (int)chunks;
    chunks += (n + STM_CHUNK_ELEMS - 1) / STM_CHUNK_ELEMS;
    STM_REQUIRE(chunks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: 2^31 chunks of %d elements or more in one call", who, STM_CHUNK_ELEMS);
    return STM_OK;
}
#endif
