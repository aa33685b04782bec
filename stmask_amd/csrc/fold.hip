// fold.hip -- the inference twin's parameter write for gfx950 (MI355X), csrc/fold.h (package-private, stmask_amd/validate.py).
//
//   stm_fold_rows_f32   up to STM_FOLD_MAX_ROWS tensors of the twin written from the live net's in one launch: plain copies, convolution weights
//                       with their BatchNorm's scale folded in, biases with its shift.  4 bytes read and 4 written per element, plus the
//                       BatchNorm vectors (cached: a channel's four values serve `inner` elements); no LDS, no second pass.
//
// The table is a kernel argument (FoldTable, ~3.8 KB): six pointers a row, element counts, channel lengths and the index of each row's first chunk.
// A workgroup owns one chunk of STM_FOLD_CHUNK elements and finds its row as csrc/optim.hip does (chunk_table.h).  The kind of a row is told by
// the pointers it carries (no var: copy; var and no mean: weight; mean: bias), so the table needs no word for it.  The scale s = gamma / sqrt(var + eps) is recomputed whenever a thread's run of
// elements enters another channel: two cached loads, one sqrt and one division against a scratch buffer of scales and a pass to fill it.
// Compiled with -ffp-contract=off and without fast-math; the division is the `/` operator and the square root sqrtf(), which hipcc expands to their
// correctly rounded forms (HIP's __fsqrt_rn is the hardware's 1-ulp v_sqrt_f32 here: measured, one channel in ten differed): every operation is
// rounded once, as torch's CPU kernels do.
#include "stm_common.h"
#include "chunk_table.h"
#include "fold.h"

namespace {

constexpr int FOLD_T = STM_FOLD_MAX_ROWS;
constexpr int FOLD_THREADS = 256;

struct FoldTable {
    float* dst[FOLD_T];
    const float* src[FOLD_T];
    const float* gamma[FOLD_T];
    const float* beta[FOLD_T];
    const float* mean[FOLD_T];
    const float* var[FOLD_T];
    int n[FOLD_T];
    int inner[FOLD_T];
    int first[FOLD_T];      // index of the row's first chunk among the chunks of this launch
    int count;
};
static_assert(sizeof(FoldTable) + 64 < 4096, "the table travels in the kernel arguments");

__device__ __forceinline__ float fold_scale(const float* __restrict__ gamma, const float* __restrict__ var, int c, float eps)
{
    return gamma[c] / sqrtf(var[c] + eps);
}

// One row kind over one chunk.  KIND 0: copy, 1: weight, 2: bias.  `e0` is the index of the chunk's first element in its tensor.
template <int KIND>
__device__ __forceinline__ void fold_chunk(float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var, int e0,
                                           int cnt, int inner, float eps)
{
    const bool vec = (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;      // a NULL src (bias of a convolution without one) is no obstacle
    const int nvec = vec ? cnt >> 2 : 0;
    for (int i = threadIdx.x; i < nvec; i += FOLD_THREADS) {
        float4 v = src ? reinterpret_cast<const float4*>(src)[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (KIND != 0) {
            const unsigned e = (unsigned)(e0 + 4 * i);
            int c = (int)(e / (unsigned)inner);
            int r = (int)(e - (unsigned)c * (unsigned)inner);
            float x[4] = {v.x, v.y, v.z, v.w};
            float s = fold_scale(gamma, var, c, eps);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (KIND == 1) {
                    x[j] = x[j] * s;
                } else {
                    const float d = x[j] - mean[c];
                    const float p = d * s;
                    x[j] = p + beta[c];
                }
                if (j < 3 && ++r == inner) {        // the next element opens the next channel (it exists: 4 i + j + 1 < cnt)
                    r = 0;
                    ++c;
                    s = fold_scale(gamma, var, c, eps);
                }
            }
            v = make_float4(x[0], x[1], x[2], x[3]);
        }
        reinterpret_cast<float4*>(dst)[i] = v;
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += FOLD_THREADS) {
        float x = src ? src[i] : 0.0f;
        if (KIND != 0) {
            const int c = (int)((unsigned)(e0 + i) / (unsigned)inner);
            const float s = fold_scale(gamma, var, c, eps);
            if (KIND == 1) {
                x = x * s;
            } else {
                const float d = x - mean[c];
                const float p = d * s;
                x = p + beta[c];
            }
        }
        dst[i] = x;
    }
}

__global__ __launch_bounds__(FOLD_THREADS) void fold_rows_kernel(const FoldTable t, int total_chunks, float eps)
{
    const int b = blockIdx.x;
    if (b >= total_chunks) return;
    int e0, cnt;                                             // e0 < n < 2^31
    const int ti = stm_chunk_of(t, b, e0, cnt);
    float* dst = t.dst[ti] + e0;
    const float* src = t.src[ti] ? t.src[ti] + e0 : nullptr;
    const float* var = t.var[ti];
    const float* mean = t.mean[ti];
    if (!var) fold_chunk<0>(dst, src, nullptr, nullptr, nullptr, nullptr, e0, cnt, 1, eps);
    else if (!mean) fold_chunk<1>(dst, src, t.gamma[ti], nullptr, nullptr, var, e0, cnt, t.inner[ti], eps);
    else fold_chunk<2>(dst, src, t.gamma[ti], t.beta[ti], mean, var, e0, cnt, t.inner[ti], eps);
}

int fold_check_row(const char* who, const stm_fold_row& r, int i)
{
    STM_REQUIRE(r.numel >= 0, STM_EINVAL, "%s: row %d has numel=%lld", who, i, (long long)r.numel);
    STM_REQUIRE(r.numel < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: row %d has numel=%lld, a row holds fewer than 2^31 elements", who, i,
                (long long)r.numel);
    STM_REQUIRE(r.kind == STM_FOLD_COPY || r.kind == STM_FOLD_WEIGHT || r.kind == STM_FOLD_BIAS, STM_EINVAL, "%s: row %d has kind=%d", who, i,
                r.kind);
    if (r.numel == 0) return STM_OK;
    STM_REQUIRE(r.dst, STM_EINVAL, "%s: row %d has %lld elements and a NULL dst", who, i, (long long)r.numel);
    STM_REQUIRE(r.src || r.kind == STM_FOLD_BIAS, STM_EINVAL, "%s: row %d has %lld elements and a NULL src", who, i, (long long)r.numel);
    if (r.kind == STM_FOLD_COPY) return STM_OK;
    STM_REQUIRE(r.gamma && r.var && (r.kind == STM_FOLD_WEIGHT || (r.beta && r.mean)), STM_EINVAL,
                "%s: row %d (kind %d) has a NULL BatchNorm pointer among those it reads", who, i, r.kind);
    STM_REQUIRE(r.inner >= 1 && r.numel % r.inner == 0, STM_EINVAL, "%s: row %d has numel=%lld and inner=%lld, whole channels are needed", who, i,
                (long long)r.numel, (long long)r.inner);
    return STM_OK;
}

}  // namespace

extern "C" size_t stm_fold_struct_bytes(int which)
{
    return which == 0 ? sizeof(stm_fold_row) : 0;
}

extern "C" int stm_fold_rows_f32(const stm_fold_row* rows, int count, stm_stream_t stream)
{
    const char* who = "stm_fold_rows_f32";
    STM_REQUIRE(count >= 0, STM_EINVAL, "%s: count=%d", who, count);
    STM_REQUIRE(count <= FOLD_T, STM_EUNSUPPORTED, "%s: count=%d, one call takes at most %d rows", who, count, FOLD_T);
    if (count == 0) return STM_OK;
    STM_REQUIRE(rows, STM_EINVAL, "%s: rows must be non-NULL", who);
    for (int i = 0; i < count; ++i) {
        const int rc = fold_check_row(who, rows[i], i);
        if (rc) return rc;
    }
    // consecutive rows of one eps (compared as bits; a copy has none and joins either side) share a launch
    int begin = 0;
    while (begin < count) {
        FoldTable t;
        memset(&t, 0, sizeof(t));
        bool have_eps = false;
        float eps = 0.0f;
        int64_t chunks = 0;
        int end = begin;
        for (; end < count; ++end) {
            const stm_fold_row& r = rows[end];
            if (r.kind != STM_FOLD_COPY && r.numel > 0) {
                if (have_eps && memcmp(&eps, &r.eps, sizeof(float)) != 0) break;
                eps = r.eps;
                have_eps = true;
            }
            const int k = end - begin;
            const bool fold = r.kind != STM_FOLD_COPY;
            const bool bias = r.kind == STM_FOLD_BIAS;
            t.dst[k] = r.dst;
            t.src[k] = r.src;
            t.gamma[k] = fold ? r.gamma : nullptr;
            t.var[k] = fold ? r.var : nullptr;
            t.beta[k] = bias ? r.beta : nullptr;
            t.mean[k] = bias ? r.mean : nullptr;
            t.n[k] = (int)r.numel;
            t.inner[k] = fold && r.numel > 0 ? (int)r.inner : 1;
            const int rc = stm_chunk_append(who, t.first, k, r.numel, chunks);
            if (rc) return rc;
        }
        t.count = end - begin;
        begin = end;
        if (chunks == 0) continue;
        hipLaunchKernelGGL(fold_rows_kernel, dim3((unsigned)chunks), dim3(FOLD_THREADS), 0, stm_hs(stream), t, (int)chunks, eps);
        STM_CHECK_LAUNCH("fold_rows_kernel");
    }
    return STM_OK;
}
