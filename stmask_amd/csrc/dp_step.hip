// dp_step.hip -- the finish of a data-parallel training step for gfx950 (MI355X), csrc/dp_step.h (package-private, stmask_amd/optim.py).
//
//   stm_dp_sgd_finish_multi_f32   the step of optim.hip over the all-reduced gradient arena: the summed gradient times 1 / world, weight decay,
//                                 momentum and the parameter write of up to STM_DP_MAX_TENSORS tensors in one launch and one pass, and 0.0f
//                                 written back over every gradient element read: 12 bytes read and 12 written per element, no LDS.  The guard
//                                 (reduced loss sum finite, bad == 0) is read by every workgroup first; a skipped step still clears its
//                                 gradients (4 bytes written per element, nothing read).
//
// The table, the chunking and the two access widths are optim.hip's: a workgroup owns one chunk of STM_DP_CHUNK elements and finds its tensor by
// a binary search over the first-chunk prefix; a chunk whose three addresses are 16-byte aligned goes through float4 accesses, four per thread
// with all twelve loads issued before the arithmetic; the zeros go out first (they depend on no load), then m, then p.
// Compiled with -ffp-contract=off: the four expressions stay four multiplies and three adds in the stated order.
#include "stm_common.h"
#include "dp_step.h"

namespace {

constexpr int DP_T = STM_DP_MAX_TENSORS;
constexpr int DP_CHUNK = STM_DP_CHUNK;
constexpr int DP_THREADS = 256;
constexpr int DP_VEC_PER_THREAD = DP_CHUNK / 4 / DP_THREADS;
static_assert(DP_CHUNK % (4 * DP_THREADS) == 0, "a chunk is a whole number of float4 per thread");

struct DpTable {
    float* p[DP_T];
    float* g[DP_T];
    float* m[DP_T];
    int64_t n[DP_T];
    int first[DP_T];      // index of the tensor's first chunk among the chunks of this launch
    int count;
};
static_assert(sizeof(DpTable) + 64 < 4096, "the table travels in the kernel arguments");

__device__ __forceinline__ bool dp_nonfinite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// the tensor of chunk b: the last i with first[i] <= b (tensors without elements share their first chunk with the next one and are passed over)
__device__ __forceinline__ int dp_find(const DpTable& t, int b)
{
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void dp_update(float& p, float s, float& m, float inv_world, float lr, float mu, float wd)
{
    const float g = s * inv_world;
    const float g1 = g + wd * p;
    m = mu * m + g1;
    p = p - lr * m;
}

__global__ __launch_bounds__(DP_THREADS) void dp_sgd_finish_multi_kernel(const DpTable t, int total_chunks, const float* loss_sum,
                                                                         const int* __restrict__ bad, int* __restrict__ counters, int first_launch,
                                                                         float inv_world, float lr, float mu, float wd)
{
    bool skip = false;
    if (loss_sum) skip = dp_nonfinite(loss_sum[0]);
    if (bad) skip = skip || bad[0] != 0;
    if (first_launch && blockIdx.x == 0 && threadIdx.x == 0) {
        const int slot = skip ? 1 : 0;
        const int seen = counters[slot];
        counters[slot] = seen + 1;
    }
    const int b = blockIdx.x;
    if (b >= total_chunks) return;
    const int ti = dp_find(t, b);
    const int64_t base = (int64_t)(b - t.first[ti]) * DP_CHUNK;
    const int64_t left = t.n[ti] - base;
    const int cnt = left < DP_CHUNK ? (int)left : DP_CHUNK;
    float* __restrict__ g = t.g[ti] + base;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (skip) {                      // nothing is read: p and m stay as they are, the gradients are cleared
        const int nz = ((uintptr_t)g & 15) == 0 ? cnt >> 2 : 0;
        for (int i = threadIdx.x; i < nz; i += DP_THREADS) reinterpret_cast<float4*>(g)[i] = zero4;
        for (int i = nz * 4 + threadIdx.x; i < cnt; i += DP_THREADS) g[i] = 0.0f;
        return;
    }
    float* __restrict__ p = t.p[ti] + base;
    float* __restrict__ m = t.m[ti] + base;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
    const int nvec = vec ? cnt >> 2 : 0;
    if (nvec == DP_CHUNK / 4) {
        float4 pv[DP_VEC_PER_THREAD], gv[DP_VEC_PER_THREAD], mv[DP_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < DP_VEC_PER_THREAD; ++k) {
            const int i = k * DP_THREADS + threadIdx.x;
            pv[k] = reinterpret_cast<const float4*>(p)[i];
            gv[k] = reinterpret_cast<const float4*>(g)[i];
            mv[k] = reinterpret_cast<const float4*>(m)[i];
        }
#pragma unroll
        for (int k = 0; k < DP_VEC_PER_THREAD; ++k) {
            const int i = k * DP_THREADS + threadIdx.x;
            dp_update(pv[k].x, gv[k].x, mv[k].x, inv_world, lr, mu, wd);
            dp_update(pv[k].y, gv[k].y, mv[k].y, inv_world, lr, mu, wd);
            dp_update(pv[k].z, gv[k].z, mv[k].z, inv_world, lr, mu, wd);
            dp_update(pv[k].w, gv[k].w, mv[k].w, inv_world, lr, mu, wd);
            reinterpret_cast<float4*>(g)[i] = zero4;
            reinterpret_cast<float4*>(m)[i] = mv[k];
            reinterpret_cast<float4*>(p)[i] = pv[k];
        }
        return;
    }
    for (int i = threadIdx.x; i < nvec; i += DP_THREADS) {
        float4 pv = reinterpret_cast<const float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<const float4*>(m)[i];
        dp_update(pv.x, gv.x, mv.x, inv_world, lr, mu, wd);
        dp_update(pv.y, gv.y, mv.y, inv_world, lr, mu, wd);
        dp_update(pv.z, gv.z, mv.z, inv_world, lr, mu, wd);
        dp_update(pv.w, gv.w, mv.w, inv_world, lr, mu, wd);
        reinterpret_cast<float4*>(g)[i] = zero4;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(p)[i] = pv;
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += DP_THREADS) {
        float pv = p[i], mv = m[i];
        dp_update(pv, g[i], mv, inv_world, lr, mu, wd);
        g[i] = 0.0f;
        m[i] = mv;
        p[i] = pv;
    }
}

int dp_fill_table(const char* who, DpTable& t, int& total_chunks, float* const* p, float* const* g, float* const* m, const int64_t* n, int count)
{
    STM_REQUIRE(count >= 1, STM_EINVAL, "%s: count=%d, at least one tensor is needed", who, count);
    STM_REQUIRE(count <= DP_T, STM_EUNSUPPORTED, "%s: count=%d, one call takes at most %d tensors", who, count, DP_T);
    STM_REQUIRE(p && g && m && n, STM_EINVAL, "%s: the arrays of pointers and element counts must be non-NULL", who);
    memset(&t, 0, sizeof(t));
    int64_t chunks = 0;
    for (int i = 0; i < count; ++i) {
        STM_REQUIRE(n[i] >= 0, STM_EINVAL, "%s: tensor %d has n=%lld elements", who, i, (long long)n[i]);
        STM_REQUIRE(n[i] == 0 || (g[i] && p[i] && m[i]), STM_EINVAL, "%s: tensor %d has %lld elements and a NULL %s", who, i, (long long)n[i],
                    !g[i] ? "g" : !p[i] ? "p" : "m");
        t.p[i] = p[i];
        t.g[i] = g[i];
        t.m[i] = m[i];
        t.n[i] = n[i];
        t.first[i] = (int)chunks;
        chunks += (n[i] + DP_CHUNK - 1) / DP_CHUNK;
        STM_REQUIRE(chunks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: 2^31 chunks of %d elements or more in one call", who, DP_CHUNK);
    }
    t.count = count;
    total_chunks = (int)chunks;
    return STM_OK;
}

}  // namespace

extern "C" int stm_dp_sgd_finish_multi_f32(float* const* p, float* const* g, float* const* m, const int64_t* n, int count, const float* loss_sum,
                                           const int* bad, int* counters, int first_launch, float inv_world, float lr, float mu, float wd,
                                           stm_stream_t stream)
{
    const char* who = "stm_dp_sgd_finish_multi_f32";
    DpTable t;
    int total_chunks = 0;
    const int rc = dp_fill_table(who, t, total_chunks, p, g, m, n, count);
    if (rc) return rc;
    STM_REQUIRE(lr - lr == 0.0f && mu - mu == 0.0f && wd - wd == 0.0f, STM_EINVAL, "%s: lr=%g mu=%g wd=%g must be finite", who, (double)lr, (double)mu,
                (double)wd);
    STM_REQUIRE(inv_world > 0.0f && inv_world <= 1.0f, STM_EINVAL, "%s: inv_world=%g must lie in (0, 1]", who, (double)inv_world);
    STM_REQUIRE(counters, STM_EINVAL, "%s: counters must be non-NULL", who);
    if (total_chunks == 0 && !first_launch) return STM_OK;
    // a step over tensors without elements still counts: one workgroup for the counter
    hipLaunchKernelGGL(dp_sgd_finish_multi_kernel, dim3((unsigned)(total_chunks > 0 ? total_chunks : 1)), dim3(DP_THREADS), 0, stm_hs(stream), t,
                       total_chunks, loss_sum, bad, counters, first_launch, inv_world, lr, mu, wd);
    STM_CHECK_LAUNCH("dp_sgd_finish_multi_kernel");
    return STM_OK;
}
