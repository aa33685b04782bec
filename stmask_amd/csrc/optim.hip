// optim.hip -- the guarded, fused SGD step of the training loop for gfx950 (MI355X), csrc/optim.h (package-private, stmask_amd/optim.py).
//
//   stm_sgd_step_multi_f32         weight decay, momentum and the parameter write of up to STM_OPTIM_MAX_TENSORS tensors in one launch and one
//                                  pass: 12 bytes read and 8 written per element, no LDS.  The guard (loss finite, bad == 0) is read by every
//                                  workgroup before it touches anything, so a skipped step costs a launch of workgroups that return at once and
//                                  the host never waits for the verdict.
//   stm_grads_nonfinite_multi_f32  the same table over the gradients alone: any NaN / inf sets bad[0].
//
// The tensor table is a kernel argument (OptimTable, ~2.3 KB): pointers, element counts and the index of each tensor's first chunk.  A workgroup
// owns one chunk of STM_OPTIM_CHUNK elements and finds its tensor by a binary search over the first-chunk prefix (wave-uniform: scalar loads from
// the kernel arguments).  A chunk whose three addresses are 16-byte aligned goes through float4 loads and stores, four per thread with all loads
// issued before the arithmetic; its last n % 4 elements, and every chunk of a tensor whose storage starts at an odd offset, take the 4-byte path.
// Compiled with -ffp-contract=off: the three expressions stay three multiplies and three adds in the stated order.
#include "stm_common.h"
#include "optim.h"

namespace {

constexpr int OPT_T = STM_OPTIM_MAX_TENSORS;
constexpr int OPT_CHUNK = STM_OPTIM_CHUNK;
constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC_PER_THREAD = OPT_CHUNK / 4 / OPT_THREADS;
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is a whole number of float4 per thread");

struct OptimTable {
    float* p[OPT_T];
    const float* g[OPT_T];
    float* m[OPT_T];
    int64_t n[OPT_T];
    int first[OPT_T];      // index of the tensor's first chunk among the chunks of this launch
    int count;
};
static_assert(sizeof(OptimTable) + 64 < 4096, "the table travels in the kernel arguments");

__device__ __forceinline__ bool opt_nonfinite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// the tensor of chunk b: the last i with first[i] <= b (tensors without elements share their first chunk with the next one and are passed over)
__device__ __forceinline__ int opt_find(const OptimTable& t, int b)
{
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void opt_update(float& p, float g, float& m, float lr, float mu, float wd)
{
    const float g1 = g + wd * p;
    m = mu * m + g1;
    p = p - lr * m;
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_step_multi_kernel(const OptimTable t, int total_chunks, const float* __restrict__ loss,
                                                                     const int* __restrict__ bad, int* __restrict__ counters, int first_launch,
                                                                     float lr, float mu, float wd)
{
    bool skip = false;
    if (loss) skip = opt_nonfinite(loss[0]);
    if (bad) skip = skip || bad[0] != 0;
    if (first_launch && blockIdx.x == 0 && threadIdx.x == 0) {
        const int slot = skip ? 1 : 0;
        const int seen = counters[slot];
        counters[slot] = seen + 1;
    }
    const int b = blockIdx.x;
    if (skip || b >= total_chunks) return;
    const int ti = opt_find(t, b);
    const int64_t base = (int64_t)(b - t.first[ti]) * OPT_CHUNK;
    const int64_t left = t.n[ti] - base;
    const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    float* __restrict__ p = t.p[ti] + base;
    const float* __restrict__ g = t.g[ti] + base;
    float* __restrict__ m = t.m[ti] + base;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
    const int nvec = vec ? cnt >> 2 : 0;
    if (nvec == OPT_CHUNK / 4) {
        float4 pv[OPT_VEC_PER_THREAD], gv[OPT_VEC_PER_THREAD], mv[OPT_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < OPT_VEC_PER_THREAD; ++k) {
            const int i = k * OPT_THREADS + threadIdx.x;
            pv[k] = reinterpret_cast<const float4*>(p)[i];
            gv[k] = reinterpret_cast<const float4*>(g)[i];
            mv[k] = reinterpret_cast<const float4*>(m)[i];
        }
#pragma unroll
        for (int k = 0; k < OPT_VEC_PER_THREAD; ++k) {
            const int i = k * OPT_THREADS + threadIdx.x;
            opt_update(pv[k].x, gv[k].x, mv[k].x, lr, mu, wd);
            opt_update(pv[k].y, gv[k].y, mv[k].y, lr, mu, wd);
            opt_update(pv[k].z, gv[k].z, mv[k].z, lr, mu, wd);
            opt_update(pv[k].w, gv[k].w, mv[k].w, lr, mu, wd);
            reinterpret_cast<float4*>(m)[i] = mv[k];
            reinterpret_cast<float4*>(p)[i] = pv[k];
        }
        return;
    }
    for (int i = threadIdx.x; i < nvec; i += OPT_THREADS) {
        float4 pv = reinterpret_cast<const float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<const float4*>(m)[i];
        opt_update(pv.x, gv.x, mv.x, lr, mu, wd);
        opt_update(pv.y, gv.y, mv.y, lr, mu, wd);
        opt_update(pv.z, gv.z, mv.z, lr, mu, wd);
        opt_update(pv.w, gv.w, mv.w, lr, mu, wd);
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(p)[i] = pv;
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += OPT_THREADS) {
        float pv = p[i], mv = m[i];
        opt_update(pv, g[i], mv, lr, mu, wd);
        m[i] = mv;
        p[i] = pv;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void grads_nonfinite_multi_kernel(const OptimTable t, int total_chunks, int* __restrict__ bad)
{
    const int b = blockIdx.x;
    if (b >= total_chunks) return;
    const int ti = opt_find(t, b);
    const int64_t base = (int64_t)(b - t.first[ti]) * OPT_CHUNK;
    const int64_t left = t.n[ti] - base;
    const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const float* __restrict__ g = t.g[ti] + base;
    const int nvec = ((uintptr_t)g & 15) == 0 ? cnt >> 2 : 0;
    bool seen = false;
    for (int i = threadIdx.x; i < nvec; i += OPT_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        seen = seen || opt_nonfinite(v.x) || opt_nonfinite(v.y) || opt_nonfinite(v.z) || opt_nonfinite(v.w);
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += OPT_THREADS) seen = seen || opt_nonfinite(g[i]);
    if (seen) bad[0] = 1;
}

// checks the arrays and fills the table; p / m may be NULL arrays (the gradient check reads g alone)
int opt_fill_table(const char* who, OptimTable& t, int& total_chunks, float* const* p, const float* const* g, float* const* m, const int64_t* n,
                   int count, bool need_pm)
{
    STM_REQUIRE(count >= 1, STM_EINVAL, "%s: count=%d, at least one tensor is needed", who, count);
    STM_REQUIRE(count <= OPT_T, STM_EUNSUPPORTED, "%s: count=%d, one call takes at most %d tensors", who, count, OPT_T);
    STM_REQUIRE(g && n && (!need_pm || (p && m)), STM_EINVAL, "%s: the arrays of pointers and element counts must be non-NULL", who);
    memset(&t, 0, sizeof(t));
    int64_t chunks = 0;
    for (int i = 0; i < count; ++i) {
        STM_REQUIRE(n[i] >= 0, STM_EINVAL, "%s: tensor %d has n=%lld elements", who, i, (long long)n[i]);
        STM_REQUIRE(n[i] == 0 || (g[i] && (!need_pm || (p[i] && m[i]))), STM_EINVAL, "%s: tensor %d has %lld elements and a NULL %s", who, i,
                    (long long)n[i], !g[i] ? "g" : (need_pm && !p[i]) ? "p" : "m");
        t.g[i] = g[i];
        if (need_pm) { t.p[i] = p[i]; t.m[i] = m[i]; }
        t.n[i] = n[i];
        t.first[i] = (int)chunks;
        chunks += (n[i] + OPT_CHUNK - 1) / OPT_CHUNK;
        STM_REQUIRE(chunks < ((int64_t)1 << 31), STM_EUNSUPPORTED, "%s: 2^31 chunks of %d elements or more in one call", who, OPT_CHUNK);
    }
    t.count = count;
    total_chunks = (int)chunks;
    return STM_OK;
}

}  // namespace

extern "C" int stm_sgd_step_multi_f32(float* const* p, const float* const* g, float* const* m, const int64_t* n, int count, const float* loss,
                                      const int* bad, int* counters, int first_launch, float lr, float mu, float wd, stm_stream_t stream)
{
    const char* who = "stm_sgd_step_multi_f32";
    OptimTable t;
    int total_chunks = 0;
    const int rc = opt_fill_table(who, t, total_chunks, p, g, m, n, count, true);
    if (rc) return rc;
    STM_REQUIRE(lr - lr == 0.0f && mu - mu == 0.0f && wd - wd == 0.0f, STM_EINVAL, "%s: lr=%g mu=%g wd=%g must be finite", who, (double)lr, (double)mu,
                (double)wd);
    STM_REQUIRE(counters, STM_EINVAL, "%s: counters must be non-NULL", who);
    if (total_chunks == 0 && !first_launch) return STM_OK;
    // a step over tensors without elements still counts: one workgroup for the counter
    hipLaunchKernelGGL(sgd_step_multi_kernel, dim3((unsigned)(total_chunks > 0 ? total_chunks : 1)), dim3(OPT_THREADS), 0, stm_hs(stream), t,
                       total_chunks, loss, bad, counters, first_launch, lr, mu, wd);
    STM_CHECK_LAUNCH("sgd_step_multi_kernel");
    return STM_OK;
}

extern "C" int stm_grads_nonfinite_multi_f32(const float* const* g, const int64_t* n, int count, int* bad, int first_launch, stm_stream_t stream)
{
    const char* who = "stm_grads_nonfinite_multi_f32";
    OptimTable t;
    int total_chunks = 0;
    const int rc = opt_fill_table(who, t, total_chunks, nullptr, g, nullptr, n, count, false);
    if (rc) return rc;
    STM_REQUIRE(bad, STM_EINVAL, "%s: bad must be non-NULL", who);
    if (first_launch)
        STM_REQUIRE(hipMemsetAsync(bad, 0, sizeof(int), stm_hs(stream)) == hipSuccess, STM_ELAUNCH, "%s: cannot clear bad", who);
    if (total_chunks == 0) return STM_OK;
    hipLaunchKernelGGL(grads_nonfinite_multi_kernel, dim3((unsigned)total_chunks), dim3(OPT_THREADS), 0, stm_hs(stream), t, total_chunks, bad);
    STM_CHECK_LAUNCH("grads_nonfinite_multi_kernel");
    return STM_OK;
}
