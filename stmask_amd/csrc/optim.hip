// optim.hip -- the guarded, fused SGD step of the training loop for gfx950 (MI355X), single-rank (csrc/optim.h) and as the finish of a
// data-parallel step (csrc/dp_step.h); both package-private, stmask_amd/optim.py.
//
//   stm_sgd_step_multi_f32         weight decay, momentum and the parameter write of up to STM_OPTIM_MAX_TENSORS tensors in one launch and one
//                                  pass: 12 bytes read and 8 written per element, no LDS.  The guard (loss finite, bad == 0) is read by every
//                                  workgroup before it touches anything, so a skipped step costs a launch of workgroups that return at once and
//                                  the host never waits for the verdict.
//   stm_dp_sgd_finish_multi_f32    the same step over the all-reduced gradient arena: the summed gradient times 1 / world first, and 0.0f
//                                  written back over every gradient element read: 12 bytes read and 12 written per element.  A skipped step
//                                  still clears its gradients (4 bytes written per element, nothing read).
//   stm_grads_nonfinite_multi_f32  the same table over the gradients alone: any NaN / inf sets bad[0].
//
// The tensor table is a kernel argument (OptimTable, ~2.3 KB, chunk_table.h): pointers, element counts and the index of each tensor's first chunk.
// A workgroup owns one chunk of STM_OPTIM_CHUNK elements.  A chunk whose three addresses are 16-byte aligned goes through float4 loads and
// stores, four per thread with all twelve loads issued before the arithmetic (the data-parallel form's zeros go out first, they depend on no
// load, then m, then p); its last n % 4 elements, and every chunk of a tensor whose storage starts at an odd offset, take the 4-byte path.
// Compiled with -ffp-contract=off: the expressions stay three multiplies (four with 1 / world) and three adds in the stated order.
#include "stm_common.h"
#include "chunk_table.h"
#include "optim.h"
#include "dp_step.h"
#include <type_traits>

namespace {

constexpr int OPT_T = STM_CHUNK_MAX_ROWS;
constexpr int OPT_CHUNK = STM_CHUNK_ELEMS;
constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC_PER_THREAD = OPT_CHUNK / 4 / OPT_THREADS;
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is a whole number of float4 per thread");

struct OptimTable {
    float* p[OPT_T];
    float* g[OPT_T];       // written by the data-parallel finish alone
    float* m[OPT_T];
    int64_t n[OPT_T];
    int first[OPT_T];      // index of the tensor's first chunk among the chunks of this launch
    int count;
};
static_assert(sizeof(OptimTable) + 64 < 4096, "the table travels in the kernel arguments");

// DP: g is the sum over the ranks
template <bool DP>
__device__ __forceinline__ void opt_update(float& p, float g, float& m, float inv_world, float lr, float mu, float wd)
{
    if constexpr (DP) g = g * inv_world;
    const float g1 = g + wd * p;
    m = mu * m + g1;
    p = p - lr * m;
}

// One chunk of the step.  DP (the data-parallel finish) differs in four places: the gradient is scaled by inv_world, every gradient element read
// is overwritten with 0.0f (so g is not const), and a skipped step still clears its gradients.
template <bool DP>
__device__ __forceinline__ void opt_step_chunk(const OptimTable& t, int total_chunks, const float* loss, const int* bad, int* counters,
                                               int first_launch, float inv_world, float lr, float mu, float wd)
{
    bool skip = false;
    if (loss) skip = stm_nonfinite(loss[0]);
    if (bad) skip = skip || bad[0] != 0;
    if (first_launch && blockIdx.x == 0 && threadIdx.x == 0) {
        const int slot = skip ? 1 : 0;
        const int seen = counters[slot];
        counters[slot] = seen + 1;
    }
    const int b = blockIdx.x;
    if ((!DP && skip) || b >= total_chunks) return;
    int64_t base;
    int cnt;
    const int ti = stm_chunk_of(t, b, base, cnt);
    std::conditional_t<DP, float, const float>* __restrict__ g = t.g[ti] + base;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (DP) {
        if (skip) {                      // nothing is read: p and m stay as they are, the gradients are cleared
            const int nz = ((uintptr_t)g & 15) == 0 ? cnt >> 2 : 0;
            for (int i = threadIdx.x; i < nz; i += OPT_THREADS) reinterpret_cast<float4*>(g)[i] = zero4;
            for (int i = nz * 4 + threadIdx.x; i < cnt; i += OPT_THREADS) g[i] = 0.0f;
            return;
        }
    }
    float* __restrict__ p = t.p[ti] + base;
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
            opt_update<DP>(pv[k].x, gv[k].x, mv[k].x, inv_world, lr, mu, wd);
            opt_update<DP>(pv[k].y, gv[k].y, mv[k].y, inv_world, lr, mu, wd);
            opt_update<DP>(pv[k].z, gv[k].z, mv[k].z, inv_world, lr, mu, wd);
            opt_update<DP>(pv[k].w, gv[k].w, mv[k].w, inv_world, lr, mu, wd);
            if constexpr (DP) reinterpret_cast<float4*>(g)[i] = zero4;
            reinterpret_cast<float4*>(m)[i] = mv[k];
            reinterpret_cast<float4*>(p)[i] = pv[k];
        }
        return;
    }
    for (int i = threadIdx.x; i < nvec; i += OPT_THREADS) {
        float4 pv = reinterpret_cast<const float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<const float4*>(m)[i];
        opt_update<DP>(pv.x, gv.x, mv.x, inv_world, lr, mu, wd);
        opt_update<DP>(pv.y, gv.y, mv.y, inv_world, lr, mu, wd);
        opt_update<DP>(pv.z, gv.z, mv.z, inv_world, lr, mu, wd);
        opt_update<DP>(pv.w, gv.w, mv.w, inv_world, lr, mu, wd);
        if constexpr (DP) reinterpret_cast<float4*>(g)[i] = zero4;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(p)[i] = pv;
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += OPT_THREADS) {
        float pv = p[i], mv = m[i];
        opt_update<DP>(pv, g[i], mv, inv_world, lr, mu, wd);
        if constexpr (DP) g[i] = 0.0f;
        m[i] = mv;
        p[i] = pv;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_step_multi_kernel(const OptimTable t, int total_chunks, const float* __restrict__ loss,
                                                                     const int* __restrict__ bad, int* __restrict__ counters, int first_launch,
                                                                     float lr, float mu, float wd)
{
    opt_step_chunk<false>(t, total_chunks, loss, bad, counters, first_launch, 0.0f, lr, mu, wd);
}

// loss_sum may point into the arena that g points into: no __restrict__
__global__ __launch_bounds__(OPT_THREADS) void dp_sgd_finish_multi_kernel(const OptimTable t, int total_chunks, const float* loss_sum,
                                                                          const int* __restrict__ bad, int* __restrict__ counters, int first_launch,
                                                                          float inv_world, float lr, float mu, float wd)
{
    opt_step_chunk<true>(t, total_chunks, loss_sum, bad, counters, first_launch, inv_world, lr, mu, wd);
}

__global__ __launch_bounds__(OPT_THREADS) void grads_nonfinite_multi_kernel(const OptimTable t, int total_chunks, int* __restrict__ bad)
{
    const int b = blockIdx.x;
    if (b >= total_chunks) return;
    int64_t base;
    int cnt;
    const int ti = stm_chunk_of(t, b, base, cnt);
    const float* __restrict__ g = t.g[ti] + base;
    const int nvec = ((uintptr_t)g & 15) == 0 ? cnt >> 2 : 0;
    bool seen = false;
    for (int i = threadIdx.x; i < nvec; i += OPT_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        seen = seen || stm_nonfinite(v.x) || stm_nonfinite(v.y) || stm_nonfinite(v.z) || stm_nonfinite(v.w);
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += OPT_THREADS) seen = seen || stm_nonfinite(g[i]);
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
        t.g[i] = const_cast<float*>(g[i]);      // only dp_sgd_finish_multi_kernel writes through it, and its caller passes float*
        if (need_pm) { t.p[i] = p[i]; t.m[i] = m[i]; }
        t.n[i] = n[i];
        const int rc = stm_chunk_append(who, t.first, i, n[i], chunks);
        if (rc) return rc;
    }
    t.count = count;
    total_chunks = (int)chunks;
    return STM_OK;
}

// the checks and the launch the two forms of the step share; dp: inv_world is checked and used
template <bool DP>
int opt_step(const char* who, float* const* p, const float* const* g, float* const* m, const int64_t* n, int count, const float* loss, const int* bad,
             int* counters, int first_launch, float inv_world, float lr, float mu, float wd, stm_stream_t stream)
{
    OptimTable t;
    int total_chunks = 0;
    const int rc = opt_fill_table(who, t, total_chunks, p, g, m, n, count, true);
    if (rc) return rc;
    STM_REQUIRE(lr - lr == 0.0f && mu - mu == 0.0f && wd - wd == 0.0f, STM_EINVAL, "%s: lr=%g mu=%g wd=%g must be finite", who, (double)lr, (double)mu,
                (double)wd);
    if constexpr (DP) STM_REQUIRE(inv_world > 0.0f && inv_world <= 1.0f, STM_EINVAL, "%s: inv_world=%g must lie in (0, 1]", who, (double)inv_world);
    STM_REQUIRE(counters, STM_EINVAL, "%s: counters must be non-NULL", who);
    if (total_chunks == 0 && !first_launch) return STM_OK;
    // a step over tensors without elements still counts: one workgroup for the counter
    const dim3 grid((unsigned)(total_chunks > 0 ? total_chunks : 1));
    if (DP) {
        hipLaunchKernelGGL(dp_sgd_finish_multi_kernel, grid, dim3(OPT_THREADS), 0, stm_hs(stream), t, total_chunks, loss, bad, counters, first_launch,
                           inv_world, lr, mu, wd);
        STM_CHECK_LAUNCH("dp_sgd_finish_multi_kernel");
    } else {
        hipLaunchKernelGGL(sgd_step_multi_kernel, grid, dim3(OPT_THREADS), 0, stm_hs(stream), t, total_chunks, loss, bad, counters, first_launch, lr,
                           mu, wd);
        STM_CHECK_LAUNCH("sgd_step_multi_kernel");
    }
    return STM_OK;
}

}  // namespace

extern "C" int stm_sgd_step_multi_f32(float* const* p, const float* const* g, float* const* m, const int64_t* n, int count, const float* loss,
                                      const int* bad, int* counters, int first_launch, float lr, float mu, float wd, stm_stream_t stream)
{
    return opt_step<false>("stm_sgd_step_multi_f32", p, g, m, n, count, loss, bad, counters, first_launch, 1.0f, lr, mu, wd, stream);
}

extern "C" int stm_dp_sgd_finish_multi_f32(float* const* p, float* const* g, float* const* m, const int64_t* n, int count, const float* loss_sum,
                                           const int* bad, int* counters, int first_launch, float inv_world, float lr, float mu, float wd,
                                           stm_stream_t stream)
{
    return opt_step<true>("stm_dp_sgd_finish_multi_f32", p, g, m, n, count, loss_sum, bad, counters, first_launch, inv_world, lr, mu, wd, stream);
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
