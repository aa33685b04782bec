// track_resolve.hip -- the temporal-fusion tracker's decisions as kernels (include/stmask_hip_tracker.h): what stmask_amd/track_host.py decides
// on host lists between two device reads -- match_tf (track_TF.py:132-156) and keep_rows -- decided on the device, as gather plans for
// stm_gather_rows2.  Integer bookkeeping over a few thousand rows, one workgroup per clip: the point is that no count, score or id has to
// reach the host before the plan exists.  No atomics on floats, no hand-off between workgroups: a clip's base in the plan is recounted by its
// own workgroup from the clips before it, so the outputs are the same from run to run.
#include "stm_common.h"
#include "../../include/stmask_hip_tracker.h"
#include <limits.h>

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_CLIPS = 1024;

struct ResolveArgs {
    const int* match;        // [D] or null (all 0)
    const float* score;      // [D]
    const int* cnt;          // [B]
    const int* off;          // [B + 1]
    const int* tm;           // [Pn]
    int* plan;               // [Pn + D]
    int* new_off;            // [B + 1]
    int* new_tm;             // [Pn + D]
    int B, Pn, D, cap;
};

// unmatched detections that open a track in a clip of pn rows (cap > 0: only while the clip holds fewer than cap)
__device__ __forceinline__ int tr_opened(int unmatched, int pn, int cap)
{
    return cap > 0 ? min(unmatched, max(cap - pn, 0)) : unmatched;
}

// a clip's tracked rows [p0, p0 + pn), never outside [0, Pn] whatever the offsets hold
__device__ __forceinline__ void tr_clip_rows(const int* off, int c, int Pn, int& p0, int& pn)
{
    p0 = min(max(off[c], 0), Pn);
    pn = min(max(off[c + 1], p0), Pn) - p0;
}

// grid B, block 256.  Detection rows of clip b: [s_doff[b], s_doff[b + 1]) (prefix of the counts, clamped to D).
__global__ __launch_bounds__(TR_THREADS) void track_resolve_tf_kernel(const ResolveArgs a)
{
    __shared__ int s_doff[TR_MAX_CLIPS + 1];
    __shared__ int s_wave[4];
    __shared__ int s_match[TR_THREADS];
    __shared__ float s_score[TR_THREADS];
    __shared__ int s_running;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int total = a.Pn + a.D;
    if (tid == 0) {
        int acc = 0;
        s_doff[0] = 0;
        for (int c = 0; c <= b; ++c) {
            acc = min(acc + max(a.cnt[c], 0), a.D);
            s_doff[c + 1] = acc;
        }
    }
    __syncthreads();

    // rows of the clips before this one: a wave per clip recounts its unmatched detections
    int wsum = 0;
    for (int c = wave; c < b; c += 4) {
        const int d0 = s_doff[c], d1 = s_doff[c + 1];
        int z = d1 - d0;
        if (a.match) {
            z = 0;
            for (int d = d0 + lane; d < d1; d += 64) z += a.match[d] == 0 ? 1 : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, STM_WAVE);
        }
        int q0, qn;
        tr_clip_rows(a.off, c, a.Pn, q0, qn);
        wsum += qn + tr_opened(z, qn, a.cap);
    }
    if (lane == 0) s_wave[wave] = wsum;
    __syncthreads();
    const int base = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];

    int p0, pn;
    tr_clip_rows(a.off, b, a.Pn, p0, pn);
    const int d0 = s_doff[b], dn = s_doff[b + 1] - d0;

    // tracked rows, 256 per pass: every thread walks the clip's detections in order (staged 256 at a time) for its row -- the host loop's
    // `score > best` from -1.0, so the first among equal scores wins
    for (int rb = 0; rb < pn; rb += TR_THREADS) {
        const int r = rb + tid;
        const int target = 1 + p0 + r;
        float best = -1.0f;
        int bd = -1;
        if (a.match) {
            for (int db = 0; db < dn; db += TR_THREADS) {
                __syncthreads();                                 // the chunk before this one has been read by everyone
                if (db + tid < dn) {
                    s_match[tid] = a.match[d0 + db + tid];
                    s_score[tid] = a.score[d0 + db + tid];
                }
                __syncthreads();
                const int m = min(TR_THREADS, dn - db);
                if (r < pn) {
                    for (int k = 0; k < m; ++k) {
                        if (s_match[k] == target && s_score[k] > best) {
                            best = s_score[k];
                            bd = db + k;
                        }
                    }
                }
            }
        }
        const int at = base + r;
        if (r < pn && at < total) {
            a.plan[at] = bd >= 0 ? a.Pn + d0 + bd : p0 + r;
            a.new_tm[at] = bd >= 0 ? 0 : a.tm[p0 + r];
        }
    }

    // unmatched detections, in detection order, behind the clip's rows (ordered compaction: ballot + prefix over 256 per pass)
    const int room = a.cap > 0 ? max(a.cap - pn, 0) : INT_MAX;
    if (tid == 0) s_running = 0;
    __syncthreads();
    for (int db = 0; db < dn; db += TR_THREADS) {
        const int j = db + tid;
        const bool f = j < dn && (a.match == nullptr || a.match[d0 + j] == 0);
        const unsigned long long bal = __ballot(f);
        const int lane_prefix = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int wp = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) wp += s_wave[w];
            tot += s_wave[w];
        }
        const int start = s_running;
        const int pos = start + wp + lane_prefix;
        const int at = base + pn + pos;
        if (f && pos < room && at < total) {
            a.plan[at] = a.Pn + d0 + j;
            a.new_tm[at] = 0;
        }
        __syncthreads();
        if (tid == 0) s_running = start + tot;
        __syncthreads();
    }
    const int end = min(base + pn + min(s_running, room), total);
    if (tid == 0) a.new_off[b] = min(base, total);
    if (b == a.B - 1) {
        if (tid == 0) a.new_off[a.B] = end;
        for (int i = end + tid; i < total; i += TR_THREADS) {     // the padding: index 0, counter 0
            a.plan[i] = 0;
            a.new_tm[i] = 0;
        }
    }
}

// grid B, block 256: the rows of the clips that stay, in order
__global__ __launch_bounds__(TR_THREADS) void track_drop_plan_kernel(const int* __restrict__ off, const int* __restrict__ drop, int B, int n_keep,
                                                                      int* __restrict__ keep, int* __restrict__ new_off)
{
    __shared__ int s_base;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int acc = 0;
        for (int c = 0; c < b; ++c) acc += drop[c] ? 0 : max(off[c + 1] - off[c], 0);
        s_base = acc;
    }
    __syncthreads();
    const int base = s_base;
    const int p0 = off[b];
    const int pn = drop[b] ? 0 : max(off[b + 1] - p0, 0);
    for (int i = tid; i < pn; i += TR_THREADS)
        if (base + i < n_keep) keep[base + i] = p0 + i;
    if (tid == 0) {
        new_off[b] = base;
        if (b == B - 1) new_off[B] = base + pn;
    }
}

}  // namespace

extern "C" int stm_track_resolve_tf(const int* match, const float* det_score, const int* det_count, const int* prev_offsets, const int* prev_tm,
                                    int B, int Pn, int D, int cap, int* plan, int* new_offsets, int* new_tm, stm_stream_t stream)
{
    STM_REQUIRE(B > 0 && B <= TR_MAX_CLIPS && Pn >= 0 && D >= 0 && cap >= 0 && (int64_t)Pn + D <= INT_MAX, STM_EINVAL,
                "stm_track_resolve_tf: bad sizes (1..%d clips)", TR_MAX_CLIPS);
    STM_REQUIRE(det_count && prev_offsets && new_offsets, STM_ENULL, "stm_track_resolve_tf: NULL argument");
    STM_REQUIRE(Pn + D == 0 || (plan && new_tm), STM_ENULL, "stm_track_resolve_tf: NULL plan or counters");
    STM_REQUIRE(Pn == 0 || prev_tm, STM_ENULL, "stm_track_resolve_tf: NULL prev_tm");
    STM_REQUIRE(!match || D == 0 || det_score, STM_ENULL, "stm_track_resolve_tf: NULL det_score");
    ResolveArgs a;
    a.match = D > 0 ? match : nullptr; a.score = det_score; a.cnt = det_count; a.off = prev_offsets; a.tm = prev_tm;
    a.plan = plan; a.new_off = new_offsets; a.new_tm = new_tm; a.B = B; a.Pn = Pn; a.D = D; a.cap = cap;
    hipLaunchKernelGGL(track_resolve_tf_kernel, dim3(B), dim3(TR_THREADS), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("track_resolve_tf_kernel");
    return STM_OK;
}

extern "C" int stm_track_drop_plan(const int* offsets, const int* drop, int B, int n_keep, int* keep_rows, int* new_offsets, stm_stream_t stream)
{
    STM_REQUIRE(B > 0 && B <= TR_MAX_CLIPS && n_keep >= 0, STM_EINVAL, "stm_track_drop_plan: bad sizes (1..%d clips)", TR_MAX_CLIPS);
    STM_REQUIRE(offsets && drop && new_offsets && (n_keep == 0 || keep_rows), STM_ENULL, "stm_track_drop_plan: NULL argument");
    hipLaunchKernelGGL(track_drop_plan_kernel, dim3(B), dim3(TR_THREADS), 0, stm_hs(stream), offsets, drop, B, n_keep, keep_rows, new_offsets);
    STM_CHECK_LAUNCH("track_drop_plan_kernel");
    return STM_OK;
}
