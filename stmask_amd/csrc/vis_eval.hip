// vis_eval.hip -- video mask AP on the device (include/stmask_hip_eval.h): COCO RLE strings back to run lengths, tube IoU from the run lists,
// and the greedy matching of YTVOSeval for every (video, category) group.  Integer counts throughout (uint32 runs, int64 areas and
// intersections): no sum depends on its order, no float atomics, the same bits from run to run.  stmask_amd/vis_eval.py is the caller.
#include "stm_common.h"
#include "../../include/stmask_hip_eval.h"
#include <limits.h>

namespace {

constexpr int VE_THREADS = 256;                 // four wavefronts, one item (string, mask, pair) each
constexpr int VE_WAVES = VE_THREADS / STM_WAVE;
constexpr int VE_MAX_VALUE_CHARS = 7;           // 35 bits: every |x| < 2^32 fits (rle_common.h stm_rle_chars)
constexpr int VE_LDS_IOU = 2048;                // doubles of a group's IoU block staged in LDS (16 KiB); larger blocks are read from global memory

// grid ceil(n / 4), block 256: a wavefront per string, 64 characters per pass.  A lane whose character ends a value (bit 5 clear) rebuilds the
// value from its (at most 7) characters; the ballot of those lanes numbers the runs, and two prefix sums (odd runs; even runs from run 2) undo
// the delta coding.
__global__ __launch_bounds__(VE_THREADS) void vis_rle_decode_kernel(const unsigned char* __restrict__ chars, const int64_t* __restrict__ off,
                                                                    const int64_t* __restrict__ hw, int n, int64_t total,
                                                                    unsigned int* __restrict__ runs, int* __restrict__ n_runs,
                                                                    int64_t* __restrict__ area, int* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VE_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                          // wavefront-uniform
    int64_t c0, c1;
    stm_slot(off, i, total, c0, c1);
    const int64_t L = c1 - c0;
    const unsigned char* __restrict__ s = chars + c0;
    unsigned int* __restrict__ out = runs + c0;

    int64_t nr = 0;                 // runs completed in the passes before this one
    int64_t value_start = 0;        // first character of the value that is still open
    unsigned long long carry_e = 0, carry_o = 0;                 // the last even (from run 2) / odd run decoded so far
    long long sum_all = 0, sum_odd = 0;                          // this lane's share
    int st = 0;
    for (int64_t b = 0; b < L; b += 64) {
        const int64_t p = b + lane;
        const bool in = p < L;
        const int raw = in ? (int)s[p] - 48 : 0;
        bool bad = (raw & ~63) != 0;                              // not a character rleToString writes
        const bool end = in && !(raw & 0x20);
        const unsigned long long ends = __ballot(end);
        const unsigned long long below = ends & ((1ull << lane) - 1ull);
        const int64_t j = nr + __popcll(below);                  // my run, when I end a value
        const int64_t start = below ? b + (63 - __clzll((long long)below)) + 1 : value_start;
        long long x = 0;
        if (end) {
            const int len = (int)(p - start) + 1;
            if (len > VE_MAX_VALUE_CHARS) {
                bad = true;
            } else {
                int c = 0;
                for (int k = 0; k < len; ++k) {
                    c = ((int)s[start + k] - 48) & 63;
                    x |= (long long)(c & 0x1f) << (5 * k);
                }
                if (c & 0x10) x |= (long long)(~0ull << (5 * len));
            }
        }
        const bool odd = (j & 1) != 0;
        const unsigned long long se = stm_wave_scan_u64(end && !odd && j >= 2 ? (unsigned long long)x : 0ull, lane);
        const unsigned long long so = stm_wave_scan_u64(end && odd ? (unsigned long long)x : 0ull, lane);
        const unsigned long long cnt = j == 0 ? (unsigned long long)x : (odd ? carry_o + so : carry_e + se);
        carry_e += __shfl(se, 63, STM_WAVE);
        carry_o += __shfl(so, 63, STM_WAVE);
        if (end) {
            if (cnt >> 32) {                                      // negative, or 2^32 and above
                bad = true;
            } else if (!bad) {
                out[j] = (unsigned int)cnt;                       // j <= start - 0 < L: a run per value, a character at least per value
                sum_all += (long long)cnt;
                if (odd) sum_odd += (long long)cnt;
            }
        }
        if (__ballot(bad)) st |= STM_VIS_RLE_RANGE;
        nr += __popcll(ends);
        if (ends) value_start = b + (63 - __clzll((long long)ends)) + 1;
    }
    if (value_start != L) st |= STM_VIS_RLE_UNTERMINATED;
    sum_all = stm_wave_sum_i64(sum_all);
    sum_odd = stm_wave_sum_i64(sum_odd);
    if (sum_all != hw[i]) st |= STM_VIS_RLE_SUM;
    if (lane == 0) {
        n_runs[i] = st ? 0 : (int)nr;
        area[i] = st ? 0 : sum_odd;
        status[i] = st;
    }
}

// grid ceil(n / 4), block 256: a wavefront per mask of uncompressed RLE, the same area and sum check
__global__ __launch_bounds__(VE_THREADS) void vis_rle_check_kernel(const unsigned int* __restrict__ runs, const int64_t* __restrict__ off,
                                                                   const int64_t* __restrict__ hw, int n, int64_t total, int* __restrict__ n_runs,
                                                                   int64_t* __restrict__ area, int* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VE_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    int64_t c0, c1;
    stm_slot(off, i, total, c0, c1);
    long long sum_all = 0, sum_odd = 0;
    for (int64_t p = c0 + lane; p < c1; p += 64) {
        const long long c = (long long)runs[p];
        sum_all += c;
        if ((p - c0) & 1) sum_odd += c;
    }
    sum_all = stm_wave_sum_i64(sum_all);
    sum_odd = stm_wave_sum_i64(sum_odd);
    int st = sum_all != hw[i] ? STM_VIS_RLE_SUM : 0;
    if (c1 - c0 > INT_MAX) st |= STM_VIS_RLE_RANGE;
    if (lane == 0) {
        n_runs[i] = st ? 0 : (int)(c1 - c0);
        area[i] = st ? 0 : sum_odd;
        status[i] = st;
    }
}

// |a & b| of two run lists (runs alternate 0, 1 from a run of 0s): a two-pointer merge.  Every step closes a run of a or of b (a zero-length run
// closes at once), so it ends after at most na + nb steps.
__device__ __forceinline__ long long ve_rle_intersection(const unsigned int* __restrict__ a, int na, const unsigned int* __restrict__ b, int nb)
{
    if (na <= 0 || nb <= 0) return 0;
    int ia = 0, ib = 0;
    unsigned int ca = a[0], cb = b[0];
    long long inter = 0;
    while (true) {
        const unsigned int c = min(ca, cb);
        if (ia & ib & 1) inter += c;
        ca -= c;
        cb -= c;
        if (ca == 0) {
            if (++ia >= na) break;
            ca = a[ia];
        }
        if (cb == 0) {
            if (++ib >= nb) break;
            cb = b[ib];
        }
    }
    return inter;
}

struct TubeArgs {
    const int* pair_d;
    const int* pair_g;
    const int* table;            // [n_tracks, max_frames]
    const int* track_len;
    const unsigned int* runs;
    const int64_t* run_off;
    const int* n_runs;
    const int64_t* area;
    int64_t* inter;
    int64_t* uni;
    double* iou;
    int64_t n_pairs, n_masks;
    int n_tracks, max_frames;
};

// grid ceil(n_pairs / 4), block 256: a wavefront per pair, a lane per frame
__global__ __launch_bounds__(VE_THREADS) void vis_tube_iou_kernel(const TubeArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * VE_WAVES + (threadIdx.x >> 6);
    if (pair >= a.n_pairs) return;
    const int td = a.pair_d[pair], tg = a.pair_g[pair];
    int nf = 0;
    if (td >= 0 && td < a.n_tracks && tg >= 0 && tg < a.n_tracks) nf = min(min(a.track_len[td], a.track_len[tg]), a.max_frames);
    long long i = 0, u = 0;
    for (int f = lane; f < nf; f += 64) {
        const int64_t md = a.table[(int64_t)td * a.max_frames + f], mg = a.table[(int64_t)tg * a.max_frames + f];
        const bool hd = md >= 0 && md < a.n_masks, hg = mg >= 0 && mg < a.n_masks;
        if (hd && hg) {
            const long long x = ve_rle_intersection(a.runs + a.run_off[md], a.n_runs[md], a.runs + a.run_off[mg], a.n_runs[mg]);
            i += x;
            u += a.area[md] + a.area[mg] - x;
        } else if (hd) {
            u += a.area[md];
        } else if (hg) {
            u += a.area[mg];
        }
    }
    i = stm_wave_sum_i64(i);
    u = stm_wave_sum_i64(u);
    if (lane == 0) {
        a.inter[pair] = i;
        a.uni[pair] = u;
        a.iou[pair] = u > 0 ? (double)i / (double)u : 0.0;
    }
}

struct MatchArgs {
    const double* iou;
    const int64_t* pair_off;
    const int* dt_off;
    const int* gt_off;
    const double* dt_area;
    const double* gt_area;
    const int* gt_crowd;
    const double* thr;
    const double* area_rng;
    int* dt_match;
    unsigned char* dt_ignore;
    unsigned char* gt_ignore;
    int n_thr, n_area, max_d, max_g;
};

// grid n_groups, block 64: thread a * n_thr + t walks the group's detections in order for area range a and threshold t
__global__ __launch_bounds__(STM_VIS_MAX_THREADS) void vis_match_kernel(const MatchArgs a)
{
    __shared__ double s_iou[VE_LDS_IOU];
    __shared__ unsigned int s_taken[STM_VIS_MAX_GT / 32][STM_VIS_MAX_THREADS];     // bit g of thread tid: ground truth g is matched at (a, t)
    const int grp = blockIdx.x, tid = threadIdx.x;
    const int d0 = a.dt_off[grp], g0 = a.gt_off[grp];
    const int D = min(max(a.dt_off[grp + 1] - d0, 0), a.max_d), G = min(max(a.gt_off[grp + 1] - g0, 0), a.max_g);
    const double* __restrict__ blk = a.iou + a.pair_off[grp];
    const bool staged = D * G <= VE_LDS_IOU;
    if (staged) {
        for (int k = tid; k < D * G; k += STM_VIS_MAX_THREADS) s_iou[k] = blk[k];
    }
    for (int k = tid; k < G * a.n_area; k += STM_VIS_MAX_THREADS) {
        const int g = k / a.n_area, ar = k - g * a.n_area;
        const double ga = a.gt_area[g0 + g];
        a.gt_ignore[(int64_t)(g0 + g) * a.n_area + ar] = (a.gt_crowd[g0 + g] != 0 || ga < a.area_rng[2 * ar] || ga > a.area_rng[2 * ar + 1]) ? 1 : 0;
    }
    for (int w = 0; w < (G + 31) / 32; ++w) s_taken[w][tid] = 0u;
    __syncthreads();
    if (tid >= a.n_thr * a.n_area) return;
    const int ar = tid / a.n_thr, t = tid - ar * a.n_thr;
    const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
    const double thr = fmin(a.thr[t], 1.0 - 1e-10);
    const double* __restrict__ src = staged ? s_iou : blk;
    for (int d = 0; d < D; ++d) {
        double best = thr;
        int m = -1, m_ignored = 0;
        for (int pass = 0; pass < 2 && m < 0; ++pass) {          // the non-ignored ground truths first; the ignored ones only while m is unset
            for (int g = 0; g < G; ++g) {
                const bool crowd = a.gt_crowd[g0 + g] != 0;
                const double ga = a.gt_area[g0 + g];
                const int ignored = (crowd || ga < lo || ga > hi) ? 1 : 0;
                if (ignored != pass) continue;
                if (((s_taken[g >> 5][tid] >> (g & 31)) & 1u) && !crowd) continue;
                const double v = src[d * G + g];
                if (v < best) continue;
                best = v;
                m = g;
                m_ignored = ignored;
            }
        }
        const int64_t o = ((int64_t)(d0 + d) * a.n_area + ar) * a.n_thr + t;
        a.dt_match[o] = m;
        if (m >= 0) {
            s_taken[m >> 5][tid] |= 1u << (m & 31);
            a.dt_ignore[o] = (unsigned char)m_ignored;
        } else {
            const double da = a.dt_area[d0 + d];
            a.dt_ignore[o] = (da < lo || da > hi) ? 1 : 0;
        }
    }
}

}  // namespace

extern "C" int stm_vis_rle_decode(const unsigned char* chars, const int64_t* offsets, const int64_t* hw, int n, int64_t total_chars,
                                  unsigned int* runs, int* n_runs, int64_t* area, int* status, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && total_chars >= 0 && total_chars <= INT_MAX, STM_EINVAL, "stm_vis_rle_decode: bad sizes (n >= 0, 0 <= total_chars < 2^31)");
    if (n == 0) return STM_OK;
    STM_REQUIRE(offsets && hw && n_runs && area && status && (total_chars == 0 || (chars && runs)), STM_ENULL, "stm_vis_rle_decode: NULL argument");
    hipLaunchKernelGGL(vis_rle_decode_kernel, dim3(stm_cdiv(n, VE_WAVES)), dim3(VE_THREADS), 0, stm_hs(stream), chars, offsets, hw, n, total_chars,
                       runs, n_runs, area, status);
    STM_CHECK_LAUNCH("vis_rle_decode_kernel");
    return STM_OK;
}

extern "C" int stm_vis_rle_check(const unsigned int* runs, const int64_t* offsets, const int64_t* hw, int n, int64_t total_runs, int* n_runs,
                                 int64_t* area, int* status, stm_stream_t stream)
{
    STM_REQUIRE(n >= 0 && total_runs >= 0, STM_EINVAL, "stm_vis_rle_check: bad sizes");
    if (n == 0) return STM_OK;
    STM_REQUIRE(offsets && hw && n_runs && area && status && (total_runs == 0 || runs), STM_ENULL, "stm_vis_rle_check: NULL argument");
    hipLaunchKernelGGL(vis_rle_check_kernel, dim3(stm_cdiv(n, VE_WAVES)), dim3(VE_THREADS), 0, stm_hs(stream), runs, offsets, hw, n, total_runs,
                       n_runs, area, status);
    STM_CHECK_LAUNCH("vis_rle_check_kernel");
    return STM_OK;
}

extern "C" int stm_vis_tube_iou(const int* pair_d, const int* pair_g, int64_t n_pairs, const int* table, const int* track_len, int n_tracks,
                                int max_frames, const unsigned int* runs, const int64_t* run_off, const int* n_runs, const int64_t* area,
                                int64_t n_masks, int64_t* inter, int64_t* uni, double* iou, stm_stream_t stream)
{
    STM_REQUIRE(n_pairs >= 0 && n_pairs <= (int64_t)INT_MAX && n_tracks >= 0 && max_frames >= 0 && n_masks >= 0, STM_EINVAL,
                "stm_vis_tube_iou: bad sizes (0 <= n_pairs < 2^31)");
    if (n_pairs == 0) return STM_OK;
    STM_REQUIRE(pair_d && pair_g && inter && uni && iou, STM_ENULL, "stm_vis_tube_iou: NULL argument");
    STM_REQUIRE(n_tracks == 0 || (track_len && (max_frames == 0 || table)), STM_ENULL, "stm_vis_tube_iou: NULL track table");
    STM_REQUIRE(n_masks == 0 || (run_off && n_runs && area), STM_ENULL, "stm_vis_tube_iou: NULL mask arrays");
    TubeArgs a;
    a.pair_d = pair_d; a.pair_g = pair_g; a.table = table; a.track_len = track_len; a.runs = runs; a.run_off = run_off; a.n_runs = n_runs;
    a.area = area; a.inter = inter; a.uni = uni; a.iou = iou; a.n_pairs = n_pairs; a.n_masks = n_masks; a.n_tracks = n_tracks;
    a.max_frames = max_frames;
    hipLaunchKernelGGL(vis_tube_iou_kernel, dim3(stm_cdiv(n_pairs, VE_WAVES)), dim3(VE_THREADS), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("vis_tube_iou_kernel");
    return STM_OK;
}

extern "C" int stm_vis_match(const double* iou, const int64_t* pair_off, const int* dt_off, const int* gt_off, int n_groups, int max_d, int max_g,
                             const double* dt_area, const double* gt_area, const int* gt_crowd, const double* thr, int n_thr, const double* area_rng,
                             int n_area, int* dt_match, unsigned char* dt_ignore, unsigned char* gt_ignore, stm_stream_t stream)
{
    STM_REQUIRE(n_groups >= 0 && n_thr > 0 && n_area > 0 && n_thr * (int64_t)n_area <= STM_VIS_MAX_THREADS, STM_EINVAL,
                "stm_vis_match: bad sizes (n_thr * n_area in 1..%d)", STM_VIS_MAX_THREADS);
    STM_REQUIRE(max_d >= 0 && max_d <= STM_VIS_MAX_DET, STM_EINVAL, "stm_vis_match: %d detections in a group (at most %d)", max_d, STM_VIS_MAX_DET);
    STM_REQUIRE(max_g >= 0 && max_g <= STM_VIS_MAX_GT, STM_EINVAL, "stm_vis_match: %d ground-truth tracks in a group (at most %d)", max_g,
                STM_VIS_MAX_GT);
    if (n_groups == 0) return STM_OK;
    STM_REQUIRE(pair_off && dt_off && gt_off && thr && area_rng, STM_ENULL, "stm_vis_match: NULL argument");
    STM_REQUIRE(max_d == 0 || (dt_area && dt_match && dt_ignore), STM_ENULL, "stm_vis_match: NULL detection arrays");
    STM_REQUIRE(max_g == 0 || (gt_area && gt_crowd && gt_ignore), STM_ENULL, "stm_vis_match: NULL ground-truth arrays");
    STM_REQUIRE(max_d == 0 || max_g == 0 || iou, STM_ENULL, "stm_vis_match: NULL iou");
    MatchArgs a;
    a.iou = iou; a.pair_off = pair_off; a.dt_off = dt_off; a.gt_off = gt_off; a.dt_area = dt_area; a.gt_area = gt_area; a.gt_crowd = gt_crowd;
    a.thr = thr; a.area_rng = area_rng; a.dt_match = dt_match; a.dt_ignore = dt_ignore; a.gt_ignore = gt_ignore; a.n_thr = n_thr; a.n_area = n_area;
    a.max_d = max_d; a.max_g = max_g;
    hipLaunchKernelGGL(vis_match_kernel, dim3(n_groups), dim3(STM_VIS_MAX_THREADS), 0, stm_hs(stream), a);
    STM_CHECK_LAUNCH("vis_match_kernel");
    return STM_OK;
}
