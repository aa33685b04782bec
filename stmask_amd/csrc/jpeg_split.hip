// jpeg_split.hip -- one entropy-coded segment decoded at many places at once on gfx950 (MI355X): what launch 1 of csrc/jpeg.h becomes for the
// images of a batch that are SPLIT.  The arithmetic of a lane is csrc/jpeg_split_core.h; this file is how it is spread over the machine and how
// the lanes' guesses are repaired.  csrc/jpeg_decode.hip's entry point makes the launches (jpeg_split_launch) and runs its serial kernel after
// them, which decodes the segments marked REDO.
//
//   jpeg_split_sync_kernel    one 64-lane workgroup per group of STM_JPEG_SUB_GROUP sub-sequences, one lane a sub-sequence; launched
//                             STM_JPEG_SPLIT_ROUNDS + 1 times.  The code is divergent by nature -- every lane walks its own Huffman codes -- so
//                             nothing is held wave-uniform here.  The group's bytes (and the few a last step may reach behind them) are staged
//                             in LDS with 16-byte loads, each sub-sequence 4 bytes further on than its raw place, so that the lanes, which read
//                             128 bytes apart, start on 64 different banks instead of one; the image's four Huffman tables lie in LDS whole
//                             (5.6 KiB: a lane's lookups are random, registers and readlane do not serve 64 different indices).  Round 0 also
//                             zeroes the image's coefficients, a slice per group.
//   jpeg_split_scan_kernel    one 256-thread workgroup per image: exclusive prefix sums of (blocks, DC sums) over the records, 256 at a time with a
//                             running carry, in place.
//   jpeg_split_write_kernel   the grid and staging of the sync kernel; every lane decodes from its true state and stores the coefficients
//                             that are not zero, 2 bytes each.
//
// No atomics; every result is a vector store (several lanes may store the same 1 to a segment's REDO mark).  Every loop is bounded by the
// segment's byte and block counts; every byte read lies inside the segment's 16-byte padded extent, every record inside the image's planes.
#include "stm_common.h"
#include "jpeg_split_core.h"

namespace {

constexpr int SUB = STM_JPEG_SUB_BYTES, GROUP = STM_JPEG_SUB_GROUP;
constexpr int TAIL = 32;                                // bytes staged behind the group: 5 data bytes of a last step, their stuffing, one to look at
constexpr int STAGED = GROUP * SUB + TAIL;
constexpr int SKEW = 4;                                 // bytes a sub-sequence is moved on in LDS
constexpr int LDS_BYTES = STAGED + (STAGED / SUB + 1) * SKEW;
static_assert(GROUP == STM_WAVE && SUB % 16 == 0 && STAGED % 16 == 0 && sizeof(stm_jpeg_huff) % 16 == 0, "one wave a group, 16-byte loads");

// the group's bytes in LDS; every lane asks for bytes of its own
struct GroupSource {
    const uint8_t* lds;
    int g0;                 // first byte of the group in the segment
    int prev;               // byte g0 - 1 (a guess looks one byte back)
    __device__ __forceinline__ int get(int p) const
    {
        const int rel = p - g0;
        if ((unsigned)rel < (unsigned)STAGED) return lds[rel + (rel / SUB) * SKEW];
        return rel == -1 ? prev : 0;
    }
};

// what a workgroup of the sync and write kernels knows of its group
struct GroupCtx {
    stm_jpeg_image im;
    int nbytes, n_sub, sub0, group, n_groups, n0, bpm, tsel;
    JpegSplitRec* rec;
    GroupSource src;
};

// the image of group g (the last one whose split field is <= 2 g + 1: csrc/jpeg.h), its one segment (the first of `segments` that names the
// image; the list is ordered by image), the tables and the group's bytes into LDS
__device__ __forceinline__ void group_setup(GroupCtx& cx, const uint8_t* __restrict__ blob, const stm_jpeg_image* __restrict__ images, int n_images,
                                            const stm_jpeg_segment* __restrict__ segments, int n_segments, uint8_t* __restrict__ planes,
                                            stm_jpeg_huff* s_huff, uint8_t* s_bytes)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (images[mid].split <= 2 * g + 1) lo = mid;
        else hi = mid - 1;
    }
    const int img = lo;
    cx.im = images[img];
    lo = 0;
    hi = n_segments - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segments[mid].image < img) lo = mid + 1;
        else hi = mid;
    }
    const stm_jpeg_segment sg = segments[lo];
    cx.nbytes = sg.nbytes;
    cx.n_sub = jpeg_split_subs(sg.nbytes);
    cx.n_groups = jpeg_split_groups(sg.nbytes);
    cx.group = g - (cx.im.split >> 1);
    cx.sub0 = cx.group * GROUP;
    cx.n0 = cx.im.hs * cx.im.vs;
    cx.bpm = jpeg_blocks_per_mcu(cx.im);
    cx.tsel = jpeg_split_tables(cx.im);
    cx.rec = reinterpret_cast<JpegSplitRec*>(planes + 64 * (int64_t)cx.im.blk_first);
    const uint8_t* seg = blob + sg.byte_off;
    const int g0 = cx.sub0 * SUB;
    {
        const uint4* global = reinterpret_cast<const uint4*>(blob + cx.im.src_off + offsetof(stm_jpeg_tables, huff));
        for (int i = lane; i < 4 * (int)sizeof(stm_jpeg_huff) / 16; i += GROUP) reinterpret_cast<uint4*>(s_huff)[i] = global[i];
        const int padded = (sg.nbytes + 15) & ~15;               // the blob holds the segment's bytes rounded up to 16
        for (int j = lane; j < STAGED / 16; j += GROUP) {
            const int rel = 16 * j;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (g0 + rel < padded) v = *reinterpret_cast<const uint4*>(seg + g0 + rel);
            uint32_t* d = reinterpret_cast<uint32_t*>(s_bytes + rel + (rel / SUB) * SKEW);
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
        }
    }
    cx.src.lds = s_bytes;
    cx.src.g0 = g0;
    cx.src.prev = g0 > 0 ? seg[g0 - 1] : 0;
    __syncthreads();
}

__global__ __launch_bounds__(GROUP) void jpeg_split_sync_kernel(const uint8_t* __restrict__ blob, const stm_jpeg_image* __restrict__ images, int n_images,
                                                                const stm_jpeg_segment* __restrict__ segments, int n_segments,
                                                                uint8_t* __restrict__ planes, int16_t* __restrict__ coef, int round, int last)
{
    __shared__ __attribute__((aligned(16))) stm_jpeg_huff s_huff[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[LDS_BYTES];
    __shared__ uint32_t s_x[GROUP];
    __shared__ int s_changed;
    GroupCtx cx;
    group_setup(cx, blob, images, n_images, segments, n_segments, planes, s_huff, s_bytes);
    const int lane = threadIdx.x, sub = cx.sub0 + lane;
    const bool live = sub < cx.n_sub;
    const int par = round & 1;
    JpegSplitNull none;
    uint32_t e = 0, x = 0, x_was = 0;
    if (round == 0) {
        // this group's slice of the image's coefficients, 16 bytes a lane
        const int64_t total = (int64_t)jpeg_image_blocks(cx.im) * 8, per = (total + cx.n_groups - 1) / cx.n_groups;
        const int64_t begin = per * cx.group, end = begin + per < total ? begin + per : total;
        uint4* z = reinterpret_cast<uint4*>(coef + 64 * (int64_t)cx.im.blk_first);
        for (int64_t i = begin + lane; i < end; i += GROUP) z[i] = make_uint4(0u, 0u, 0u, 0u);
        if (live) {
            e = sub == 0 ? 0u : jpeg_split_guess(cx.src, cx.nbytes, sub);          // sub-sequence 0: the true state, which packs to 0
            x = jpeg_split_run(cx.src, cx.nbytes, s_huff, cx.n0, cx.bpm, cx.tsel, sub, e, none);
        }
    } else if (live) {
        const uint32_t e_was = cx.rec[sub].e[par ^ 1];
        x = x_was = cx.rec[sub].x[par ^ 1];
        e = sub == 0 ? 0u : cx.rec[sub - 1].x[par ^ 1];                            // the round before: of another group, for lane 0
        if (e != e_was) x = jpeg_split_run(cx.src, cx.nbytes, s_huff, cx.n0, cx.bpm, cx.tsel, sub, e, none);
    }
    // the repair inside the group: lane j is final after j turns at the latest
    for (int it = 0; it < GROUP; ++it) {
        s_x[lane] = x;
        if (lane == 0) s_changed = 0;
        __syncthreads();
        if (live && lane > 0 && s_x[lane - 1] != e) {
            e = s_x[lane - 1];
            x = jpeg_split_run(cx.src, cx.nbytes, s_huff, cx.n0, cx.bpm, cx.tsel, sub, e, none);
            s_changed = 1;
        }
        __syncthreads();
        const int any = s_changed;
        __syncthreads();
        if (!any) break;
    }
    if (!live) return;
    cx.rec[sub].e[par] = e;
    cx.rec[sub].x[par] = x;
    if (round == 0 && sub == 0) cx.rec[0].redo = 0;
    if (last) {
        if (x != x_was) cx.rec[0].redo = 1;
        JpegSplitCount cnt = {0, 0, 0, 0};
        jpeg_split_run(cx.src, cx.nbytes, s_huff, cx.n0, cx.bpm, cx.tsel, sub, e, cnt);
        cx.rec[sub].blocks = cnt.blocks;
        cx.rec[sub].dc[0] = (int16_t)cnt.d0;
        cx.rec[sub].dc[1] = (int16_t)cnt.d1;
        cx.rec[sub].dc[2] = (int16_t)cnt.d2;
    }
}

constexpr int SCAN_THREADS = 256;

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_scan_kernel(const stm_jpeg_image* __restrict__ images, const stm_jpeg_segment* __restrict__ segments,
                                                                        int n_segments, uint8_t* __restrict__ planes)
{
    __shared__ int s_v[4][SCAN_THREADS];
    const int img = blockIdx.x, t = threadIdx.x;
    const stm_jpeg_image im = images[img];
    if (!(im.split & 1)) return;
    int lo = 0, hi = n_segments - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segments[mid].image < img) lo = mid + 1;
        else hi = mid;
    }
    const stm_jpeg_segment sg = segments[lo];
    const int n_sub = jpeg_split_subs(sg.nbytes);
    JpegSplitRec* rec = reinterpret_cast<JpegSplitRec*>(planes + 64 * (int64_t)im.blk_first);
    int carry[4] = {0, 0, 0, 0};
    for (int t0 = 0; t0 < n_sub; t0 += SCAN_THREADS) {
        const int i = t0 + t;
        int v[4] = {0, 0, 0, 0};
        if (i < n_sub) {
            v[0] = rec[i].blocks;
            v[1] = rec[i].dc[0];
            v[2] = rec[i].dc[1];
            v[3] = rec[i].dc[2];
        }
        int sum[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) s_v[q][t] = sum[q] = v[q];
        __syncthreads();
        for (int o = 1; o < SCAN_THREADS; o <<= 1) {
            int add[4] = {0, 0, 0, 0};
            if (t >= o) {
#pragma unroll
                for (int q = 0; q < 4; ++q) add[q] = s_v[q][t - o];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) s_v[q][t] = sum[q] = (int)((unsigned)sum[q] + (unsigned)add[q]);
            __syncthreads();
        }
        if (i < n_sub) {
            rec[i].blocks = (int)((unsigned)carry[0] + (unsigned)sum[0] - (unsigned)v[0]);
            rec[i].dc[0] = (int16_t)((unsigned)carry[1] + (unsigned)sum[1] - (unsigned)v[1]);
            rec[i].dc[1] = (int16_t)((unsigned)carry[2] + (unsigned)sum[2] - (unsigned)v[2]);
            rec[i].dc[2] = (int16_t)((unsigned)carry[3] + (unsigned)sum[3] - (unsigned)v[3]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) carry[q] = (int)((unsigned)carry[q] + (unsigned)s_v[q][SCAN_THREADS - 1]);
        __syncthreads();
    }
    // the data holds fewer blocks than the MCUs need (a count that wrapped is no better: it comes from a chain that did not converge)
    if (t == 0 && (carry[0] < 0 || (int64_t)carry[0] < (int64_t)sg.mcu_count * jpeg_blocks_per_mcu(im))) rec[0].redo = 1;
}

__global__ __launch_bounds__(GROUP) void jpeg_split_write_kernel(const uint8_t* __restrict__ blob, const stm_jpeg_image* __restrict__ images, int n_images,
                                                                 const stm_jpeg_segment* __restrict__ segments, int n_segments,
                                                                 uint8_t* __restrict__ planes, int16_t* __restrict__ coef, int par)
{
    __shared__ __attribute__((aligned(16))) stm_jpeg_huff s_huff[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[LDS_BYTES];
    GroupCtx cx;
    group_setup(cx, blob, images, n_images, segments, n_segments, planes, s_huff, s_bytes);
    const int sub = cx.sub0 + (int)threadIdx.x;
    if (sub >= cx.n_sub || cx.rec[0].redo) return;           // (the mark is of an earlier launch: the serial kernel will write every block)
    const JpegSplitRec* r = cx.rec + sub;
    const uint32_t e = r->e[par];
    JpegSplitWrite w;
    w.coef = coef;
    w.first = cx.im.blk_first;
    w.hs = cx.im.hs;
    w.vs = cx.im.vs;
    w.mcu_w = cx.im.mcu_w;
    w.mcu_h = cx.im.mcu_h;
    w.mcu_first = 0;
    w.n0 = cx.n0;
    w.bpm = cx.bpm;
    w.expected = cx.im.mcu_w * cx.im.mcu_h * cx.bpm;
    w.seq = r->blocks;
    w.preds = (uint64_t)(uint16_t)r->dc[0] | ((uint64_t)(uint16_t)r->dc[1] << 16) | ((uint64_t)(uint16_t)r->dc[2] << 32);
    w.bad = 0;
    const JpegSplitState st = jpeg_split_unpack(e, sub * SUB, cx.bpm);
    w.open(st.k ? w.seq - 1 : -1, st.u);                     // the block the lane enters in the middle of, if any
    jpeg_split_run(cx.src, cx.nbytes, s_huff, cx.n0, cx.bpm, cx.tsel, sub, e, w);
    if (w.bad) cx.rec[0].redo = 1;
}

}  // namespace

// Launch 1 for the split images of a checked batch: STM_JPEG_SPLIT_LAUNCHES - 1 launches; the serial kernel, told of `planes`, follows.
int jpeg_split_launch(const uint8_t* blob, const stm_jpeg_image* d_images, int n_images, const stm_jpeg_segment* d_segments, int n_segments,
                      int total_groups, uint8_t* planes, int16_t* coef, hipStream_t stream)
{
    for (int round = 0; round <= STM_JPEG_SPLIT_ROUNDS; ++round) {
        hipLaunchKernelGGL(jpeg_split_sync_kernel, dim3((unsigned)total_groups), dim3(GROUP), 0, stream, blob, d_images, n_images, d_segments, n_segments,
                           planes, coef, round, (int)(round == STM_JPEG_SPLIT_ROUNDS));
        STM_CHECK_LAUNCH("jpeg_split_sync_kernel");
    }
    hipLaunchKernelGGL(jpeg_split_scan_kernel, dim3((unsigned)n_images), dim3(SCAN_THREADS), 0, stream, d_images, d_segments, n_segments, planes);
    STM_CHECK_LAUNCH("jpeg_split_scan_kernel");
    hipLaunchKernelGGL(jpeg_split_write_kernel, dim3((unsigned)total_groups), dim3(GROUP), 0, stream, blob, d_images, n_images, d_segments, n_segments, planes,
                       coef, STM_JPEG_SPLIT_ROUNDS & 1);
    STM_CHECK_LAUNCH("jpeg_split_write_kernel");
    return STM_OK;
}
