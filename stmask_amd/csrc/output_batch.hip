// output_batch.hip -- the output stage of a whole step in a fixed number of launches (include/stmask_hip_output.h): every tracked row of every
// frame goes from soft mask to finished COCO RLE string, pixel box, score, class and id, into one device buffer (header | row records |
// string arena) that the host copies once.  output.hip does the same for the rows of ONE frame and leaves the string packing to the host;
// here every row carries its frame's sizes, and the strings are packed on the device too:
//   1. select + boxes, one thread per row: postprocess_ytbvis's row rule and pixel_boxes in torch's own fp32 operation sequence
//      (tensor / python_float multiplies by the fp32 reciprocal; a comparison rounds the Python float to fp32); writes the row's record and
//      its frame geometry.  The frame descriptors travel in the kernel argument, 64 frames per launch;
//   2. resize + threshold + bit-pack of the kept rows (stm_bilinear_tap / stm_bilinear_blend, column-major, one ballot per 64 pixels);
//   3. run extraction, one workgroup per kept row (rle_common.h), which also sums the row's string length;
//   4. exclusive sum of the string lengths in row order (one workgroup) -> every row's place in the arena, the header;
//   5. string packing, one workgroup per row: characters per run, workgroup scan, characters written in place.
// Integer and fp32 arithmetic only, no atomics: the buffer is the same bytes at every run.
#include "../../include/stmask_hip_output.h"
#include "rle_common.h"
#include <algorithm>

namespace {

constexpr int kMultiFrames = 64;
struct OutputFramesArg {
    stm_output_frame f[kMultiFrames];
};

struct RowGeom {
    int crop_h, crop_w, out_h, out_w;
};

__device__ __forceinline__ int load_index(const void* p, int is_i64, int r)
{
    return is_i64 ? (int)reinterpret_cast<const long long*>(p)[r] : reinterpret_cast<const int*>(p)[r];
}

__device__ __forceinline__ int trunc_to_int(float v)
{
    const long long t = (long long)v;                       // .long(): truncation towards zero
    return (int)(t < -2147483647LL - 1 ? -2147483647LL - 1 : (t > 2147483647LL ? 2147483647LL : t));
}

// stage 1.  This launch owns the rows whose frame lies in [f0, f0 + k); the first launch (f0 == 0) also owns the rows whose frame is no frame.
__global__ __launch_bounds__(256) void select_boxes_kernel(const OutputFramesArg a, int f0, int k, int n_frames, int n,
                                                           const int* __restrict__ frame_of_row, const float* __restrict__ score,
                                                           const void* __restrict__ cls, int cls_is_i64, const void* __restrict__ box_id,
                                                           int box_id_is_i64, const float* __restrict__ box,
                                                           const uint8_t* __restrict__ row_keep, float score_threshold,
                                                           stm_output_row* __restrict__ rows, RowGeom* __restrict__ geom)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int f = frame_of_row[r];
    const bool bad = f < 0 || f >= n_frames;
    if (bad ? f0 != 0 : (f < f0 || f >= f0 + k)) return;
    stm_output_row o;
    o.frame = f;
    o.status = bad ? STM_ROW_BAD_FRAME : 0;
    o.n_runs = 0;
    o.str_off = 0;
    o.str_len = 0;
    o.cls = load_index(cls, cls_is_i64, r);
    o.box_id = load_index(box_id, box_id_is_i64, r);
    const float s = score[r];
    o.score_bits = __float_as_uint(s);
    o.box[0] = o.box[1] = o.box[2] = o.box[3] = 0;
    RowGeom g = {0, 0, 0, 0};
    if (!bad) {
        const stm_output_frame d = a.f[f - f0];
        const float x1 = box[4 * r + 0], y1 = box[4 * r + 1], x2 = box[4 * r + 2], y2 = box[4 * r + 3];
        bool keep = row_keep == nullptr || row_keep[r] != 0;
        if (score_threshold > 0.0f) keep = keep && s > score_threshold;
        // center_size: (box[:, 2:] + box[:, :2]) / 2, the division by 2 as torch's multiplication by 0.5f
        const float cx = (x2 + x1) * 0.5f, cy = (y2 + y1) * 0.5f;
        keep = keep && !(cx > d.s_w) && !(cy > d.s_h);
        if (keep) {
            o.status = STM_ROW_KEPT;
            float lo, hi;
            stm_sanitize(x1 * d.inv_s_w, x2 * d.inv_s_w, d.out_w, 0, lo, hi);
            o.box[0] = trunc_to_int(lo);
            o.box[2] = trunc_to_int(hi);
            stm_sanitize(y1 * d.inv_s_h, y2 * d.inv_s_h, d.out_h, 0, lo, hi);
            o.box[1] = trunc_to_int(lo);
            o.box[3] = trunc_to_int(hi);
            g.crop_h = d.crop_h; g.crop_w = d.crop_w; g.out_h = d.out_h; g.out_w = d.out_w;
        }
    }
    rows[r] = o;
    geom[r] = g;
}

// stage 2.  blockIdx.x = row; the workgroups of a row (gridDim.y of them) stride over its groups of 4 words, a wavefront makes one word.  Row r's
// words lie at bits[r * max_words ...].  (A grid of rows x groups workgroups in one dimension passes 2^32 threads at a few thousand 720p rows.)
__global__ __launch_bounds__(256) void resize_threshold_pack_rows_kernel(const float* __restrict__ masks, int mh, int mw,
                                                                         const stm_output_row* __restrict__ rows,
                                                                         const RowGeom* __restrict__ geom, float thr, int max_words,
                                                                         unsigned long long* __restrict__ bits)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x;
    if (!(rows[r].status & STM_ROW_KEPT)) return;
    const RowGeom g = geom[r];
    const int64_t n_px = (int64_t)g.out_h * g.out_w;
    const int words = (int)((n_px + 63) / 64);              // (<= max_words: max_words is the largest frame's)
    const float* m = masks + (int64_t)r * mh * mw;
    const float scale_h = (float)g.crop_h / (float)g.out_h, scale_w = (float)g.crop_w / (float)g.out_w;
    for (int word = blockIdx.y * 4 + wave; word < words; word += gridDim.y * 4) {   // (wave-uniform: the ballot sees whole wavefronts)
        const int64_t p = (int64_t)word * 64 + lane;        // column-major pixel index: p = x * out_h + y
        bool b = false;
        if (p < n_px) {
            const int x = (int)(p / g.out_h), y = (int)(p - (int64_t)x * g.out_h);
            int y0, y1, x0, x1;
            float ly, hy, lx, hx;
            stm_bilinear_tap(y, scale_h, g.crop_h, y0, y1, ly, hy);
            stm_bilinear_tap(x, scale_w, g.crop_w, x0, x1, lx, hx);
            b = stm_bilinear_blend(m, mw, y0, y1, x0, x1, ly, hy, lx, hx) > thr;
        }
        const unsigned long long bal = __ballot(b);
        if (lane == 0) bits[(int64_t)r * max_words + word] = bal;
    }
}

// stage 3.  One workgroup of 1024 per row.
__global__ __launch_bounds__(1024) void rle_runs_rows_kernel(const unsigned long long* __restrict__ bits, int max_words,
                                                             stm_output_row* __restrict__ rows, const RowGeom* __restrict__ geom,
                                                             unsigned int* __restrict__ counts, unsigned int* __restrict__ trans_ws,
                                                             int max_runs)
{
    __shared__ int wave_tot[16];
    __shared__ int len_tot[16];
    const int r = blockIdx.x;
    if (!(rows[r].status & STM_ROW_KEPT)) return;           // (uniform over the workgroup)
    const RowGeom g = geom[r];
    const int64_t n_px = (int64_t)g.out_h * g.out_w;
    const int words = (int)((n_px + 63) / 64);
    unsigned int* cnt = counts + (int64_t)r * max_runs;
    const int nr = stm_rle_runs_block(bits + (int64_t)r * max_words, words, n_px, trans_ws + (int64_t)r * max_runs, cnt, max_runs, wave_tot);
    if (nr > max_runs) {
        if (threadIdx.x == 0) {
            rows[r].n_runs = nr;
            rows[r].status |= STM_ROW_RUN_OVERFLOW;
        }
        return;
    }
    __threadfence_block();
    __syncthreads();                                        // the counts of the other threads
    int len = 0;
    for (int j = threadIdx.x; j < nr; j += 1024) len += stm_rle_chars(stm_rle_value(cnt, j), nullptr);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d);
    if ((threadIdx.x & 63) == 0) len_tot[threadIdx.x >> 6] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < 16; ++w) total += len_tot[w];
        rows[r].n_runs = nr;
        rows[r].str_len = total;
    }
}

// stage 4.  One workgroup of 1024: str_off = exclusive sum of str_len in row order; rows whose string would end past the arena are marked.
__global__ __launch_bounds__(1024) void string_offsets_kernel(stm_output_row* __restrict__ rows, int n, int arena_bytes,
                                                              stm_output_header* __restrict__ header)
{
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int base = 0;
    for (int r0 = 0; r0 < n; r0 += 1024) {
        const int r = r0 + tid;
        const int v = r < n ? rows[r].str_len : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(incl, off, 64);
            if (lane >= off) incl += u;
        }
        __syncthreads();                                    // wave_tot of the previous round has been read
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wave_tot[w];
            total += wave_tot[w];
        }
        if (r < n) {
            const int off = base + before + incl - v;
            rows[r].str_off = off;
            if (v > 0 && off + v > arena_bytes) rows[r].status |= STM_ROW_ARENA_OVERFLOW;
        }
        base += total;
    }
    if (tid == 0) {
        header->n_rows = n;
        header->total_bytes = base;
        header->arena_bytes = arena_bytes;
        header->reserved = 0;
    }
}

// stage 5.  One workgroup of 256 per row: 256 runs per round, their character counts scanned, the characters written at their place.
__global__ __launch_bounds__(256) void pack_strings_kernel(const stm_output_row* __restrict__ rows, const unsigned int* __restrict__ counts,
                                                           int max_runs, unsigned char* __restrict__ arena, int arena_bytes)
{
    __shared__ unsigned sw[4];
    const stm_output_row o = rows[blockIdx.x];
    if (!(o.status & STM_ROW_KEPT) || (o.status & (STM_ROW_RUN_OVERFLOW | STM_ROW_ARENA_OVERFLOW)) || o.str_len <= 0) return;
    const unsigned int* cnt = counts + (int64_t)blockIdx.x * max_runs;
    const int nr = min(o.n_runs, max_runs);
    const int end = min(o.str_off + o.str_len, arena_bytes);
    unsigned base = 0;
    for (int j0 = 0; j0 < nr; j0 += 256) {
        const int j = j0 + threadIdx.x;
        unsigned char ch[13];
        const int k = j < nr ? stm_rle_chars(stm_rle_value(cnt, j), ch) : 0;
        unsigned total;
        const unsigned pos = stm_block_excl_scan((unsigned)k, sw, total);
        const int at = o.str_off + (int)(base + pos);
        for (int i = 0; i < k; ++i)
            if (at + i < end) arena[at + i] = ch[i];
        base += total;
    }
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t stm_output_struct_bytes(int which)
{
    switch (which) {
        case 0: return sizeof(stm_output_frame);
        case 1: return sizeof(stm_output_row);
        case 2: return sizeof(stm_output_header);
        default: return 0;
    }
}

extern "C" size_t stm_output_stage_workspace_bytes(int n, int64_t max_out_px, int max_runs)
{
    if (n <= 0 || max_out_px <= 0 || max_runs <= 0) return 0;
    const size_t words = ((size_t)max_out_px + 63) / 64;
    return (size_t)n * words * 8 + align8((size_t)n * sizeof(RowGeom)) + 2 * align8((size_t)n * max_runs * 4) + 256;
}

extern "C" int stm_output_stage_multi_f32(const float* masks, int n, int mh, int mw, const int* frame_of_row, const float* score, const void* cls,
                                          int cls_is_i64, const void* box_id, int box_id_is_i64, const float* box, const uint8_t* row_keep,
                                          const stm_output_frame* frames, int n_frames, float score_threshold, float thr, int max_runs, void* out,
                                          size_t out_bytes, void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_output_stage_multi_f32";
    STM_REQUIRE(n >= 0, STM_EINVAL, "%s: n=%d", who, n);
    if (n == 0) return STM_OK;
    STM_REQUIRE(masks && frame_of_row && score && cls && box_id && box && frames && out, STM_ENULL,
                "%s: masks / frame_of_row / score / cls / box_id / box / frames / out must be non-NULL", who);
    STM_REQUIRE(mh > 0 && mw > 0 && n_frames > 0 && max_runs > 0, STM_EINVAL, "%s: bad sizes mask=%dx%d n_frames=%d max_runs=%d", who, mh, mw,
                n_frames, max_runs);
    STM_REQUIRE((int64_t)n * max_runs * 7 < ((int64_t)1 << 31), STM_EINVAL, "%s: n * max_runs * 7 = %lld characters do not fit 31 bits", who,
                (long long)n * max_runs * 7);
    int64_t max_px = 0;
    for (int i = 0; i < n_frames; ++i) {
        const stm_output_frame& d = frames[i];
        STM_REQUIRE(d.crop_h > 0 && d.crop_h <= mh && d.crop_w > 0 && d.crop_w <= mw, STM_EINVAL, "%s: frame %d: crop %dx%d outside the %dx%d mask", who,
                    i, d.crop_h, d.crop_w, mh, mw);
        STM_REQUIRE(d.out_h > 0 && d.out_w > 0 && (int64_t)d.out_h * d.out_w < ((int64_t)1 << 31), STM_EINVAL, "%s: frame %d: bad output size %dx%d", who,
                    i, d.out_h, d.out_w);
        max_px = (int64_t)d.out_h * d.out_w > max_px ? (int64_t)d.out_h * d.out_w : max_px;
    }
    const int max_words = (int)((max_px + 63) / 64);
    STM_REQUIRE(n <= (1 << 22), STM_EINVAL, "%s: n=%d rows exceed one grid", who, n);
    // workgroups of a row in stage 2: one per 4 words, but no more than 65535 and no more than 2^22 in the whole grid (they stride)
    const int groups = (int)std::min<int64_t>(std::min<int64_t>(stm_cdiv(max_words, 4), 65535), std::max<int64_t>(1, ((int64_t)1 << 22) / n));
    const size_t head = sizeof(stm_output_header) + (size_t)n * sizeof(stm_output_row);
    STM_REQUIRE(out_bytes >= head, STM_EWORKSPACE, "%s: out holds %zu bytes, header and %d records need %zu", who, out_bytes, n, head);
    STM_REQUIRE(workspace && workspace_bytes >= stm_output_stage_workspace_bytes(n, max_px, max_runs), STM_EWORKSPACE, "%s: workspace too small", who);
    STM_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 7) == 0, STM_EINVAL, "%s: out must be 4-byte, workspace 8-byte aligned", who);
    const size_t arena_cap = out_bytes - head;
    const int arena_bytes = (int)(arena_cap > 0x7fffffffu ? 0x7fffffffu : arena_cap);

    char* ws = reinterpret_cast<char*>(workspace);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(ws);
    ws += (size_t)n * max_words * 8;
    RowGeom* geom = reinterpret_cast<RowGeom*>(ws);
    ws += align8((size_t)n * sizeof(RowGeom));
    unsigned int* counts = reinterpret_cast<unsigned int*>(ws);
    ws += align8((size_t)n * max_runs * 4);
    unsigned int* trans = reinterpret_cast<unsigned int*>(ws);
    stm_output_header* header = reinterpret_cast<stm_output_header*>(out);
    stm_output_row* rows = reinterpret_cast<stm_output_row*>(header + 1);
    unsigned char* arena = reinterpret_cast<unsigned char*>(rows + n);
    hipStream_t hs = stm_hs(stream);

    for (int f0 = 0; f0 < n_frames; f0 += kMultiFrames) {
        const int k = min(kMultiFrames, n_frames - f0);
        OutputFramesArg a = {};
        for (int i = 0; i < k; ++i) a.f[i] = frames[f0 + i];
        hipLaunchKernelGGL(select_boxes_kernel, dim3(stm_cdiv(n, 256)), dim3(256), 0, hs, a, f0, k, n_frames, n, frame_of_row, score, cls,
                           cls_is_i64, box_id, box_id_is_i64, box, row_keep, score_threshold, rows, geom);
        STM_CHECK_LAUNCH("select_boxes_kernel");
    }
    hipLaunchKernelGGL(resize_threshold_pack_rows_kernel, dim3(n, groups), dim3(256), 0, hs, masks, mh, mw, rows, geom, thr, max_words, bits);
    STM_CHECK_LAUNCH("resize_threshold_pack_rows_kernel");
    hipLaunchKernelGGL(rle_runs_rows_kernel, dim3(n), dim3(1024), 0, hs, bits, max_words, rows, geom, counts, trans, max_runs);
    STM_CHECK_LAUNCH("rle_runs_rows_kernel");
    hipLaunchKernelGGL(string_offsets_kernel, dim3(1), dim3(1024), 0, hs, rows, n, arena_bytes, header);
    STM_CHECK_LAUNCH("string_offsets_kernel");
    hipLaunchKernelGGL(pack_strings_kernel, dim3(n), dim3(256), 0, hs, rows, counts, max_runs, arena, arena_bytes);
    STM_CHECK_LAUNCH("pack_strings_kernel");
    return STM_OK;
}
