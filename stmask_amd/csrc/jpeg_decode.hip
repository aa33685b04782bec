// jpeg_decode.hip -- baseline JPEG frames decoded on gfx950 (MI355X), csrc/jpeg.h (package-private, stmask_amd/jpeg.py).  The arithmetic is
// csrc/jpeg_core.h; this file is how it is spread over the machine.
//
//   jpeg_entropy_kernel   one wavefront (one 64-thread workgroup) per restart interval.  Huffman decoding is serial, so the wave runs it
//                         wave-uniformly: every lane holds the same bit buffer, position and prediction (JPEG_UNIFORM tells the compiler so of
//                         the values read from LDS), nothing diverges.  The lanes share the rest of the work: they stage the segment into LDS 1 KiB
//                         at a time with one 16-byte load each and hold the 64 bytes being read one a lane, so a byte is a v_readlane, not an LDS
//                         round trip; the first-level lookups of the image's four Huffman tables sit in 4 registers a lane each (1 KiB a table),
//                         read the same way, and the tables' canonical part for longer codes in LDS; and lane n keeps coefficient n (natural
//                         order) of the current block in a register -- it takes the value when the symbol of its zig-zag position is decoded --
//                         so a finished block leaves as one 128-byte store, 2 bytes a lane, and never passes through LDS or scratch.
//                         A malformed segment sets its status word and writes zero blocks from there on.  Parallel decoding INSIDE one segment
//                         (self-synchronising sub-sequences) is csrc/jpeg_split.hip, for the images marked split; its launches come first,
//                         and for the segment of such an image this kernel returns at once unless they marked it REDO (record 0 of the
//                         image's plane region), in which case it decodes the segment as any other and says so in the status word.
//   jpeg_idct_kernel      8 lanes per 8x8 block.  Lane j loads row j of the coefficients (16 bytes) and of the quantisation table, multiplies and
//                         parks the row in LDS; then it runs the column pass over column j in place, the row pass over row j, and stores the 8
//                         samples of row j as 8 bytes.  int32 throughout.
//   jpeg_colour_kernel    one lane per 4 pixels of the frame's flat pixel list: chroma upsampling and YCbCr per pixel, 12 bytes stored as three
//                         dwords (frames start 16-byte aligned, so every store is aligned; rows follow one another without gaps).  Images the
//                         host decoded (STM_JPEG_RAW) are copied from the blob the same 12 bytes at a time.
//
// No atomics; every result is written with vector stores.  The image of a block or pixel group is found by binary search over the descriptors'
// blk_first / quad_first in device memory.
#include "stm_common.h"
#include "jpeg_split_core.h"

// csrc/jpeg_split.hip: the launches in front of jpeg_entropy_kernel for a batch with split images
int jpeg_split_launch(const uint8_t* blob, const stm_jpeg_image* d_images, int n_images, const stm_jpeg_segment* d_segments, int n_segments,
                      int total_groups, uint8_t* planes, int16_t* coef, hipStream_t stream);

namespace {

constexpr int JPEG_STAGE = 1024;                       // bytes of a segment in LDS at a time
// the canonical part of a Huffman table (what decodes the codes longer than the first-level lookup), as it lies behind `look` in stm_jpeg_huff
struct HuffRest {
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t huffval[256];
};
constexpr int JPEG_REST_OFF = (int)offsetof(stm_jpeg_huff, maxcode);
static_assert(sizeof(HuffRest) == sizeof(stm_jpeg_huff) - JPEG_REST_OFF && offsetof(HuffRest, valoff) == offsetof(stm_jpeg_huff, valoff) - JPEG_REST_OFF &&
                  offsetof(HuffRest, huffval) == offsetof(stm_jpeg_huff, huffval) - JPEG_REST_OFF, "HuffRest is the tail of stm_jpeg_huff");
static_assert(sizeof(stm_jpeg_huff) % 16 == 0 && sizeof(stm_jpeg_tables) % 16 == 0 && offsetof(stm_jpeg_tables, huff) % 16 == 0 && JPEG_REST_OFF % 16 == 0 &&
                  sizeof(HuffRest) % 16 == 0, "16-byte loads");
static_assert(sizeof(stm_jpeg_image) == 96 && sizeof(stm_jpeg_segment) == 24, "the descriptors as stmask_amd/_lib.py mirrors them");

// the segment's bytes through a 1 KiB window in LDS and, of that, 64 bytes one a lane; every lane asks for the same byte
struct LdsSource {
    const uint8_t* seg;     // 16-byte aligned
    uint8_t* win;
    int nbytes;
    int base;               // first byte of the window, -JPEG_STAGE before the first load
    int cbase;              // first byte of the 64 in `cur`, -64 before the first
    int cur;                // byte cbase + lane

    __device__ __forceinline__ int get(int pos)
    {
        if ((unsigned)(pos - cbase) >= 64u) {
            if ((unsigned)(pos - base) >= (unsigned)JPEG_STAGE) {
                base = pos & ~(JPEG_STAGE - 1);
                __syncthreads();                                     // (one wave: orders the window's reads before its next writes)
                const int o = base + 16 * (int)threadIdx.x;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (o < nbytes) v = *reinterpret_cast<const uint4*>(seg + o);      // the blob holds nbytes rounded up to 16
                reinterpret_cast<uint4*>(win)[threadIdx.x] = v;
                __syncthreads();
            }
            cbase = pos & ~63;
            cur = win[cbase - base + (int)threadIdx.x];
        }
        return __builtin_amdgcn_readlane(cur, pos & 63);
    }
};

// One Huffman table as the wave holds it: the first-level lookup in 4 registers a lane -- entry i in register i >> 7, lane (i >> 1) & 63, half
// i & 1 -- and the canonical part in LDS.
struct LaneHuff {
    uint32_t first[4];
    const HuffRest* rest;

    __device__ __forceinline__ void load(const stm_jpeg_huff* global, const HuffRest* lds, int lane)
    {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(global->look);
#pragma unroll
        for (int r = 0; r < 4; ++r) first[r] = w[64 * r + lane];
        rest = lds;
    }
    __device__ __forceinline__ int look(unsigned i) const
    {
        const unsigned r = i >> 7;
        const uint32_t v = r == 0 ? first[0] : (r == 1 ? first[1] : (r == 2 ? first[2] : first[3]));
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)((i >> 1) & 63));
        return (int)((i & 1) ? w >> 16 : w & 0xFFFFu);
    }
    __device__ __forceinline__ int maxcode(int l) const { return JPEG_UNIFORM(rest->maxcode[l]); }
    __device__ __forceinline__ int valoff(int l) const { return JPEG_UNIFORM(rest->valoff[l]); }
    __device__ __forceinline__ int huffval(int i) const { return JPEG_UNIFORM(rest->huffval[i]); }
};

// lane n's coefficient of the block being decoded; myk: the zig-zag position of natural index n
struct LaneSink {
    int myk;
    int mine;
    __device__ __forceinline__ void put(int k, int v)
    {
        if (k == myk) mine = v;
    }
};

__global__ __launch_bounds__(STM_WAVE) void jpeg_entropy_kernel(const uint8_t* __restrict__ blob, const stm_jpeg_image* __restrict__ images,
                                                                const stm_jpeg_segment* __restrict__ segments, int n_segments,
                                                                int16_t* __restrict__ coef, int* __restrict__ status,
                                                                const uint8_t* __restrict__ split_planes)     // null: no image of the batch is split
{
    __shared__ __attribute__((aligned(16))) HuffRest s_rest[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_win[JPEG_STAGE];
    const int s = blockIdx.x;
    if (s >= n_segments) return;
    const int lane = threadIdx.x;
    const stm_jpeg_segment sg = segments[s];
    const stm_jpeg_image im = images[sg.image];
    int redone = 0;
    if (split_planes && (im.split & 1)) {
        if (!reinterpret_cast<const JpegSplitRec*>(split_planes + 64 * (int64_t)im.blk_first)->redo) {
            if (lane == 0) status[s] = 0;
            return;
        }
        redone = STM_JPEG_REDONE;
    }
    const stm_jpeg_huff* global = reinterpret_cast<const stm_jpeg_huff*>(blob + im.src_off + offsetof(stm_jpeg_tables, huff));
    {
        constexpr int PER = (int)sizeof(HuffRest) / 16;                        // 16-byte pieces of one table's canonical part
        for (int i = lane; i < 4 * PER; i += STM_WAVE) {
            const int k = i / PER, j = i - k * PER;
            reinterpret_cast<uint4*>(s_rest + k)[j] = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(global + k) + JPEG_REST_OFF)[j];
        }
    }
    __syncthreads();
    LaneHuff tab[4];                                                           // DC 0, DC 1, AC 0, AC 1
#pragma unroll
    for (int k = 0; k < 4; ++k) tab[k].load(global + k, s_rest + k, lane);
    int myk = 0;                                                               // jpeg_natural(myk) == lane
    for (int k = 0; k < 64; ++k)
        if (jpeg_natural(k) == lane) myk = k;
    LdsSource src{blob + sg.byte_off, s_win, sg.nbytes, -JPEG_STAGE, -64, 0};
    JpegBits<LdsSource> br(src, sg.nbytes);
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int err = 0;
    const int mcu_w = im.mcu_w;
    int my = sg.mcu_first / mcu_w, mx = sg.mcu_first - my * mcu_w;
    for (int m = 0; m < sg.mcu_count; ++m) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= im.ncomp) break;
            const int hs = jpeg_comp_hs(im, c), vs = jpeg_comp_vs(im, c), bw = mcu_w * hs;
            const LaneHuff dc = im.td[c] ? tab[1] : tab[0];
            const LaneHuff ac = im.ta[c] ? tab[3] : tab[2];
            int& pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
            const int64_t first = (int64_t)im.blk_first + jpeg_comp_first(im, c);
            for (int by = 0; by < vs; ++by) {
                for (int bx = 0; bx < hs; ++bx) {
                    LaneSink sink{myk, 0};
                    if (!err) {
                        err = jpeg_decode_block(br, dc, ac, pred, sink);
                        if (err) sink.mine = 0;
                    }
                    const int64_t blk = first + (int64_t)(my * vs + by) * bw + (mx * hs + bx);
                    coef[blk * 64 + lane] = (int16_t)sink.mine;
                }
            }
        }
        if (++mx == mcu_w) {
            mx = 0;
            ++my;
        }
    }
    if (lane == 0) status[s] = err | redone;
}

// the image of batch-wide index g: the last one whose first index (a field of the descriptor) is <= g.  Images without blocks share their first
// index with the next image and are passed over unless they are last, and g never reaches those.
template <int32_t stm_jpeg_image::*FIRST>
__device__ __forceinline__ int jpeg_find(const stm_jpeg_image* __restrict__ images, int n_images, int g)
{
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (images[mid].*FIRST <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

constexpr int IDCT_THREADS = 256;
constexpr int IDCT_LD = 9;                  // ints per parked row: the column reads of 8 lanes fall on 8 banks

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const uint8_t* __restrict__ blob, const stm_jpeg_image* __restrict__ images,
                                                                 int n_images, int total_blocks, const int16_t* __restrict__ coef,
                                                                 uint8_t* __restrict__ planes)
{
    __shared__ int32_t s_blk[IDCT_THREADS / 8][8 * IDCT_LD];
    const int64_t t = (int64_t)blockIdx.x * IDCT_THREADS + threadIdx.x;
    const int g = (int)(t >> 3), j = (int)(t & 7);
    const bool live = g < total_blocks;
    int32_t* tile = s_blk[threadIdx.x >> 3];
    const stm_jpeg_image& im = images[live ? jpeg_find<&stm_jpeg_image::blk_first>(images, n_images, g) : 0];     // (read in place: no private copy)
    int b = 0, c = 0;
    if (live) {
        b = g - im.blk_first;
        const int n0 = jpeg_comp_first(im, 1);
        if (b >= n0) {
            c = 1 + (b - n0) / (im.mcu_w * im.mcu_h);
            b -= jpeg_comp_first(im, c);
        }
        const uint4 raw = *reinterpret_cast<const uint4*>(coef + (int64_t)g * 64 + 8 * j);
        const uint4 qraw = *reinterpret_cast<const uint4*>(blob + im.src_off + 128 * im.tq[c] + 16 * j);
        const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {qraw.x, qraw.y, qraw.z, qraw.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tile[j * IDCT_LD + 2 * i] = (int32_t)(int16_t)(rw[i] & 0xFFFFu) * (int32_t)(qw[i] & 0xFFFFu);
            tile[j * IDCT_LD + 2 * i + 1] = (int32_t)(int16_t)(rw[i] >> 16) * (int32_t)(qw[i] >> 16);
        }
    }
    __syncthreads();
    int32_t in[8], out[8];
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = tile[r * IDCT_LD + j];
        jpeg_idct8(in, out, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) tile[r * IDCT_LD + j] = out[r];          // column j is this lane's alone: in place
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = tile[j * IDCT_LD + r];
        jpeg_idct8(in, out, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            lo |= (uint32_t)jpeg_sample(out[r]) << (8 * r);
            hi |= (uint32_t)jpeg_sample(out[4 + r]) << (8 * r);
        }
        const int bw = jpeg_comp_bw(im, c);
        const int by = b / bw, bx = b - by * bw;
        uint8_t* plane = planes + 64 * ((int64_t)im.blk_first + jpeg_comp_first(im, c));
        *reinterpret_cast<uint2*>(plane + ((int64_t)(by * 8 + j) * bw + bx) * 8) = make_uint2(lo, hi);
    }
}

constexpr int COLOUR_THREADS = 256;

__global__ __launch_bounds__(COLOUR_THREADS) void jpeg_colour_kernel(const uint8_t* __restrict__ blob, const stm_jpeg_image* __restrict__ images,
                                                                     int n_images, int total_quads, const uint8_t* __restrict__ planes,
                                                                     uint8_t* __restrict__ out, int bgr)
{
    const int64_t t = (int64_t)blockIdx.x * COLOUR_THREADS + threadIdx.x;
    if (t >= total_quads) return;
    const int q = (int)t;
    const stm_jpeg_image im = images[jpeg_find<&stm_jpeg_image::quad_first>(images, n_images, q)];
    const int i = q - im.quad_first;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + im.out_off) + 3 * (int64_t)i;
    uint32_t w0, w1, w2;
    if (im.kind == STM_JPEG_RAW) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(blob + im.src_off) + 3 * (int64_t)i;
        w0 = src[0];
        w1 = src[1];
        w2 = src[2];
    } else {
        const uint8_t* pl = planes + 64 * (int64_t)im.blk_first;
        const int n = im.width * im.height;
        int y = (4 * i) / im.width, x = 4 * i - y * im.width;
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = 0;
            if (4 * i + k < n) {
                int r, g, b;
                jpeg_pixel(im, pl, x, y, r, g, b);
                px[k] = bgr ? ((uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16)) : ((uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16));
                if (++x == im.width) {
                    x = 0;
                    ++y;
                }
            }
        }
        w0 = px[0] | (px[1] << 24);
        w1 = (px[1] >> 8) | (px[2] << 16);
        w2 = (px[2] >> 16) | (px[3] << 8);
    }
    dst[0] = w0;
    dst[1] = w1;
    dst[2] = w2;
}

}  // namespace

extern "C" size_t stm_jpeg_struct_bytes(int which)
{
    return which == 0 ? sizeof(stm_jpeg_image) : which == 1 ? sizeof(stm_jpeg_segment) : which == 2 ? sizeof(stm_jpeg_tables) : 0;
}

extern "C" size_t stm_jpeg_workspace_bytes(const stm_jpeg_image* images, int n_images)
{
    if (!images || n_images <= 0) return 0;
    int64_t blocks = 0;
    for (int i = 0; i < n_images; ++i) {
        if (jpeg_image_reason(images[i])) return 0;
        blocks += jpeg_image_blocks(images[i]);
    }
    return (size_t)blocks * 192;
}

extern "C" int stm_jpeg_decode_u8(const stm_jpeg_image* images, int n_images, const stm_jpeg_segment* segments, int n_segments, const void* blob,
                                  size_t blob_bytes, size_t images_off, size_t segments_off, void* out, size_t out_bytes, int* status,
                                  void* workspace, size_t workspace_bytes, int bgr, int stages, stm_stream_t stream)
{
    const char* who = "stm_jpeg_decode_u8";
    STM_REQUIRE(n_images >= 0 && n_segments >= 0, STM_EINVAL, "%s: n_images=%d n_segments=%d", who, n_images, n_segments);
    if (n_images == 0) {
        STM_REQUIRE(n_segments == 0, STM_EINVAL, "%s: %d segments and no image", who, n_segments);
        return STM_OK;
    }
    STM_REQUIRE(images && blob && out, STM_EINVAL, "%s: images, blob and out must be non-NULL for %d images", who, n_images);
    STM_REQUIRE(n_segments == 0 || (segments && status), STM_EINVAL, "%s: segments and status must be non-NULL for %d segments", who, n_segments);
    STM_REQUIRE(stm_aligned16(blob) && stm_aligned16(out) && stm_aligned16(workspace), STM_EINVAL, "%s: blob, out and workspace must be 16-byte aligned",
                who);
    STM_REQUIRE(images_off % 16 == 0 && segments_off % 8 == 0 && images_off <= blob_bytes &&
                    (size_t)n_images * sizeof(stm_jpeg_image) <= blob_bytes - images_off && segments_off <= blob_bytes &&
                    (size_t)n_segments * sizeof(stm_jpeg_segment) <= blob_bytes - segments_off,
                STM_EINVAL, "%s: the descriptors at %zu and %zu do not lie inside the blob of %zu bytes", who, images_off, segments_off, blob_bytes);
    int64_t total_blocks = 0, total_quads = 0;
    const char* why = "";
    int which = 0;
    const int rc = jpeg_check_batch(images, n_images, segments, n_segments, blob_bytes, out_bytes, &total_blocks, &total_quads, &why, &which);
    STM_REQUIRE(rc == STM_OK, rc, "%s: image or segment %d has %s", who, which, why);
    STM_REQUIRE(total_blocks == 0 || workspace, STM_EINVAL, "%s: workspace must be non-NULL", who);
    STM_REQUIRE((uint64_t)total_blocks * 192 <= workspace_bytes, STM_EWORKSPACE, "%s: workspace of %zu bytes, %lld needed", who, workspace_bytes,
                (long long)total_blocks * 192);
    const uint8_t* b8 = static_cast<const uint8_t*>(blob);
    const stm_jpeg_image* d_images = reinterpret_cast<const stm_jpeg_image*>(b8 + images_off);
    const stm_jpeg_segment* d_segments = reinterpret_cast<const stm_jpeg_segment*>(b8 + segments_off);
    int16_t* coef = static_cast<int16_t*>(workspace);
    uint8_t* planes = static_cast<uint8_t*>(workspace) + 128 * total_blocks;
    if ((stages & STM_JPEG_STAGE_ENTROPY) && n_segments) {
        const int total_groups = (int)jpeg_total_groups(images, n_images, segments, n_segments);
        if (total_groups) {
            const int rs = jpeg_split_launch(b8, d_images, n_images, d_segments, n_segments, total_groups, planes, coef, stm_hs(stream));
            if (rs != STM_OK) return rs;
        }
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_segments), dim3(STM_WAVE), 0, stm_hs(stream), b8, d_images, d_segments, n_segments, coef,
                           status, total_groups ? planes : nullptr);
        STM_CHECK_LAUNCH("jpeg_entropy_kernel");
    }
    if ((stages & STM_JPEG_STAGE_IDCT) && total_blocks) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)stm_cdiv(total_blocks * 8, IDCT_THREADS)), dim3(IDCT_THREADS), 0, stm_hs(stream), b8, d_images,
                           n_images, (int)total_blocks, coef, planes);
        STM_CHECK_LAUNCH("jpeg_idct_kernel");
    }
    if (stages & STM_JPEG_STAGE_COLOUR) {
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)stm_cdiv(total_quads, COLOUR_THREADS)), dim3(COLOUR_THREADS), 0, stm_hs(stream), b8, d_images,
                           n_images, (int)total_quads, planes, static_cast<uint8_t*>(out), bgr);
        STM_CHECK_LAUNCH("jpeg_colour_kernel");
    }
    return STM_OK;
}
