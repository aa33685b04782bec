/* jpeg.h -- baseline JPEG frames decoded on the device (stmask_amd/jpeg.py: decode_batch), gfx950 (MI355X).
 *
 * Package-private: exported by libstmask_hip.so, restated in stmask_amd/_lib.py JPEG_SIGNATURES and bound on first use by _lib.private_call().
 * Not part of the drop-in boundary of include/ (a C client of that boundary hands over pixels), so STM_ABI_VERSION does not count these.
 *
 * The host reads the file and parses its markers (jpeg.py: parse); everything from the entropy-coded bits to the uint8 [H, W, 3] frame is done
 * here, in three launches for a batch of any size and any mix of sizes (more, a fixed number, when an image is split: below):
 *     1  entropy decode      one wavefront per (image, restart interval): Huffman symbols -> int16 coefficients in natural order
 *     2  dequantise + IDCT   libjpeg's `islow` integer transform, level shift, clamp -> uint8 component planes padded to whole MCUs
 *     3  upsample + colour   libjpeg's fancy h2v1 / h2v2 chroma upsampling and fixed-point YCbCr -> the interleaved frame, bgr or rgb
 * The arithmetic of all three is csrc/jpeg_core.h, which a host program can run as it stands.
 *
 * Everything the kernels read travels in ONE blob in device memory (one copy from pinned memory): the image descriptors, the segment
 * descriptors, the table sets (quantisation and Huffman, shared by the images that use equal ones), every entropy-coded segment (16-byte
 * aligned, a zero guard behind it) and the pixels of the files the host decoded itself (kind STM_JPEG_RAW, copied to their frame by launch 3).
 * The descriptors are not kernel arguments, so a batch has no frame limit.  The host copies of the descriptors are what the entry point checks
 * before it launches; the blob must hold the same bytes at images_off / segments_off.
 *
 * Supported: 8-bit baseline, Huffman, one interleaved scan; 1 component, or 3 (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; width
 * and height 1..8192.
 *
 * A file without restart markers is one segment, and one wavefront's work from its first bit to its last, unless its image is SPLIT
 * (stm_jpeg_image.split, opt-in; csrc/jpeg_split.hip, the arithmetic in csrc/jpeg_split_core.h).  A baseline Huffman stream re-synchronises a
 * few dozen symbols after a wrong start, so the segment is cut into sub-sequences of STM_JPEG_SUB_BYTES raw (still stuffed) bytes, each decoded
 * by a lane of its own from a guessed state; a sub-sequence owns the symbols whose first bit lies in it.  STM_JPEG_SUB_GROUP sub-sequences
 * make a group, one workgroup's work.  Launch 1 then becomes STM_JPEG_SPLIT_LAUNCHES launches, whatever the batch and its data:
 *     sync round 0            every lane decodes from its guess (sub-sequence 0 from the true state); inside the group each lane then decodes
 *                             again from its predecessor's exit state until no exit state of the group changes; the images' coefficients are
 *                             zeroed on the way
 *     sync rounds 1 .. R      R = STM_JPEG_SPLIT_ROUNDS: the same repair with the first lane of a group entering from the exit state the group
 *                             before it left in the round before, so a correction crosses one more group boundary per round.  The last round
 *                             counts, per sub-sequence, the blocks that start in it and their DC differences per component, and marks the
 *                             segment REDO when an exit state still changed: a segment whose last round changed nothing has, by induction from
 *                             sub-sequence 0, the true state at every entry
 *     scan                    exclusive prefix sums of the counts over the segment's sub-sequences (DC predictions wrap as int16, and
 *                             wrap-around sums are associative); fewer blocks than the segment's MCUs need: REDO
 *     write                   every lane decodes once more, now with its true first block and predictions, and stores the non-zero coefficients;
 *                             blocks past the expected count are dropped (pad bits can look like one); any STM_JPEG_E* condition before that: REDO
 *     redo                    the serial kernel of launch 1 over all segments, as for an unsplit batch; for the segment of a split image it
 *                             returns at once unless the segment is marked REDO, and then decodes it from scratch and sets STM_JPEG_REDONE in
 *                             its status word.  A damaged file, or one that did not converge, so has the serial path's pixels and status.
 * The records of the sub-sequences (32 bytes each: entry and exit states of the two latest rounds, the counts, and in record 0 the REDO mark) lie
 * in the image's own plane region, which nothing else uses before launch 2: no workspace is added, and an image is split only if they fit there.
 *
 * Malformed entropy data sets the segment's status word (STM_JPEG_E*) and leaves the rest of the segment's blocks zero; no input makes a kernel
 * read outside the blob or loop without bound (every loop is bounded by the segment's byte count and its block count).
 *
 * Refused before any launch: a count below zero, a NULL pointer with a non-zero count, a width or height outside 1..8192, a component count or
 * sampling outside the list, a table selector out of range, offsets that are misaligned, out of order or outside the blob / out / workspace,
 * segments that do not tile their image's MCUs in order, a descriptor field that disagrees with the ones it derives from -- a split field
 * out of order, or on an image with another number of segments than one or whose records do not fit, among them -- (STM_EINVAL); 2^31 or more
 * 8x8 blocks or 4-pixel groups, or 2^30 or more sub-sequence groups, in one batch (STM_EUNSUPPORTED). */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/stmask_hip.h"

#define STM_JPEG_MAX_DIM 8192
#define STM_JPEG_LOOK_BITS 9 /* width of the first-level Huffman lookup */

#define STM_JPEG_DECODE 0 /* stm_jpeg_image.kind */
#define STM_JPEG_RAW 1

/* status words of launch 1 */
#define STM_JPEG_ENOCODE 1    /* no Huffman code within 16 bits */
#define STM_JPEG_EINDEX 2     /* a coefficient index past 63 */
#define STM_JPEG_ESIZE 3      /* a size category above 11 (DC) or 10 (AC) */
#define STM_JPEG_ETRUNCATED 4 /* the segment ended before its blocks were done */
#define STM_JPEG_REDONE (1 << 8) /* or-ed in: the segment of a split image that the serial kernel decoded after all */

#define STM_JPEG_SUB_BYTES 128    /* a sub-sequence of a split segment, in raw (stuffed) bytes */
#define STM_JPEG_SUB_GROUP 64     /* sub-sequences per workgroup */
#define STM_JPEG_SPLIT_ROUNDS 2   /* R: sync rounds after round 0 */
#define STM_JPEG_SPLIT_LAUNCHES (STM_JPEG_SPLIT_ROUNDS + 4) /* what launch 1 becomes for a batch with a split image */
#define STM_JPEG_SPLIT_MAX_BYTES (1 << 30) /* a longer segment is not split */

#define STM_JPEG_STAGE_ENTROPY 1 /* the `stages` argument: which launches to make (7: all; anything else is for timing one of them) */
#define STM_JPEG_STAGE_IDCT 2
#define STM_JPEG_STAGE_COLOUR 4

#ifdef __cplusplus
extern "C" {
#endif

/* One Huffman table in the form the kernel reads.  look[first STM_JPEG_LOOK_BITS bits of the stream] = (code length << 8) | symbol, 0 when the
 * code is longer; then the canonical decode: a code of l bits with value <= maxcode[l] (-1: no code of that length) is symbol
 * huffval[code + valoff[l]]. */
typedef struct stm_jpeg_huff {
    uint16_t look[1 << STM_JPEG_LOOK_BITS];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t huffval[256];
} stm_jpeg_huff;

/* A table set: four quantisation tables in natural (row-major) order, then the Huffman tables DC 0, DC 1, AC 0, AC 1. */
typedef struct stm_jpeg_tables {
    uint16_t quant[4][64];
    stm_jpeg_huff huff[4];
} stm_jpeg_tables;

/* One frame.  Its 8x8 blocks are numbered blk_first .. : component 0's in raster order (mcu_h * vs rows of mcu_w * hs), then component 1's and
 * 2's (mcu_h rows of mcu_w).  Block g of the batch has its 64 int16 coefficients at workspace + 128 g and its 64 plane bytes inside the
 * component's plane, which starts at workspace + 128 * total_blocks + 64 * (first block of the component) and is (blocks per row * 8) wide.
 * The frame is written to out + out_off as ceil(width * height / 4) groups of 12 bytes (the last one padded). */
typedef struct stm_jpeg_image {
    int64_t out_off;    /* multiple of 16 */
    int64_t src_off;    /* in the blob, multiple of 16: the stm_jpeg_tables (STM_JPEG_DECODE) or the pixels, in the requested order (STM_JPEG_RAW) */
    int32_t kind;
    int32_t width, height;
    int32_t ncomp;      /* 1 or 3; 3 for STM_JPEG_RAW */
    int32_t hs, vs;     /* component 0's sampling factors; the others' are 1 */
    int32_t mcu_w, mcu_h;
    int32_t tq[3], td[3], ta[3];    /* per component: quantisation table 0..3, DC table 0..1, AC table 0..1 */
    int32_t blk_first;  /* STM_JPEG_RAW images have no blocks */
    int32_t quad_first; /* first 4-pixel group of the frame among the batch's */
    int32_t split;      /* 0: no image up to this one is split.  Else 2 * (the image's first sub-sequence group among the batch's) + (1 if THIS image is
                         * split: exactly one segment, of 2 or more sub-sequences whose records fit in 64 bytes per block).  Images without groups share
                         * their first group with the next image, as blk_first does. */
} stm_jpeg_image;

/* One restart interval (or the whole scan): nbytes of entropy-coded data at blob + byte_off (multiple of 16; the blob holds at least nbytes
 * rounded up to 16 from there), the markers around it removed, covering MCUs mcu_first .. mcu_first + mcu_count - 1 of `image`. */
typedef struct stm_jpeg_segment {
    int64_t byte_off;
    int32_t nbytes;
    int32_t image;
    int32_t mcu_first;
    int32_t mcu_count;
} stm_jpeg_segment;

/* which = 0: sizeof(stm_jpeg_image), 1: sizeof(stm_jpeg_segment), 2: sizeof(stm_jpeg_tables); anything else 0 */
size_t stm_jpeg_struct_bytes(int which);

/* Bytes of workspace stm_jpeg_decode_u8 needs for these images (coefficients and planes); 0 for images it would refuse. */
size_t stm_jpeg_workspace_bytes(const stm_jpeg_image* images, int n_images);

/* images / segments: host arrays.  blob, out, status (int32 [n_segments]) and workspace: device memory, 16-byte aligned.  bgr != 0: bytes
 * B, G, R per pixel, else R, G, B.  No host wait. */
int stm_jpeg_decode_u8(const stm_jpeg_image* images, int n_images, const stm_jpeg_segment* segments, int n_segments, const void* blob,
                       size_t blob_bytes, size_t images_off, size_t segments_off, void* out, size_t out_bytes, int* status, void* workspace,
                       size_t workspace_bytes, int bgr, int stages, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
