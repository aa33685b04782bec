/* stmask_hip_output.h -- the batched output stage of libstmask_hip.so: every tracked instance of every frame of a step goes from soft mask
 * to finished COCO RLE string, pixel box, score, class and id in a fixed number of launches, into ONE device buffer the host copies once.
 * A second header beside stmask_hip.h (whose prototype list and STM_ABI_VERSION are unchanged): new entry points only, same library, same
 * error codes, same stream convention.  INTEGRATION.md section 16 describes the buffer and what is exact.
 */
#ifndef STMASK_HIP_OUTPUT_H
#define STMASK_HIP_OUTPUT_H

#include "stmask_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame of a step (img_meta of output_utils.postprocess_ytbvis, reduced to what the device needs).
 * crop: the un-padded part of the mask; out: the size the masks are resized to; s_w / s_h: img / pad as fp32 (the box-centre rule compares
 * against them); inv_s_w / inv_s_h: 1.0f / s_w, 1.0f / s_h in fp32 (the box rescale multiplies by them). */
typedef struct stm_output_frame {
    int crop_h, crop_w, out_h, out_w;
    float s_w, s_h, inv_s_w, inv_s_h;
} stm_output_frame;

/* status bits of a row record */
#define STM_ROW_KEPT 1           /* the row passed the selection; its box is valid */
#define STM_ROW_RUN_OVERFLOW 2   /* more than max_runs runs (n_runs says how many): no string */
#define STM_ROW_ARENA_OVERFLOW 4 /* the string (str_len bytes) did not fit into the arena: not written */
#define STM_ROW_BAD_FRAME 8      /* frame_of_row outside [0, n_frames): the row is not kept */

/* One record per INPUT row, kept or not, in row order. */
typedef struct stm_output_row {
    int frame, status, n_runs, str_off, str_len, cls, box_id;
    uint32_t score_bits;         /* the fp32 score, bit for bit */
    int box[4];                  /* x1, y1, x2, y2 in pixels of the output frame */
} stm_output_row;

/* In front of the records.  total_bytes: sum of the str_len of all rows (what a large enough arena holds); the strings of the rows lie
 * compact and in row order: row r's at arena[str_off .. str_off + str_len). */
typedef struct stm_output_header {
    int n_rows, total_bytes, arena_bytes, reserved;
} stm_output_header;

/* sizeof the structs above as the library was compiled: 0 stm_output_frame, 1 stm_output_row, 2 stm_output_header, else 0 */
size_t stm_output_struct_bytes(int which);

/* Scratch of one call: n rows, max_out_px = the largest out_h * out_w among the frames. */
size_t stm_output_stage_workspace_bytes(int n, int64_t max_out_px, int max_runs);

/* masks [n, mh, mw] fp32; per row: frame_of_row int32, score fp32, cls / box_id (int64 when *_is_i64, else int32), box [n, 4] fp32 normalised,
 * row_keep bytes or NULL (non-zero = the pipeline's keep rule holds).  A row is kept when row_keep allows it, score > score_threshold (applied
 * when score_threshold > 0) and its box centre is not beyond s_w / s_h.  out: stm_output_header | n stm_output_row | arena, out_bytes in all.
 * n == 0: STM_OK, nothing is launched or written. */
int stm_output_stage_multi_f32(const float* masks, int n, int mh, int mw, const int* frame_of_row, const float* score, const void* cls,
                               int cls_is_i64, const void* box_id, int box_id_is_i64, const float* box, const uint8_t* row_keep,
                               const stm_output_frame* frames, int n_frames, float score_threshold, float thr, int max_runs, void* out,
                               size_t out_bytes, void* workspace, size_t workspace_bytes, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
