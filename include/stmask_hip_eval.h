/* stmask_hip_eval.h -- video mask AP (YouTube-VIS, YTVOSeval iouType='segm', useCats=1) on the device: COCO RLE strings back to run lengths,
 * the intersection over union of whole tracks ("tubes") from the run lists, and the greedy matching of every (video, category) group at every
 * IoU threshold and area range.  A fifth header beside stmask_hip.h, stmask_hip_output.h, stmask_hip_tracker.h and stmask_hip_train.h (whose
 * prototype lists and STM_ABI_VERSION are unchanged): new entry points only, same library, same error codes, same stream convention.
 * INTEGRATION.md section 18 restates the evaluation contract; stmask_amd/vis_eval.py is the caller.
 *
 * Every count is an integer (run lengths uint32, areas and intersections int64), so the results do not depend on the order of any sum and are
 * the same bits from run to run.  No entry point reads anything back; zero masks, pairs or groups launch nothing.
 */
#ifndef STMASK_HIP_EVAL_H
#define STMASK_HIP_EVAL_H

#include "stmask_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STM_VIS_MAX_DET 100     /* detections of one (video, category) group: maxDets[-1], the host truncates to it */
#define STM_VIS_MAX_GT 1024     /* ground-truth tracks of one group (a bit per track and thread in LDS) */
#define STM_VIS_MAX_THREADS 64  /* n_thr * n_area of stm_vis_match: one thread each, one wavefront per group */

/* status bits of a mask (stm_vis_rle_decode, stm_vis_rle_check); a flagged mask gets n_runs = 0 and area = 0 */
#define STM_VIS_RLE_UNTERMINATED 1   /* the string's last character still has the continuation bit set */
#define STM_VIS_RLE_RANGE 2          /* a run length outside [0, 2^32) (or a value of more than 7 characters) */
#define STM_VIS_RLE_SUM 4            /* the runs do not sum to h * w */

/* COCO compressed RLE strings -> run lengths (the inverse of pycocotools' rleToString: character - 48 carries 5 value bits, bit 5 = "more
 * follows", bit 4 of a value's last group is its sign, and from run 3 on the value is a delta on the run two before).
 *   chars [offsets[n]]   the strings of n masks, concatenated;  offsets [n + 1] int64, ascending from 0;  hw [n] int64, h * w of each mask
 *   total_chars          offsets[n] as the host knows it (< 2^31): the size of chars and of runs
 *   runs [total_chars]   uint32; mask i's runs start at offsets[i] (a mask never has more runs than characters)
 *   n_runs [n] int32, area [n] int64 (the sum of the odd-indexed runs), status [n] int32 (0, or STM_VIS_RLE_* bits)
 * One wavefront per string.  Nothing is written outside runs[offsets[i] .. offsets[i + 1]) whatever the characters are. */
int stm_vis_rle_decode(const unsigned char* chars, const int64_t* offsets, const int64_t* hw, int n, int64_t total_chars, unsigned int* runs,
                       int* n_runs, int64_t* area, int* status, stm_stream_t stream);

/* The same area and sum check for uncompressed RLE (run lengths given as integers): runs [offsets[n]] uint32, read only. */
int stm_vis_rle_check(const unsigned int* runs, const int64_t* offsets, const int64_t* hw, int n, int64_t total_runs, int* n_runs, int64_t* area,
                      int* status, stm_stream_t stream);

/* Tube IoU of n_pairs (detection track, ground-truth track) pairs.
 *   pair_d, pair_g [n_pairs] int32   rows of table
 *   table [n_tracks, max_frames] int32: the mask index of a track's frame or -1;  track_len [n_tracks] int32 (<= max_frames)
 *   runs, run_off [n_masks] int64, n_runs [n_masks] int32, area [n_masks] int64: the masks (mask i's runs at runs + run_off[i])
 * For every frame f < min(len_d, len_g): both masks present: i += |d & g|, u += area_d + area_g - |d & g|; one present: u += its area.
 *   inter, uni [n_pairs] int64;  iou [n_pairs] double = (double)i / (double)u, or 0.0 when u == 0
 * One wavefront per pair, a lane per frame (a two-pointer merge of the two run lists), an int64 wavefront reduction. */
int stm_vis_tube_iou(const int* pair_d, const int* pair_g, int64_t n_pairs, const int* table, const int* track_len, int n_tracks, int max_frames,
                     const unsigned int* runs, const int64_t* run_off, const int* n_runs, const int64_t* area, int64_t n_masks, int64_t* inter,
                     int64_t* uni, double* iou, stm_stream_t stream);

/* Greedy matching of n_groups (video, category) groups; one wavefront per group, one thread per (area range a, threshold t).
 *   iou [pair_off[n_groups]] double: group k's [D, G] block, row-major, at pair_off[k] (int64 [n_groups + 1]); D and G from
 *   dt_off, gt_off [n_groups + 1] int32 (rows of the detection / ground-truth arrays; detections sorted by descending score)
 *   dt_area [dt_rows], gt_area [gt_rows] double: avg_area of the tracks;  gt_crowd [gt_rows] int32
 *   thr [n_thr] double;  area_rng [n_area, 2] double (inclusive bounds);  n_thr * n_area <= STM_VIS_MAX_THREADS
 *   max_d, max_g: the largest D and G of the call, <= STM_VIS_MAX_DET and STM_VIS_MAX_GT (the kernel walks no further)
 * A ground truth is ignored when it is crowd or its area lies outside the range; the walk visits the non-ignored ones, then the ignored ones,
 * each in row order (the stable non-ignored-first sort).  Per detection: best = min(t, 1 - 1e-10), m = -1; skip a ground truth matched at
 * this (a, t) unless it is crowd; stop at the ignored ones when m is set; skip iou < best; else best = iou, m = g.
 *   dt_match [dt_rows, n_area, n_thr] int32   the matched ground truth's row within its group, or -1
 *   dt_ignore [dt_rows, n_area, n_thr] uint8  the matched ground truth's flag; unmatched: the detection's own area outside the range
 *   gt_ignore [gt_rows, n_area] uint8 */
int stm_vis_match(const double* iou, const int64_t* pair_off, const int* dt_off, const int* gt_off, int n_groups, int max_d, int max_g,
                  const double* dt_area, const double* gt_area, const int* gt_crowd, const double* thr, int n_thr, const double* area_rng,
                  int n_area, int* dt_match, unsigned char* dt_ignore, unsigned char* gt_ignore, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
