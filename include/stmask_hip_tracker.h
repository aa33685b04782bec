/* stmask_hip_tracker.h -- the temporal-fusion tracker's decisions on the device: the greedy resolution of a step (which detection replaces
 * which tracked row, which one opens a new track) and the keep plan of a per-clip drop, both as gather plans for stm_gather_rows2.
 * A third header beside stmask_hip.h and stmask_hip_output.h (whose prototype lists and STM_ABI_VERSION are unchanged): new entry points only,
 * same library, same error codes, same stream convention.  INTEGRATION.md section 17 describes the plan and its padding.
 */
#ifndef STMASK_HIP_TRACKER_H
#define STMASK_HIP_TRACKER_H

#include "stmask_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Greedy resolution of track_TF.py:132-156 for all B clips of a step, one workgroup per clip, one launch, no host read.
 *   match [D]          0, or 1 + the global tracked row detection d matched (stm_match_scores_embed_f32); NULL = all 0
 *   det_score [D]      the detections' scores; det_count [B]: detections per clip (their rows are sorted by clip; the counts sum to D)
 *   prev_offsets [B+1] first tracked row of every clip, prev_offsets[B] = Pn; prev_tm [Pn]: frames-since-last-match counters
 *   cap                > 0: an unmatched detection opens a track only while its clip holds fewer than cap rows; 0: no limit
 * Per clip: a tracked row is replaced by the best-scoring detection matched to it (strict > from -1.0 in detection order: the first among
 * equal scores) and its counter becomes 0; a row nothing matched keeps its index and counter; unmatched detections follow in detection order
 * with counter 0.
 *   plan [Pn + D]      indices into cat(tracked rows, detection rows), detection d at Pn + d; clip after clip, compact from entry 0; the
 *                      entries from new_offsets[B] on are 0 (a valid index: a gather may run over all Pn + D entries)
 *   new_offsets [B+1]  first row of every clip in the plan, new_offsets[B] = rows in all
 *   new_tm [Pn + D]    the counters of the plan's rows, 0 from new_offsets[B] on
 * Entries of match outside the detection's own clip are ignored (the detection neither replaces a row nor opens a track).  B <= 1024; sized
 * for the tens of clips a step holds: every workgroup recounts the clips before it (O(B * D) in all) behind a one-thread prefix of the counts. */
int stm_track_resolve_tf(const int* match, const float* det_score, const int* det_count, const int* prev_offsets, const int* prev_tm, int B,
                         int Pn, int D, int cap, int* plan, int* new_offsets, int* new_tm, stm_stream_t stream);

/* Keep plan of a per-clip drop: the rows of the clips with drop[b] == 0, in order.  offsets [B+1]; drop [B]; keep_rows [n_keep] with n_keep =
 * the kept clips' rows in all (the host knows every clip's row count); new_offsets [B+1].  B <= 1024. */
int stm_track_drop_plan(const int* offsets, const int* drop, int B, int n_keep, int* keep_rows, int* new_offsets, stm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
