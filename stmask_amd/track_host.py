"""The tracker's host decisions: plain functions on lists of ints and floats, no torch, no state.

The batched pipeline keeps the tracked instances of all clips in concatenated row tensors (rows sorted by clip).  What the reference
decides per clip with tensor scalars -- which detection replaces which tracked instance, which one opens a new track, which ids leave
with the frame (track_TF.py:129-156, track.py:92-179) -- is decided here for all clips of a step at once, and leaves as ONE gather plan:
indices into cat(tracked rows, detection rows), detection d at sum(prev_n) + d.
"""


def clip_offsets(counts):
    """[0, c0, c0 + c1, ...]: the first row of every clip in a concatenated set, and the total."""
    off = [0]
    for n in counts:
        off.append(off[-1] + n)
    return off


def keep_rows(prev_n, gone):
    """Rows of the tracked set that stay when the clips `gone` drop theirs."""
    off = clip_offsets(prev_n)
    return [r for b in range(len(prev_n)) if b not in gone for r in range(off[b], off[b + 1])]


def match_tf(prev_n, tracked, counts, ids, scores, cap=0):
    """Greedy resolution of the temporal-fusion tracker (track_TF.py:132-156) -> (plan, new prev_n, new frames-since-last-match counters).
    ids[d]: 0 (a new object) or 1 + the global row of the tracked instance detection d matched; of several detections on one instance the
    best-scoring wins, the first among equals.  cap > 0: the benchmark-only max_instances rule (BatchedClipPipeline.max_instances) -- an
    unmatched detection opens a track only while its clip holds fewer."""
    p_off, d_off = clip_offsets(prev_n), clip_offsets(counts)
    Pn = p_off[-1]
    plan, new_n, new_tracked = [], [], []
    for b, pn in enumerate(prev_n):
        p0, d0 = p_off[b], d_off[b]
        src = list(range(p0, p0 + pn))
        tm = list(tracked[b])
        best = [-1.0] * pn
        for d in range(d0, d_off[b + 1]):
            mid = ids[d]
            if mid == 0:
                if cap and len(src) >= cap:
                    continue
                src.append(Pn + d)
                tm.append(0)
            else:
                obj = mid - 1 - p0
                if scores[d] > best[obj]:
                    best[obj] = scores[d]
                    src[obj] = Pn + d
                    tm[obj] = 0
        plan += src
        new_n.append(len(src))
        new_tracked.append(tm)
    return plan, new_n, new_tracked


def match_nontf(prev_n, counts, ids, scores, n_over):
    """Greedy resolution of the tracker without temporal fusion (track.py:92-170) -> (plan, new prev_n, object id per detection; -1: lost its
    object to a better-scoring detection).  n_over[d] = (mask_ious[d] > 0.3).sum(): a matched object's row is replaced only while it is
    below 2 (track.py:162)."""
    p_off, d_off = clip_offsets(prev_n), clip_offsets(counts)
    Pn = p_off[-1]
    plan, new_n, obj_ids = [], [], [-1] * d_off[-1]
    for b, pn in enumerate(prev_n):
        p0, d0 = p_off[b], d_off[b]
        src = list(range(p0, p0 + pn))
        if pn == 0:
            # (track.py:92-97: the first frame with detections -- they become the objects)
            for d in range(d0, d_off[b + 1]):
                obj_ids[d] = d - d0
                src.append(Pn + d)
        else:
            best_score, best_det = [-1.0] * pn, [-1] * pn
            for d in range(d0, d_off[b + 1]):
                mid = ids[d]
                if mid == 0:
                    obj_ids[d] = len(src)
                    src.append(Pn + d)
                else:
                    obj = mid - 1 - p0
                    if scores[d] > best_score[obj]:
                        if best_det[obj] != -1:
                            obj_ids[best_det[obj]] = -1
                        obj_ids[d] = obj
                        best_score[obj], best_det[obj] = scores[d], d
                        if n_over[d] < 2:                        # track.py:162
                            src[obj] = Pn + d
        plan += src
        new_n.append(len(src))
    return plan, new_n, obj_ids


def output_rows(counts, obj_ids, remove_false_inst):
    """The frame's detections that leave with an object id (remove_false_inst, track.py:172-179), in detection order -> (detection rows,
    their clips, their slots in the clip's output)."""
    d_off = clip_offsets(counts)
    rows, dst_b, dst_j = [], [], []
    for b in range(len(counts)):
        j_out = 0
        for d in range(d_off[b], d_off[b + 1]):
            if obj_ids[d] >= 0 or not remove_false_inst:
                rows.append(d)
                dst_b.append(b)
                dst_j.append(j_out)
                j_out += 1
    return rows, dst_b, dst_j
