"""stmask_amd.track_host (the tracker's host decisions for all clips of a step) against a per-clip restatement of the reference's lines:
track_TF.py:129-156 (temporal fusion) and track.py:92-179 (without).  The restatements work on ONE clip with local indices, as the
reference does; the tests map them to the batched convention -- global rows, match id = 1 + the global tracked row, one gather plan into
cat(tracked rows, detection rows) with detection d at sum(prev_n) + d.  Integer decisions: equality, every case."""
import random

import pytest

from stmask_amd import track_host as th


# ---- the reference, one clip ------------------------------------------------------------------------------------------------------------------
def ref_tf_clip(n_prev, tracked_mask, match_ids, det_score, cap=0):
    """track_TF.py:129-156.  The tracked set as a list of sources: ('p', i) = tracked instance i as it was, ('d', idx) = detection idx.
    cap: the benchmark's max_instances rule (no reference line: an unmatched detection is skipped while the set holds cap rows)."""
    rows = [("p", i) for i in range(n_prev)]
    tracked_mask = list(tracked_mask)
    best_match_scores = [-1.0] * n_prev
    for idx, match_id in enumerate(match_ids):
        if match_id == 0:
            if cap and len(rows) >= cap:
                continue
            rows.append(("d", idx))                                   # :134-139
            tracked_mask.append(0)
        else:
            obj_id = match_id - 1                                       # :144
            if det_score[idx] > best_match_scores[obj_id]:              # :146
                best_match_scores[obj_id] = det_score[idx]
                rows[obj_id] = ("d", idx)                              # :153-155
                tracked_mask[obj_id] = 0                                # :156
    return rows, tracked_mask


def ref_nontf_clip(n_prev, match_ids, det_score, n_over, remove_false_inst):
    """track.py:92-179 -> (tracked set as sources, det_obj_ids, detections that leave: local indices)."""
    n_dets = len(match_ids)
    if n_prev == 0:                                                     # :94-103: prev_det_bbox is None
        rows = [("d", idx) for idx in range(n_dets)]
        det_obj_ids = list(range(n_dets))
    else:
        rows = [("p", i) for i in range(n_prev)]
        det_obj_ids = [-1] * n_dets                                     # :134
        best_match_scores, best_match_idx = [-1.0] * n_prev, [-1] * n_prev
        for idx, match_id in enumerate(match_ids):
            if match_id == 0:
                det_obj_ids[idx] = len(rows)                            # :139
                rows.append(("d", idx))
            else:
                obj_id = match_id - 1
                if det_score[idx] > best_match_scores[obj_id]:          # :155
                    if best_match_idx[obj_id] != -1:
                        det_obj_ids[best_match_idx[obj_id]] = -1        # :157
                    det_obj_ids[idx] = obj_id
                    best_match_scores[obj_id] = det_score[idx]
                    best_match_idx[obj_id] = idx
                    if n_over[idx] < 2:                                 # :162
                        rows[obj_id] = ("d", idx)
    leave = [idx for idx in range(n_dets) if det_obj_ids[idx] >= 0 or not remove_false_inst]   # :174-178
    return rows, det_obj_ids, leave


# ---- batched cases <-> per-clip pieces ----------------------------------------------------------------------------------------------------------
def offsets(counts):
    return [sum(counts[:b]) for b in range(len(counts) + 1)]


def to_global(local_ids, prev_n):
    """Per-clip local match ids (0 / 1 + local object) -> the batched ids (0 / 1 + global tracked row), concatenated."""
    p_off = offsets(prev_n)
    return [0 if m == 0 else m + p_off[b] for b, ms in enumerate(local_ids) for m in ms]


def plan_of(rows_per_clip, prev_n, counts):
    p_off, d_off = offsets(prev_n), offsets(counts)
    return [p_off[b] + i if kind == "p" else p_off[-1] + d_off[b] + i for b, rows in enumerate(rows_per_clip) for kind, i in rows]


def cat(per_clip):
    return [v for xs in per_clip for v in xs]


def check_tf(prev_n, tracked, local_ids, scores, cap=0):
    counts = [len(m) for m in local_ids]
    ref = [ref_tf_clip(prev_n[b], tracked[b], local_ids[b], scores[b], cap) for b in range(len(prev_n))]
    before = ([list(t) for t in tracked], list(prev_n))
    plan, new_n, new_tracked = th.match_tf(prev_n, tracked, counts, to_global(local_ids, prev_n), cat(scores), cap)
    assert plan == plan_of([r[0] for r in ref], prev_n, counts)
    assert new_n == [len(r[0]) for r in ref] and new_tracked == [r[1] for r in ref]
    assert (tracked, prev_n) == before                                  # inputs untouched
    return plan, new_n


def check_nontf(prev_n, local_ids, scores, n_over):
    counts = [len(m) for m in local_ids]
    d_off = offsets(counts)
    plan, new_n, obj_ids = th.match_nontf(prev_n, counts, to_global(local_ids, prev_n), cat(scores), cat(n_over))
    for remove in (True, False):
        ref = [ref_nontf_clip(prev_n[b], local_ids[b], scores[b], n_over[b], remove) for b in range(len(prev_n))]
        assert plan == plan_of([r[0] for r in ref], prev_n, counts)
        assert new_n == [len(r[0]) for r in ref] and obj_ids == cat(r[1] for r in ref)
        rows, dst_b, dst_j = th.output_rows(counts, obj_ids, remove)
        assert rows == [d_off[b] + i for b, r in enumerate(ref) for i in r[2]]
        assert dst_b == [b for b, r in enumerate(ref) for _ in r[2]]
        assert dst_j == [j for r in ref for j in range(len(r[2]))]
    return plan, new_n, obj_ids


def random_case(rng, B, equal_scores):
    """Clip 0 holds nothing when B > 1, one clip detects nothing; match ids repeat (few objects, many detections)."""
    prev_n = [0 if (B > 1 and b == 0) else rng.randint(1, 4) for b in range(B)]
    empty = rng.randrange(B) if B > 1 else -1
    counts = [0 if b == empty else rng.randint(1, 6) for b in range(B)]
    tracked = [[rng.randint(0, 12) for _ in range(n)] for n in prev_n]
    ids = [[rng.randint(0, prev_n[b]) for _ in range(counts[b])] for b in range(B)]
    pool = [0.25, 0.5] if equal_scores else None
    scores = [[rng.choice(pool) if pool else rng.random() for _ in range(counts[b])] for b in range(B)]
    n_over = [[rng.randint(0, 2) for _ in range(counts[b])] for b in range(B)]
    return prev_n, tracked, ids, scores, n_over


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------
def test_clip_offsets():
    assert th.clip_offsets([]) == [0] and th.clip_offsets([3]) == [0, 3] and th.clip_offsets([2, 0, 5]) == [0, 2, 2, 7]


@pytest.mark.parametrize("prev_n, gone, keep", [
    ([2, 0, 3], set(), [0, 1, 2, 3, 4]),            # none gone
    ([2, 0, 3], {0}, [2, 3, 4]),                    # some
    ([2, 1, 3], {1}, [0, 1, 3, 4, 5]),
    ([2, 1, 3], {0, 2}, [2]),
    ([2, 0, 3], {1}, [0, 1, 2, 3, 4]),              # a clip without rows
    ([2, 1, 3], {0, 1, 2}, []),                     # all
    ([4], {0}, []),
    ([4], set(), [0, 1, 2, 3]),
])
def test_keep_rows(prev_n, gone, keep):
    assert th.keep_rows(prev_n, gone) == keep
    assert keep == [r for b in range(len(prev_n)) if b not in gone for r in range(sum(prev_n[:b]), sum(prev_n[:b + 1]))]


def test_match_tf_named_cases():
    # two and three detections on one object, distinct scores: the best one wins wherever it stands
    plan, _ = check_tf([2], [[3, 4]], [[1, 1]], [[0.4, 0.9]])
    assert plan == [2 + 1, 1]
    plan, _ = check_tf([2], [[3, 4]], [[2, 2, 2]], [[0.5, 0.9, 0.7]])
    assert plan == [0, 2 + 1]
    # ... equal scores: strict >, the first one wins
    plan, _ = check_tf([2], [[3, 4]], [[1, 1]], [[0.5, 0.5]])
    assert plan == [2 + 0, 1]
    plan, _ = check_tf([2], [[3, 4]], [[2, 2, 2]], [[0.5, 0.5, 0.5]])
    assert plan == [0, 2 + 0]
    # B = 3: a clip without tracked rows beside clips with rows, a clip without detections, new objects and matches mixed
    plan, new_n = check_tf([0, 2, 3], [[], [1, 0], [5, 11, 2]], [[0, 0], [], [3, 0, 1, 3]], [[0.9, 0.8], [], [0.3, 0.6, 0.7, 0.3]])
    assert new_n == [2, 2, 4] and plan == [5, 6, 0, 1, 5 + 4, 3, 5 + 2, 5 + 3]


@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4, 6])
def test_match_tf_cap_below_at_and_above_the_clip_size(cap):
    # clip 0 holds 3 rows (cap 1, 2 below; 3 at; 4, 6 above), clip 1 none, clip 2 one; every clip gets unmatched detections and clip 0 a match too
    plan, new_n = check_tf([3, 0, 1], [[0, 2, 9], [], [4]], [[0, 2, 0, 0], [0, 0, 0], [0, 1]], [[0.9, 0.8, 0.7, 0.6], [0.5, 0.4, 0.3], [0.2, 0.1]], cap)
    if cap:
        assert new_n == [max(3, min(cap, 6)), min(cap, 3), max(1, min(cap, 2))]
        assert 4 + 1 in plan                        # a match is never capped
    else:
        assert new_n == [6, 3, 2]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("equal_scores", [False, True], ids=["distinct", "equal"])
def test_match_tf_seeded(B, equal_scores):
    rng = random.Random(1000 * B + equal_scores)
    for i in range(60):
        prev_n, tracked, ids, scores, _ = random_case(rng, B, equal_scores)
        big = max(prev_n) + 1
        check_tf(prev_n, tracked, ids, scores, cap=(0, 1, max(prev_n), big, big + 3)[i % 5])


def test_match_nontf_named_cases():
    # displacement: the second detection on object 0 scores higher -> the first loses its id; n_over 0 / 1 let the row be replaced, 2 does not
    for n_over, row0 in ((0, 2 + 1), (1, 2 + 1), (2, 2 + 0)):
        plan, _, obj_ids = check_nontf([2], [[1, 1]], [[0.4, 0.9]], [[0, n_over]])
        assert obj_ids == [-1, 0] and plan == [row0, 1]
    # the gate is read on the detection that takes the object at that moment: a blocked winner leaves the earlier replacement in place
    plan, _, obj_ids = check_nontf([1], [[1, 1, 1]], [[0.4, 0.9, 0.6]], [[1, 2, 0]])
    assert obj_ids == [-1, 0, -1] and plan == [1 + 0]
    # equal scores: the first keeps the object, the others get no id
    plan, _, obj_ids = check_nontf([2], [[2, 2, 2]], [[0.5, 0.5, 0.5]], [[0, 0, 0]])
    assert obj_ids == [1, -1, -1] and plan == [0, 2 + 0]
    # B = 3: the first-frame rule for the clip without rows (match ids are not read there), a clip without detections, new ids counted from the clip's set
    plan, new_n, obj_ids = check_nontf([0, 2, 3], [[0, 0], [], [3, 0, 1, 3, 0]], [[0.9, 0.8], [], [0.3, 0.6, 0.7, 0.8, 0.1]], [[0, 0], [], [0, 0, 2, 1, 0]])
    assert obj_ids == [0, 1, -1, 3, 0, 2, 4] and new_n == [2, 2, 5]
    assert plan == [5, 6, 0, 1, 2, 3, 5 + 5, 5 + 3, 5 + 6]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("equal_scores", [False, True], ids=["distinct", "equal"])
def test_match_nontf_and_output_rows_seeded(B, equal_scores):
    rng = random.Random(2000 * B + equal_scores)
    seen = set()
    for _ in range(60):
        prev_n, _, ids, scores, n_over = random_case(rng, B, equal_scores)
        _, _, obj_ids = check_nontf(prev_n, ids, scores, n_over)
        seen.add(-1 in obj_ids)
    assert seen == {True, False}                    # remove_false_inst had rows to remove, and frames where it had none
