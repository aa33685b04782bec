"""The yardstick of the video mask AP tests: YTVOSeval(iouType='segm', useCats=1) restated in plain numpy, following the contract's loops literally
(INTEGRATION.md section 18).  It shares nothing with the device code: every RLE is decoded to a dense boolean array and pixels are *counted* (no run
merging), the matching is the nested Python loop over thresholds, detections and sorted ground truths, and accumulate walks precision backwards
element by element.  Slow on purpose; the tests keep the frames small.  Not a test module (no test_ prefix): imported by the vis_eval tests."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(.0, 1.0, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e10]]


def string_to_counts(s):
    """maskApi.c rleFrString: the run lengths of a compressed COCO RLE string, as Python ints."""
    if isinstance(s, str):
        s = s.encode()
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("the string ends inside a value")
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def counts_of(rle):
    c = rle["counts"]
    return string_to_counts(c) if isinstance(c, (str, bytes)) else [int(v) for v in c]


_dense_cache = {}       # id(rle dict) -> (the dict, its dense form): evaluate() decodes a frame once, not once per pair


def dense(rle):
    """The mask as a flat boolean array of h * w pixels (column-major, as RLE counts them); treat it as read-only."""
    hit = _dense_cache.get(id(rle))
    if hit is not None and hit[0] is rle:
        return hit[1]
    out = _dense(rle)
    _dense_cache[id(rle)] = (rle, out)
    return out


def _dense(rle):
    cnts = counts_of(rle)
    h, w = rle["size"]
    if any(c < 0 or c >= 2 ** 32 for c in cnts):
        raise ValueError("a run length outside [0, 2^32)")
    if sum(cnts) != h * w:
        raise ValueError("the runs do not sum to h * w")
    out = np.zeros(h * w, dtype=bool)
    p = 0
    for j, c in enumerate(cnts):
        if j & 1:
            out[p:p + c] = True
        p += c
    return out


def avg_area_of_masks(segs):
    areas = [int(dense(s).sum()) for s in segs if s is not None]
    nz = [a for a in areas if a != 0]
    return float(np.mean(nz)) if nz else 0.0


def tube_counts(d_segs, g_segs):
    """(intersection, union) pixel counts over the frames the two lists share (zip)."""
    i = u = 0
    for sd, sg in zip(d_segs, g_segs):
        if sd is not None and sg is not None:
            a, b = dense(sd), dense(sg)
            i += int((a & b).sum())
            u += int((a | b).sum())
        elif sd is not None:
            u += int(dense(sd).sum())
        elif sg is not None:
            u += int(dense(sg).sum())
    return i, u


def match_group(ious, dt_area, gt_area, gt_crowd, thrs=IOU_THRS, area_rng=AREA_RNG):
    """The matching of one group from its [D, G] IoU block -> dt_match [D, A, T] (row of the ground truth in the order given, or -1),
    dt_ignore [D, A, T], gt_ignore [G, A]."""
    D, G, A, T = len(dt_area), len(gt_area), len(area_rng), len(thrs)
    dt_match = -np.ones((D, A, T), dtype=np.int32)
    dt_ignore = np.zeros((D, A, T), dtype=bool)
    gt_ignore = np.zeros((G, A), dtype=bool)
    for a, (lo, hi) in enumerate(area_rng):
        ig = np.array([bool(gt_crowd[g]) or gt_area[g] < lo or gt_area[g] > hi for g in range(G)], dtype=bool)
        gt_ignore[:, a] = ig
        gtind = np.argsort(ig.astype(np.uint8), kind="mergesort")          # non-ignored first, stable
        for t, thr in enumerate(thrs):
            taken = np.zeros(G, dtype=bool)
            for d in range(D):
                best, m = min([thr, 1 - 1e-10]), -1
                for pos in range(G):
                    g = gtind[pos]
                    if taken[g] and not gt_crowd[g]:
                        continue
                    if m > -1 and not ig[m] and ig[g]:
                        break
                    if ious[d, g] < best:
                        continue
                    best, m = ious[d, g], g
                if m == -1:
                    continue
                dt_match[d, a, t] = m
                dt_ignore[d, a, t] = ig[m]
                taken[m] = True
            for d in range(D):
                if dt_match[d, a, t] == -1 and (dt_area[d] < lo or dt_area[d] > hi):
                    dt_ignore[d, a, t] = True
    return dt_match, dt_ignore, gt_ignore


def evaluate(annotations, results):
    """-> (cat_ids, groups): per (video, category) with any ground truth or detection, ordered by category then video: dict with video_id,
    category_id, dt_scores, ious / inter / union [D, G], dt_area, gt_area, dt_match, dt_ignore, gt_ignore."""
    _dense_cache.clear()
    vid_ids = [v["id"] for v in annotations["videos"]]
    cat_ids = sorted(c["id"] for c in annotations["categories"])
    for i, r in enumerate(results):
        if r["video_id"] not in vid_ids:
            raise ValueError(f"result {i}: unknown video_id")
    groups = []
    for cat in cat_ids:
        for vid in vid_ids:
            gt = [a for a in annotations["annotations"] if a["video_id"] == vid and a["category_id"] == cat]
            dt = [r for r in results if r["video_id"] == vid and r["category_id"] == cat]
            if not gt and not dt:
                continue
            order = np.argsort([-float(r["score"]) for r in dt], kind="mergesort")[:MAX_DETS[-1]] if dt else []
            dt = [dt[k] for k in order]
            D, G = len(dt), len(gt)
            inter, union, ious = np.zeros((D, G), dtype=np.int64), np.zeros((D, G), dtype=np.int64), np.zeros((D, G))
            for d in range(D):
                for g in range(G):
                    i, u = tube_counts(dt[d]["segmentations"], gt[g]["segmentations"])
                    inter[d, g], union[d, g] = i, u
                    ious[d, g] = float(i) / float(u) if u > 0 else 0.0
            gt_area = []
            for a in gt:
                if a.get("areas") is not None:
                    nz = [x for x in a["areas"] if x]
                    gt_area.append(float(np.mean(nz)) if nz else 0.0)
                else:
                    gt_area.append(avg_area_of_masks(a["segmentations"]))
            dt_area = [avg_area_of_masks(r["segmentations"]) for r in dt]
            gt_crowd = [bool(a.get("iscrowd", 0)) for a in gt]
            dtm, dti, gti = match_group(ious, dt_area, gt_area, gt_crowd)
            groups.append({"video_id": vid, "category_id": cat, "dt_scores": np.array([float(r["score"]) for r in dt], dtype=np.float64),
                           "ious": ious, "inter": inter, "union": union, "dt_area": np.array(dt_area), "gt_area": np.array(gt_area),
                           "dt_match": dtm, "dt_ignore": dti, "gt_ignore": gti})
    return cat_ids, groups


def accumulate(groups, cat_ids):
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, cat in enumerate(cat_ids):
        E = [g for g in groups if g["category_id"] == cat]
        if not E:
            continue
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                scores = np.concatenate([e["dt_scores"][:max_det] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dt_match"][:max_det, a, :] for e in E], axis=0)[inds]     # [N, T]
                dt_ig = np.concatenate([e["dt_ignore"][:max_det, a, :] for e in E], axis=0)[inds]
                gt_ig = np.concatenate([e["gt_ignore"][:, a] for e in E])
                npig = int(np.count_nonzero(gt_ig == 0))
                if npig == 0:
                    continue
                for t in range(T):
                    tp = np.cumsum([bool(dtm[i, t] >= 0 and not dt_ig[i, t]) for i in range(len(inds))]).astype(np.float64)
                    fp = np.cumsum([bool(dtm[i, t] < 0 and not dt_ig[i, t]) for i in range(len(inds))]).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    idx = np.searchsorted(rc, REC_THRS, side="left")
                    for ri, pi in enumerate(idx):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return {"precision": precision, "recall": recall}


def summarize(ev):
    def mean_valid(s):
        s = s[s > -1]
        return -1.0 if len(s) == 0 else float(np.mean(s))

    p, r = ev["precision"], ev["recall"]
    return np.array([mean_valid(p[:, :, :, 0, 2]), mean_valid(p[0:1, :, :, 0, 2]), mean_valid(p[5:6, :, :, 0, 2]),
                     mean_valid(p[:, :, :, 1, 2]), mean_valid(p[:, :, :, 2, 2]), mean_valid(p[:, :, :, 3, 2]),
                     mean_valid(r[:, :, 0, 0]), mean_valid(r[:, :, 0, 1]), mean_valid(r[:, :, 0, 2]),
                     mean_valid(r[:, :, 1, 2]), mean_valid(r[:, :, 2, 2]), mean_valid(r[:, :, 3, 2])])


def stats_of(annotations, results):
    cat_ids, groups = evaluate(annotations, results)
    return summarize(accumulate(groups, cat_ids))
