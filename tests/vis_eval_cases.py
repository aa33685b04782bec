"""Inputs of the video mask AP tests, made at test time from a seed: the closed-form cases whose scores are known on paper, and a small generated
YouTube-VIS set that walks every branch of the evaluation.  Results carry compressed RLE strings (what the served pipeline writes), ground truth
carries uncompressed run-length lists (what the YouTube-VIS files hold).  Not a test module: imported by the vis_eval tests."""
import numpy as np

import vis_eval_restate as R
from stmask_amd.output_utils import rle_counts_to_string


def counts_of_mask(mask):
    """Run lengths of a [h, w] boolean mask, column-major, starting with a run of zeros (possibly of length 0)."""
    flat = np.asarray(mask, dtype=bool).reshape(-1, order="F")
    edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
    cnts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return ([0] + cnts) if flat.size and flat[0] else cnts


def rle(mask, compressed=True):
    h, w = mask.shape
    cnts = counts_of_mask(mask)
    return {"size": [h, w], "counts": rle_counts_to_string(cnts).decode() if compressed else cnts}


def box(h, w, y0, x0, bh, bw):
    m = np.zeros((h, w), dtype=bool)
    m[max(y0, 0):max(y0 + bh, 0), max(x0, 0):max(x0 + bw, 0)] = True
    return m


def _video(vid, h, w, n):
    return {"id": vid, "height": h, "width": w, "length": n, "file_names": [f"v{vid}/{f:05d}.jpg" for f in range(n)]}


def _ann(aid, vid, cat, masks, crowd=0, with_areas=True):
    a = {"id": aid, "video_id": vid, "category_id": cat, "iscrowd": crowd,
         "segmentations": [None if m is None else rle(m, compressed=False) for m in masks]}
    if with_areas:
        a["areas"] = [None if m is None else int(m.sum()) for m in masks]
    return a


def _res(vid, cat, score, masks):
    return {"video_id": vid, "category_id": cat, "score": score, "segmentations": [None if m is None else rle(m) for m in masks]}


def _anns(videos, cats, anns):
    return {"videos": videos, "categories": [{"id": c, "name": f"c{c}"} for c in cats], "annotations": anns}


def closed_form_cases():
    """name -> (annotations, results, {stat index: expected value}, {stat index: exact value}); one video each, frames of 24 x 40."""
    h, w = 24, 40
    gt = box(h, w, 4, 5, 10, 10)
    cases = {}
    # 1: one ground truth, one identical detection (two frames)
    cases["identical"] = (_anns([_video(1, h, w, 2)], [1], [_ann(1, 1, 1, [gt, gt])]), [_res(1, 1, 0.9, [gt, gt])],
                          {i: 1.0 for i in (0, 1, 2, 3, 6, 7, 8, 9)}, {i: -1.0 for i in (4, 5, 10, 11)})
    # 2: a detection of 100 pixels that shares 76 with the 10 x 10 block: i = 76, u = 100 + 100 - 76 = 124, IoU 0.6129: thresholds .5, .55 and .6
    # match.  (No whole-pixel shift of the block shares 76 pixels -- 76 is not a product of two integers up to 10 -- so 24 pixels of the block are
    # moved below it instead.)
    det = box(h, w, 4, 5, 10, 10)
    det[4:14, 5:7] = False                       # 80 left of the block ...
    det[4:8, 7] = False                          # ... 76 left
    det |= box(h, w, 14, 5, 2, 10)               # + 20 outside
    det |= box(h, w, 16, 5, 1, 4)                # + 4 outside: 100 pixels, 76 shared
    assert det.sum() == 100 and (det & gt).sum() == 76 and (det | gt).sum() == 124
    cases["iou_76_124"] = (_anns([_video(1, h, w, 1)], [1], [_ann(1, 1, 1, [gt])]), [_res(1, 1, 0.9, [det])],
                           {0: 0.3, 1: 1.0, 2: 0.0, 8: 0.3}, {})
    # 3: two ground truths, one detection equal to the first
    gt2 = box(h, w, 4, 25, 8, 8)
    cases["two_gt_one_det"] = (_anns([_video(1, h, w, 1)], [1], [_ann(1, 1, 1, [gt]), _ann(2, 1, 1, [gt2])]), [_res(1, 1, 0.9, [gt])],
                               {0: 51.0 / 101.0, 8: 0.5}, {})
    return cases


def threshold_pairs():
    """(ground truth, detection, i, u) with IoU exactly 1/2 and exactly 3/5, on 24 x 40."""
    h, w = 24, 40
    gt = box(h, w, 2, 2, 10, 10)                                   # 100 pixels
    half = box(h, w, 2, 2, 5, 10)                                  # 50 of them: i = 50, u = 100
    three_fifths = box(h, w, 2, 2, 6, 10)                          # 60 of them: i = 60, u = 100
    return gt, half, three_fifths


def generated_set(seed=20260):
    """(annotations, results): 6 videos, 3 categories.  See the assertions of check_coverage() for what it is built to contain."""
    rng = np.random.RandomState(seed)
    sizes = [(24, 40, 5), (37, 53, 9), (160, 200, 4), (288, 320, 3), (24, 40, 1), (37, 53, 6)]
    videos = [_video(v + 1, h, w, n) for v, (h, w, n) in enumerate(sizes)]
    anns, results, aid = [], [], 1

    def track(h, w, n, bh, bw, y0, x0, dy=1, dx=1, ellipse=False):
        out = []
        yy, xx = np.mgrid[0:h, 0:w]
        for f in range(n):
            cy, cx = y0 + dy * f, x0 + dx * f
            if ellipse:
                out.append((((yy - cy - bh / 2.0) / (bh / 2.0)) ** 2 + ((xx - cx - bw / 2.0) / (bw / 2.0)) ** 2) <= 1.0)
            else:
                out.append(box(h, w, cy, cx, bh, bw))
        return out

    def derive(masks, sy, sx, erode):
        out = []
        for m in masks:
            d = np.roll(np.roll(m, sy, axis=0), sx, axis=1)
            for _ in range(erode):
                d = d & np.roll(d, 1, axis=0) & np.roll(d, 1, axis=1)
            out.append(d)
        return out

    # (video, category, object geometry, detection derivation (shift, erosion), score)
    plan = [
        (1, 1, (8, 9, 2, 3), (0, 0, 0), 0.95), (1, 2, (10, 6, 10, 20), (1, 1, 0), 0.80), (1, 1, (6, 12, 14, 4), (2, 1, 1), 0.50),
        (2, 1, (12, 14, 3, 4), (1, 0, 0), 0.90), (2, 2, (9, 20, 20, 10), (2, 2, 0), 0.50), (2, 2, (14, 10, 5, 30), (0, 3, 1), 0.70),
        (3, 1, (140, 150, 5, 10), (6, 9, 0), 0.85), (3, 2, (130, 160, 20, 20), (20, 25, 2), 0.60),
        (4, 1, (270, 300, 4, 6), (8, 5, 0), 0.75), (4, 2, (265, 290, 10, 12), (30, 40, 3), 0.65),
        (6, 1, (10, 10, 5, 5), None, 0.0), (6, 3, (12, 12, 8, 20), None, 0.0),        # video 6 has no results
    ]
    for k, (vid, cat, (bh, bw, y0, x0), how, score) in enumerate(plan):
        h, w, n = sizes[vid - 1]
        masks = track(h, w, n, bh, bw, y0, x0, ellipse=(k % 3 == 1))
        gt_masks = list(masks)
        if k in (1, 5) and n > 2:
            gt_masks[1] = None                                     # a frame without the object
        anns.append(_ann(aid, vid, cat, gt_masks, crowd=0, with_areas=(k % 2 == 0)))
        aid += 1
        if how is None:
            continue
        det = derive(masks, *how)
        if k in (2, 5) and n > 3:
            det[2] = None                                          # a frame without the detection
        if k == 3:
            det = det[:n - 3]                                      # a detection list shorter than its video
        results.append(_res(vid, cat, score, det))
    # a crowd ground truth in video 2, category 2, and two detections inside it (both may match it)
    h, w, n = sizes[1]
    crowd = track(h, w, n, 16, 16, 18, 30, dy=0, dx=0)
    anns.append(_ann(aid, 2, 2, crowd, crowd=1, with_areas=False))
    aid += 1
    results.append(_res(2, 2, 0.40, derive(crowd, 1, 1, 0)))
    results.append(_res(2, 2, 0.40, derive(crowd, 0, 2, 1)))       # tied scores
    # false positives, and category 3 in video 1: detections without any ground truth
    results.append(_res(1, 1, 0.30, track(24, 40, 5, 4, 4, 18, 30, dy=0, dx=0)))
    results.append(_res(3, 2, 0.55, track(160, 200, 4, 30, 30, 120, 5, dy=0, dx=0)))
    results.append(_res(1, 3, 0.20, track(24, 40, 5, 5, 5, 1, 1)))
    # video 5: one ground truth and 101 detections of category 1; the low-scoring tail is tied, so the stable sort decides which one is cut
    gt5 = box(24, 40, 5, 5, 9, 11)
    anns.append(_ann(aid, 5, 1, [gt5], with_areas=True))
    aid += 1
    results.append(_res(5, 1, 0.88, [np.roll(gt5, 1, axis=1)]))
    for j in range(100):
        results.append(_res(5, 1, 0.05 if j >= 50 else 0.10 + 0.001 * (j % 7), [box(24, 40, int(rng.randint(0, 20)), int(rng.randint(0, 36)), 3, 3)]))
    return _anns(videos, [1, 2, 3], anns), results


def check_coverage(annotations, results):
    """The generator's own assertions, on the CPU: -> the restatement's (cat_ids, groups, eval, stats)."""
    cat_ids, groups = R.evaluate(annotations, results)
    ev = R.accumulate(groups, cat_ids)
    stats = R.summarize(ev)
    assert 0.2 < stats[0] < 0.8, stats
    assert stats[3] != -1 and stats[4] != -1 and stats[5] != -1, stats
    counts = {}
    for r in results:
        counts[(r["video_id"], r["category_id"])] = counts.get((r["video_id"], r["category_id"]), 0) + 1
    assert max(counts.values()) == 101
    assert any(g["ious"].shape[0] == 100 for g in groups)
    assert any(g["ious"].shape[1] == 0 and g["ious"].shape[0] > 0 for g in groups)          # detections, no ground truth
    assert any(g["ious"].shape[0] == 0 and g["ious"].shape[1] > 0 for g in groups)          # ground truth, no detections
    assert any(a["iscrowd"] for a in annotations["annotations"])
    assert any(s is None for a in annotations["annotations"] for s in a["segmentations"])
    assert any(s is None for r in results for s in r["segmentations"])
    lengths = {v["id"]: v["length"] for v in annotations["videos"]}
    assert any(len(r["segmentations"]) < lengths[r["video_id"]] for r in results)
    assert {v["id"] for v in annotations["videos"]} - {r["video_id"] for r in results}       # a video without results
    scores = [r["score"] for r in results]
    assert len(set(scores)) < len(scores)                                                     # tied scores
    vals = np.concatenate([g["ious"].reshape(-1) for g in groups])
    vals = vals[vals > 0]
    assert vals.min() < 0.45 and vals.max() == 1.0 and np.count_nonzero((vals > 0.5) & (vals < 0.95)) >= 4, np.sort(vals)
    return cat_ids, groups, ev, stats
