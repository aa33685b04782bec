"""Video mask AP of a YouTube-VIS results file: `calc_metrics` of the reference's layers/eval_utils.py:109-119, SURVEY.md row 15.

The reference hands the number to the youtubevos fork of cocoapi (`YTVOS`, `YTVOSeval(iouType='segm')`), which is not a dependency of this
package and is not imported here, not even optionally.  `VisEval` restates its contract and runs the mask work on the
MI355X (csrc/vis_eval.hip, include/stmask_hip_eval.h): the compressed RLE strings of all results are decoded to run lengths in one launch
(`pack_masks`; uncompressed ground truth is checked by `stm_vis_rle_check`), the tube IoU of every (detection, ground truth) pair of every (video,
category) group is a merge of run lists (`tube_iou`), and the greedy matching of all groups at 10 thresholds x 4 area ranges is one launch
(`match_groups`).  The host parses, groups and sorts (numpy), and folds the compact match arrays into precision / recall in float64
(`accumulate_groups`, `summarize_eval`).  The constructor holds the whole host part, the
one per-mask Python loop (`flatten_masks`) included; `evaluate()` is uploads, launches and one round of copies.  There is no CPU fallback for
the device part.

Not built: iouType='bbox', proposal mode (useCats = 0), polygons, per-frame COCO evaluation.
"""
import json

import numpy as np
import torch

from ._lib import StmError, c_p, call

IOU_THRS = np.linspace(.5, .95, 10)            # the bits are part of the contract: IOU_THRS[2] is 0.6000000000000001
REC_THRS = np.linspace(.0, 1.0, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = np.array([[0, 1e10], [0, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e10]], dtype=np.float64)
AREA_LBL = ("all", "small", "medium", "large")
MAX_DET, MAX_GT = 100, 1024                    # STM_VIS_MAX_DET, STM_VIS_MAX_GT
RLE_UNTERMINATED, RLE_RANGE, RLE_SUM = 1, 2, 4  # STM_VIS_RLE_* status bits


# what the device part of this module did since the last reset_counters(): launches of the four stm_vis_* entry points, bytes copied each way, and
# device -> host copies (each one waits for the stream); scripts/bench_vis_eval.py reports them.  The torch glue between them is not counted.
COUNTERS = {"launches": 0, "h2d_bytes": 0, "d2h_bytes": 0, "host_syncs": 0}


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0


def _launch(name, n_items, *args):
    if n_items > 0:                      # the library launches nothing for zero items
        COUNTERS["launches"] += 1
    call(name, *args)


def _up(x, device):
    t = torch.from_numpy(np.ascontiguousarray(x))
    COUNTERS["h2d_bytes"] += t.numel() * t.element_size()
    return t.to(device)


def _down(t):
    COUNTERS["d2h_bytes"] += t.numel() * t.element_size()
    COUNTERS["host_syncs"] += 1
    return t.cpu().numpy()


def _p(t):
    return c_p(t.data_ptr()) if t is not None and t.numel() else c_p(0)


def _stream():
    return c_p(torch.cuda.current_stream().cuda_stream)


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise StmError("vis_eval needs the MI355X: the RLE decode, tube IoU and matching kernels have no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise StmError(f"vis_eval needs a GPU device, got {device}; there is no CPU fallback")
    return device


class MaskSet:
    """Run lists of n masks on the device.  runs: int32 storage of the uint32 run lengths; run_off [n] int64; n_runs [n] int32; area [n] int64;
    status [n] int32 (STM_VIS_RLE_* bits; a flagged mask has n_runs = area = 0); pos [n] (host): where the i-th mask handed in sits."""

    def __init__(self, runs, run_off, n_runs, area, status, pos):
        self.runs, self.run_off, self.n_runs, self.area, self.status, self.pos = runs, run_off, n_runs, area, status, pos
        self.n = int(n_runs.shape[0])

    def run_list(self, i):
        """The runs of the i-th mask handed in, as a numpy uint32 array (a device read: for tests and error messages)."""
        k = int(self.pos[i])
        o, n = int(self.run_off[k]), int(self.n_runs[k])
        return self.runs[o:o + n].cpu().numpy().view(np.uint32)


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


class HostMasks:
    """flatten_masks' result: the masks of a call as flat host arrays, string masks first.  chars uint8 [s_off[-1]] with s_off [ns + 1]; flat uint32
    [l_off[-1]] (the uncompressed run lengths) with l_off [nl + 1]; hw int64 [ns + nl] in that order; pos [n]: where the i-th mask handed in sits."""

    def __init__(self, chars, s_off, flat, l_off, hw, pos):
        self.chars, self.s_off, self.flat, self.l_off, self.hw, self.pos = chars, s_off, flat, l_off, hw, pos
        self.ns, self.nl = len(s_off) - 1, len(l_off) - 1


def flatten_masks(rles, who=None):
    """COCO RLE dicts {'size': [h, w], 'counts': str | bytes | list of ints} -> HostMasks: the one per-mask Python loop of an evaluation (it is
    part of the parse).  `who(i)` names mask i in an error."""
    name = who or (lambda i: f"mask {i}")
    strs, lists, s_idx, l_idx = [], [], [], []
    hw = np.empty(len(rles), dtype=np.int64)
    for i, r in enumerate(rles):
        c = r["counts"]
        h, w = r["size"]
        hw[i] = int(h) * int(w)
        if isinstance(c, str):
            strs.append(c.encode("ascii", "replace"))
            s_idx.append(i)
        elif isinstance(c, (bytes, bytearray)):
            strs.append(bytes(c))
            s_idx.append(i)
        elif isinstance(c, (list, tuple, np.ndarray)):
            lists.append(c)
            l_idx.append(i)
        else:
            raise ValueError(f"{name(i)}: counts is {type(c).__name__}, neither a compressed string nor a list of run lengths "
                             "(polygons are not built)")
    if len(rles) and (hw.min() < 0 or hw.max() >= 2 ** 32):
        raise StmError(f"{name(int(np.argmax((hw < 0) | (hw >= 2 ** 32))))}: h * w must be below 2^32")
    ns, nl = len(strs), len(lists)
    s_off = _offsets([len(s) for s in strs])
    l_off = _offsets([len(c) for c in lists])
    if s_off[-1] >= 2 ** 31 or l_off[-1] >= 2 ** 31:
        raise StmError("vis_eval: 2^31 or more RLE characters / runs in one call")
    flat = np.zeros(0, dtype=np.int64)
    if l_off[-1]:
        flat = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in lists])
        if flat.min() < 0 or flat.max() >= 2 ** 32:
            bad = int(np.searchsorted(l_off, int(np.argmax((flat < 0) | (flat >= 2 ** 32))), "right")) - 1
            raise ValueError(f"{name(l_idx[bad])}: a run length outside [0, 2^32)")
    pos = np.empty(len(rles), dtype=np.int64)
    pos[np.asarray(s_idx, dtype=np.int64)] = np.arange(ns)
    pos[np.asarray(l_idx, dtype=np.int64)] = ns + np.arange(nl)
    order = np.asarray(s_idx + l_idx, dtype=np.int64)
    return HostMasks(np.frombuffer(b"".join(strs), dtype=np.uint8).copy(), s_off, flat.astype(np.uint32), l_off, hw[order], pos)


def upload_masks(hm, device=None):
    """HostMasks -> MaskSet: the compressed strings decoded by stm_vis_rle_decode, the integer lists checked by stm_vis_rle_check.  No host read:
    the caller looks at `status` when it copies its results."""
    device = _device(device)
    ns, nl, total_c, total_l = hm.ns, hm.nl, int(hm.s_off[-1]), int(hm.l_off[-1])
    n = ns + nl
    runs = torch.empty(total_c + total_l, dtype=torch.int32, device=device)
    n_runs = torch.empty(n, dtype=torch.int32, device=device)
    area = torch.empty(n, dtype=torch.int64, device=device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    hw_d = _up(hm.hw, device)
    run_off = _up(np.concatenate([hm.s_off[:-1], total_c + hm.l_off[:-1]]), device)
    with torch.cuda.device(device):
        if ns:
            chars = _up(hm.chars, device) if total_c else None
            off_d = _up(hm.s_off, device)
            _launch("stm_vis_rle_decode", ns, _p(chars), _p(off_d), _p(hw_d), ns, total_c, _p(runs), _p(n_runs), _p(area), _p(status), _stream())
        if nl:
            if total_l:
                runs[total_c:] = _up(hm.flat.view(np.int32), device)
            off_d = _up(hm.l_off, device)
            _launch("stm_vis_rle_check", nl, _p(runs[total_c:]), _p(off_d), _p(hw_d[ns:]), nl, total_l, _p(n_runs[ns:]), _p(area[ns:]),
                    _p(status[ns:]), _stream())
    return MaskSet(runs, run_off, n_runs, area, status, hm.pos)


def pack_masks(rles, device=None, who=None):
    """flatten_masks + upload_masks: COCO RLE dicts -> MaskSet on the device."""
    device = _device(device)
    return upload_masks(flatten_masks(rles, who), device)


def raise_for_status(status_host, pos, who):
    """ValueError naming the first flagged mask (status_host: the MaskSet's status on the host)."""
    bad = np.flatnonzero(status_host[pos] != 0)
    if bad.size:
        i = int(bad[0])
        st = int(status_host[pos[i]])
        what = [w for bit, w in ((RLE_UNTERMINATED, "the string ends inside a value"), (RLE_RANGE, "a run length outside [0, 2^32)"),
                                 (RLE_SUM, "the runs do not sum to h * w")) if st & bit]
        raise ValueError(f"{who(i)}: malformed RLE ({'; '.join(what)})")


def tube_iou(masks, table, track_len, pair_d, pair_g):
    """stm_vis_tube_iou: table [n_tracks, F] int32 (positions in `masks` or -1), track_len [n_tracks] int32, pair_d / pair_g [n_pairs] int32,
    all on the device -> (inter int64, union int64, iou float64), each [n_pairs]."""
    dev = masks.n_runs.device
    for t in (table, track_len, pair_d, pair_g):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
            raise StmError("tube_iou: expected contiguous int32 tensors on the masks' device")
    n_tracks, frames = (int(table.shape[0]), int(table.shape[1])) if table.dim() == 2 else (0, 0)
    n_pairs = int(pair_d.shape[0])
    if int(pair_g.shape[0]) != n_pairs or int(track_len.shape[0]) != n_tracks:
        raise StmError("tube_iou: pair lists or track lengths do not fit")
    inter = torch.empty(n_pairs, dtype=torch.int64, device=dev)
    uni = torch.empty(n_pairs, dtype=torch.int64, device=dev)
    iou = torch.empty(n_pairs, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _launch("stm_vis_tube_iou", n_pairs, _p(pair_d), _p(pair_g), n_pairs, _p(table), _p(track_len), n_tracks, frames, _p(masks.runs), _p(masks.run_off),
             _p(masks.n_runs), _p(masks.area), masks.n, _p(inter), _p(uni), _p(iou), _stream())
    return inter, uni, iou


def match_groups(iou, pair_off, dt_off, gt_off, dt_area, gt_area, gt_crowd, max_d, max_g, thr=IOU_THRS, area_rng=AREA_RNG):
    """stm_vis_match for the groups described by pair_off (int64 [n + 1]), dt_off and gt_off (int32 [n + 1]): device tensors; max_d / max_g: the
    largest group sizes (host ints, refused above 100 / 1024) -> dt_match int32 [rows, A, T], dt_ignore bool [rows, A, T], gt_ignore bool
    [gt_rows, A]."""
    dev = pair_off.device
    n_groups = int(pair_off.shape[0]) - 1
    thr_d = _up(np.asarray(thr, dtype=np.float64), dev)
    rng_d = _up(np.asarray(area_rng, dtype=np.float64), dev)
    T, A = int(thr_d.shape[0]), int(rng_d.shape[0])
    rows, gt_rows = int(dt_area.shape[0]), int(gt_area.shape[0])
    dt_match = torch.full((rows, A, T), -1, dtype=torch.int32, device=dev)
    dt_ignore = torch.zeros((rows, A, T), dtype=torch.uint8, device=dev)
    gt_ignore = torch.zeros((gt_rows, A), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _launch("stm_vis_match", n_groups, _p(iou), _p(pair_off), _p(dt_off), _p(gt_off), max(n_groups, 0), int(max_d), int(max_g), _p(dt_area), _p(gt_area),
             _p(gt_crowd), _p(thr_d), T, _p(rng_d), A, _p(dt_match), _p(dt_ignore), _p(gt_ignore), _stream())
    return dt_match, dt_ignore.bool(), gt_ignore.bool()


def track_avg_area(masks, table):
    """avg_area of every row of table on the device: the mean of the non-zero per-frame areas, 0.0 when there are none (an int64 sum divided once
    in float64: the value numpy's mean of the integers gives)."""
    if table.shape[0] == 0 or table.shape[1] == 0 or masks.n == 0:
        return torch.zeros(table.shape[0], dtype=torch.float64, device=table.device)
    idx = table.long()
    a = masks.area[idx.clamp(min=0)] * (idx >= 0)
    cnt = (a > 0).sum(1)
    return torch.where(cnt > 0, a.sum(1).double() / cnt.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=table.device))


def _load(x):
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        with open(x) as f:
            return json.load(f)
    return x


def file_avg_area(areas):
    """avg_area from an annotation's `areas` list: the mean of its non-zero entries (None counts as absent), 0.0 when there are none."""
    nz = [a for a in areas if a]
    return float(np.mean(nz)) if nz else 0.0


def group_tracks(annotations, results):
    """The host part of evaluate(): -> (video ids, category ids ascending, groups).  A group is a dict {video_id, category_id, gt: [annotation],
    dt: [result], dt_index: [position in results]} for every (video, category) with a ground truth or a detection, ordered by category, then by
    the video's place in the file; detections by descending score (stable), the first 100.  A result of an unknown video is a ValueError, one of
    an unknown category is dropped."""
    vid_ids = [v["id"] for v in annotations["videos"]]
    cat_ids = sorted(c["id"] for c in annotations["categories"])
    vid_set, cat_set = set(vid_ids), set(cat_ids)
    gts, dts = {}, {}
    for ann in annotations.get("annotations") or []:
        if ann["video_id"] not in vid_set:
            raise ValueError(f"annotation {ann.get('id')}: video_id {ann['video_id']} is not in the annotation file's videos")
        if ann["category_id"] in cat_set:
            gts.setdefault((ann["video_id"], ann["category_id"]), []).append(ann)
    for i, res in enumerate(results):
        if res["video_id"] not in vid_set:
            raise ValueError(f"result {i}: video_id {res['video_id']} is not in the annotation file")
        if res["category_id"] in cat_set:
            dts.setdefault((res["video_id"], res["category_id"]), []).append(i)
    groups = []
    for cat in cat_ids:
        for vid in vid_ids:
            g, d = gts.get((vid, cat), []), dts.get((vid, cat), [])
            if not g and not d:
                continue
            scores = np.array([float(results[i]["score"]) for i in d], dtype=np.float64)
            keep = np.argsort(-scores, kind="mergesort")[:MAX_DET]
            d = [d[k] for k in keep]
            groups.append({"video_id": vid, "category_id": cat, "gt": g, "dt": [results[i] for i in d], "dt_index": d,
                           "dt_scores": scores[keep]})
    return vid_ids, cat_ids, groups


def accumulate_groups(groups, cat_ids, thr=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, n_area=len(AREA_RNG)):
    """YTVOSeval.accumulate from the compact match arrays.  groups: dicts with category_id, dt_scores [D] (descending), dt_match [D, A, T] (a
    ground-truth row or -1), dt_ignore [D, A, T], gt_ignore [G, A], in evaluation order.  -> {"precision": [T, R, K, A, M], "recall":
    [T, K, A, M], "counts": [T, R, K, A, M]}, -1 where a cell has no non-ignored ground truth."""
    T, R, K, A, M = len(thr), len(rec_thrs), len(cat_ids), n_area, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    by_cat = {c: [] for c in cat_ids}
    for g in groups:
        by_cat[g["category_id"]].append(g)
    for k, cat in enumerate(cat_ids):
        gs = by_cat[cat]
        if not gs:
            continue
        for a in range(A):
            gt_ig = np.concatenate([np.asarray(g["gt_ignore"], dtype=bool).reshape(-1, A)[:, a] for g in gs])
            npig = int(np.count_nonzero(~gt_ig))
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                scores = np.concatenate([np.asarray(g["dt_scores"], dtype=np.float64)[:max_det] for g in gs])
                order = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([np.asarray(g["dt_match"]).reshape(-1, A, T)[:max_det, a, :] for g in gs], axis=0)[order].T      # [T, N]
                dt_ig = np.concatenate([np.asarray(g["dt_ignore"], dtype=bool).reshape(-1, A, T)[:max_det, a, :] for g in gs], axis=0)[order].T
                tp_sum = np.cumsum((dtm >= 0) & ~dt_ig, axis=1).astype(np.float64)
                fp_sum = np.cumsum((dtm < 0) & ~dt_ig, axis=1).astype(np.float64)
                nd = tp_sum.shape[1]
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]                       # non-increasing from the right
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    ok = inds < nd
                    q[ok] = pr[inds[ok]]
                    precision[t, :, k, a, m] = q
    return {"precision": precision, "recall": recall, "counts": [T, R, K, A, M]}


def _mean_valid(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize_eval(ev, thr=IOU_THRS, max_dets=MAX_DETS):
    """The 12 stats of YTVOSeval.summarize (segm) and their lines in cocoapi's layout -> (stats float64 [12], [12 lines])."""
    pr, rc = ev["precision"], ev["recall"]
    last = len(max_dets) - 1
    t50, t75 = 0, int(np.argmin(np.abs(np.asarray(thr) - 0.75)))
    rows = ([(1, None, 0, last), (1, t50, 0, last), (1, t75, 0, last), (1, None, 1, last), (1, None, 2, last), (1, None, 3, last)] +
            [(0, None, 0, m) for m in range(len(max_dets))] + [(0, None, a, last) for a in (1, 2, 3)])
    stats, lines = np.zeros(len(rows)), []
    for i, (ap, t, a, m) in enumerate(rows):
        src = pr if ap else rc
        s = src[:, :, :, a, m] if ap else src[:, :, a, m]
        if t is not None:
            s = s[t:t + 1]
        stats[i] = _mean_valid(s)
        iou = f"{thr[0]:0.2f}:{thr[-1]:0.2f}" if t is None else f"{thr[t]:0.2f}"
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, AREA_LBL[a], max_dets[m], stats[i]))
    return stats, lines


class VisEval:
    """YTVOSeval(iouType='segm', useCats=1) for `annotations` (a YouTube-VIS dict or the path of its json) and `results` (the list
    eval_utils.video_records() returns, or the path of a results json).  evaluate() -> ious, accumulate() -> eval, summarize() -> stats."""

    def __init__(self, annotations, results, device=None):
        self.annotations, self.results = _load(annotations), _load(results)
        if not isinstance(self.annotations, dict) or "videos" not in self.annotations or "categories" not in self.annotations:
            raise ValueError("annotations: expected a YouTube-VIS dict with 'videos', 'categories' and 'annotations'")
        if not isinstance(self.results, (list, tuple)):
            raise ValueError("results: expected a list of {'video_id', 'category_id', 'score', 'segmentations'} records")
        self.device = device
        self.vid_ids, self.cat_ids, self.groups = group_tracks(self.annotations, self.results)
        self.ious, self.eval, self.stats, self.lines = {}, None, None, None
        self.counters = {}
        self._flatten()

    def _flatten(self):
        """The rest of the host part: every group's tracks as a [track, frame] -> mask table, the masks as flat arrays, the pair list."""
        groups = self.groups
        sizes = {v["id"]: (int(v["height"]), int(v["width"])) for v in self.annotations["videos"]}
        # tracks: every group's ground truths, then every group's detections; masks in track order
        tracks, names, rles = [], [], []
        for g in groups:
            tracks.extend((f"annotation {a.get('id')}", g["video_id"], a["segmentations"]) for a in g["gt"])
        self._n_gt = n_gt = len(tracks)
        for g in groups:
            tracks.extend((f"result {i}", g["video_id"], r["segmentations"]) for i, r in zip(g["dt_index"], g["dt"]))
        self._track_len = np.array([len(s) for _, _, s in tracks], dtype=np.int32)
        table = np.full((len(tracks), int(self._track_len.max()) if tracks else 0), -1, dtype=np.int32)
        for t, (label, vid, segs) in enumerate(tracks):
            for f, r in enumerate(segs):
                if r is None:
                    continue
                if not isinstance(r, dict) or "counts" not in r or "size" not in r:
                    raise ValueError(f"{label} (video {vid}) frame {f}: not an RLE dict (polygons are not built)")
                if tuple(int(x) for x in r["size"]) != sizes[vid]:
                    raise ValueError(f"{label} (video {vid}) frame {f}: size {list(r['size'])} is not the video's {list(sizes[vid])}")
                table[t, f] = len(rles)
                rles.append(r)
                names.append((label, vid, f))
        self._who = lambda i: f"{names[i][0]} (video {names[i][1]}) frame {names[i][2]}"
        self._masks = flatten_masks(rles, self._who)
        if len(rles):
            table[table >= 0] = self._masks.pos[table[table >= 0]]
        self._table = table
        D = np.array([len(g["dt"]) for g in groups], dtype=np.int64)
        G = np.array([len(g["gt"]) for g in groups], dtype=np.int64)
        self._max_d, self._max_g = (int(D.max()), int(G.max())) if len(groups) else (0, 0)
        if self._max_g > MAX_GT:
            raise StmError(f"vis_eval: {self._max_g} ground-truth tracks in one (video, category) group, at most {MAX_GT}")
        self._dt_off, self._gt_off, self._pair_off = _offsets(D), _offsets(G), _offsets(D * G)
        dt_off, gt_off = self._dt_off, self._gt_off
        none = [np.zeros(0, np.int64)]
        self._pair_d = np.concatenate([np.repeat(n_gt + dt_off[k] + np.arange(D[k]), G[k]) for k in range(len(groups))] or none).astype(np.int32)
        self._pair_g = np.concatenate([np.tile(gt_off[k] + np.arange(G[k]), D[k]) for k in range(len(groups))] or none).astype(np.int32)
        gts = [a for g in groups for a in g["gt"]]
        self._crowd = np.array([int(bool(a.get("iscrowd", 0))) for a in gts], dtype=np.int32)
        self._has_file = np.array([a.get("areas") is not None for a in gts], dtype=bool)
        self._file_area = np.array([file_avg_area(a["areas"]) if a.get("areas") is not None else 0.0 for a in gts], dtype=np.float64)
        self.counters = {"masks": len(rles), "tracks": len(tracks), "pairs": int(self._pair_off[-1]), "groups": len(groups),
                         "rle_bytes": int(self._masks.s_off[-1])}

    def evaluate(self):
        """Decode, tube IoU and matching of all groups on the device: uploads, four launches (and the torch glue of avg_area), one round of
        copies.  No per-mask Python loop.  Fills `ious` and the groups' dt_match / dt_ignore / gt_ignore."""
        dev = _device(self.device)
        groups, n_gt = self.groups, self._n_gt
        dt_off, gt_off, pair_off = self._dt_off, self._gt_off, self._pair_off
        up = lambda x: _up(x, dev)
        masks = upload_masks(self._masks, dev)
        table_d, len_d = up(self._table), up(self._track_len)
        avg = track_avg_area(masks, table_d)
        gt_area = torch.where(up(self._has_file), up(self._file_area), avg[:n_gt]) if n_gt else avg[:0]
        dt_area = avg[n_gt:]
        inter, uni, iou = tube_iou(masks, table_d, len_d, up(self._pair_d), up(self._pair_g))
        dt_match, dt_ignore, gt_ignore = match_groups(iou, up(pair_off), up(dt_off.astype(np.int32)), up(gt_off.astype(np.int32)), dt_area.contiguous(),
                                                      gt_area.contiguous(), up(self._crowd), self._max_d, self._max_g)
        # the copies (the only host synchronisation of evaluate())
        status = _down(masks.status)
        raise_for_status(status, masks.pos, self._who)
        iou_h, inter_h, uni_h = _down(iou), _down(inter), _down(uni)
        dtm_h, dti_h, gti_h = _down(dt_match), _down(dt_ignore), _down(gt_ignore)
        self.dt_area, self.gt_area = _down(dt_area), _down(gt_area)
        self.ious, self.inter, self.union = {}, {}, {}
        for k, g in enumerate(groups):
            key, shape = (g["video_id"], g["category_id"]), (len(g["dt"]), len(g["gt"]))
            sl = slice(int(pair_off[k]), int(pair_off[k + 1]))
            self.ious[key], self.inter[key], self.union[key] = iou_h[sl].reshape(shape), inter_h[sl].reshape(shape), uni_h[sl].reshape(shape)
            g["dt_match"], g["dt_ignore"] = dtm_h[dt_off[k]:dt_off[k + 1]], dti_h[dt_off[k]:dt_off[k + 1]]
            g["gt_ignore"] = gti_h[gt_off[k]:gt_off[k + 1]]
        return self

    def accumulate(self):
        if any("dt_match" not in g for g in self.groups):
            raise StmError("VisEval.accumulate: run evaluate() first")
        self.eval = accumulate_groups(self.groups, self.cat_ids)
        return self

    def summarize(self, output_file=None):
        if self.eval is None:
            raise StmError("VisEval.summarize: run accumulate() first")
        self.stats, self.lines = summarize_eval(self.eval)
        for line in self.lines:
            print(line)
        if output_file is not None:
            with open(output_file, "w") as f:
                f.write("\n".join(self.lines) + "\n")
        return self.stats


def calc_metrics(anno_file, dt_file, output_file=None):
    """layers/eval_utils.py:109-119: the 12 summary numbers (float64) of the results file `dt_file` against the YouTube-VIS annotations
    `anno_file`, printed in cocoapi's layout and written to `output_file` when one is given."""
    e = VisEval(anno_file, dt_file)
    e.evaluate()
    e.accumulate()
    stats = e.summarize(output_file)
    print("finish validation")
    return stats
