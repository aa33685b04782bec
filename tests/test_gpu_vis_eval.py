"""Video mask AP on the MI355X (stmask_amd/vis_eval.py, csrc/vis_eval.hip) against the dense numpy restatement (tests/vis_eval_restate.py): the RLE
string decode, the tube IoU, the greedy matching, and the whole evaluation of the generated set.  Everything the device produces is an integer
count or a float64 quotient of two of them formed in the restatement's order, so the comparisons are exact; only the 12 summary means get a bound
(1e-12: a mean of at most 10 * 101 * K values in [0, 1] moves by at most n * 2^-53 with the summation order)."""
import numpy as np
import pytest
import torch

import vis_eval_cases as C
import vis_eval_restate as R
from stmask_amd import ops, output_utils, vis_eval
from stmask_amd.output_utils import rle_counts_to_string

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def generated():
    """The generated set, the restatement's evaluation of it (computed once, read-only) and the package's."""
    ann, res = C.generated_set()
    cat_ids, groups, ev, stats = C.check_coverage(ann, res)
    e = vis_eval.VisEval(ann, res)
    e.evaluate()
    e.accumulate()
    return {"ann": ann, "res": res, "cat_ids": cat_ids, "groups": groups, "eval": ev, "stats": stats, "pkg": e}


def _str_rle(cnts, size=None):
    return {"size": size or [1, int(sum(cnts))], "counts": rle_counts_to_string(cnts)}


def _host(ms):
    """(runs per mask as lists, area, status) of a MaskSet, in the order the masks were handed in."""
    runs, off, nr = ms.runs.cpu().numpy().view(np.uint32), ms.run_off.cpu().numpy(), ms.n_runs.cpu().numpy()
    area, st = ms.area.cpu().numpy(), ms.status.cpu().numpy()
    return [runs[off[k]:off[k] + nr[k]].tolist() for k in ms.pos], area[ms.pos], st[ms.pos]


# ---- decode ----------------------------------------------------------------------------------------------------------------------------------
def _decode_masks():
    rng = np.random.RandomState(11)
    rles = [C.rle(rng.rand(6, 8) > 0.5), C.rle(rng.rand(37, 53) > 0.4), C.rle(rng.rand(37, 53) > 0.97), C.rle(rng.rand(360, 640) > 0.5),
            C.rle(np.zeros((6, 8), dtype=bool)), C.rle(np.ones((37, 53), dtype=bool)), C.rle(np.zeros((0, 5), dtype=bool))]
    big = [2 ** 20 + 5, 3, 2 ** 15 + 9, 2 ** 15 + 1, 70000, 1, 3, 60000, 2, 1, 2 ** 21, 2 ** 15, 40, 7]     # 4- and 5-character values, negative deltas
    rles += [_str_rle(big), _str_rle([0, 2 ** 22, 1, 1]), _str_rle([5, 100, 7, 3, 2, 1, 90, 1]), _str_rle([2 ** 32 - 1], [65535, 65537])]
    rles += [C.rle(rng.rand(37, 53) > 0.5, compressed=False), {"size": [6, 8], "counts": [48]}, {"size": [6, 8], "counts": [0, 48]},
             {"size": [3, 3], "counts": [2, 0, 0, 3, 4]}]                                                       # uncompressed, zero-length runs inside
    return rles


def test_decode_runs_and_areas_equal_the_restatement():
    rles = _decode_masks()
    ms = vis_eval.pack_masks(rles, DEV)
    runs, area, status = _host(ms)
    assert not status.any(), status
    for i, r in enumerate(rles):
        want = R.counts_of(r)
        assert runs[i] == want, i
        assert int(area[i]) == sum(want[1::2]), i
        if r["size"][0] * r["size"][1] <= 4 * 2 ** 20:
            assert int(area[i]) == int(R.dense(r).sum()), i                                                   # counted pixels
    assert ms.run_list(3).tolist() == R.counts_of(rles[3])
    assert len(rles[0]["counts"]) > 0 and isinstance(rles[0]["counts"], str) and isinstance(rles[7]["counts"], bytes)     # str and bytes both enter


def test_decode_inverts_the_shipped_encoder():
    torch.manual_seed(5)
    soft = torch.rand(5, 20, 28, device=DEV)
    soft[3] = 0.0
    soft[4] = 1.0
    counts, n_runs = ops.mask_resize_rle(soft, 20, 28, 37, 53)
    rles = output_utils.encode_masks(soft, 20, 28, 37, 53)
    ms = vis_eval.pack_masks(rles, DEV)
    runs, area, status = _host(ms)
    counts, n_runs = counts.cpu().numpy(), n_runs.cpu().numpy()
    assert not status.any()
    for i in range(5):
        assert runs[i] == counts[i, :n_runs[i]].tolist(), i
        assert int(area[i]) == int(counts[i, 1:n_runs[i]:2].sum())
    assert runs[3] == [37 * 53] and runs[4] == [0, 37 * 53]


def test_malformed_strings_are_flagged_and_leave_their_neighbours_intact():
    rng = np.random.RandomState(12)
    good = [C.rle(rng.rand(37, 53) > 0.5) for _ in range(4)]
    ok = rle_counts_to_string([5, 3, 40])
    unterminated = {"size": [6, 8], "counts": ok[:-1] + bytes([((ok[-1] - 48) | 0x20) + 48])}
    negative = {"size": [6, 8], "counts": rle_counts_to_string([5, -3, 46])}
    too_big = {"size": [1, 2 ** 32 - 1], "counts": rle_counts_to_string([7, 2 ** 32, 5])}
    long_value = {"size": [6, 8], "counts": b"o" * 9 + b"1"}                        # a value of ten characters
    bad_sum = {"size": [6, 8], "counts": rle_counts_to_string([5, 3, 41])}
    bad_list = {"size": [6, 8], "counts": [5, 3, 39]}
    rles = [good[0], unterminated, good[1], negative, too_big, long_value, good[2], bad_sum, good[3], bad_list]
    ms = vis_eval.pack_masks(rles, DEV)                                                # no exception here: no host read
    runs, area, status = _host(ms)
    assert status[1] & vis_eval.RLE_UNTERMINATED and status[7] == vis_eval.RLE_SUM and status[9] == vis_eval.RLE_SUM
    assert status[3] & vis_eval.RLE_RANGE and status[4] & vis_eval.RLE_RANGE and status[5] & vis_eval.RLE_RANGE
    for i in (1, 3, 4, 5, 7, 9):
        assert runs[i] == [] and area[i] == 0
    for i, g in zip((0, 2, 6, 8), good):
        assert status[i] == 0 and runs[i] == R.counts_of(g) and int(area[i]) == int(R.dense(g).sum())
    for i, word in ((1, "ends inside a value"), (3, "outside"), (7, "sum"), (9, "sum")):
        with pytest.raises(ValueError, match=word):
            vis_eval.raise_for_status(status[i:i + 1], np.array([0]), lambda k: "mask")
    # ... and through the public interface: the record is named
    ann, res, _, _ = C.closed_form_cases()["two_gt_one_det"]
    res = [dict(res[0]), dict(res[0], segmentations=[dict(bad_sum, size=[24, 40])])]
    with pytest.raises(ValueError, match=r"result 1 \(video 1\) frame 0.*sum"):
        vis_eval.VisEval(ann, res).evaluate()
    with pytest.raises(ValueError, match="polygons"):
        vis_eval.VisEval(ann, [dict(res[0], segmentations=[{"size": [24, 40], "counts": 7}])]).evaluate()
    with pytest.raises(ValueError, match="run length outside"):
        vis_eval.pack_masks([{"size": [6, 8], "counts": [50, -2]}], DEV)
    with pytest.raises(vis_eval.StmError, match="2\\^32"):
        vis_eval.pack_masks([{"size": [65536, 65536], "counts": [2 ** 32]}], DEV)


# ---- tube IoU --------------------------------------------------------------------------------------------------------------------------------
def _tube(tracks, pairs):
    """tracks: lists of RLE dicts / None; pairs: (d, g) track indices -> host (inter, union, iou)."""
    rles, table = [], np.full((len(tracks), max(len(t) for t in tracks)), -1, dtype=np.int32)
    for t, segs in enumerate(tracks):
        for f, r in enumerate(segs):
            if r is not None:
                table[t, f] = len(rles)
                rles.append(r)
    ms = vis_eval.pack_masks(rles, DEV)
    table[table >= 0] = ms.pos[table[table >= 0]]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(DEV)
    inter, uni, iou = vis_eval.tube_iou(ms, up(table), up([len(t) for t in tracks]), up([p[0] for p in pairs]), up([p[1] for p in pairs]))
    assert not ms.status.any()
    return inter.cpu().numpy(), uni.cpu().numpy(), iou.cpu().numpy()


def test_tube_iou_equals_the_dense_count():
    rng = np.random.RandomState(13)
    rand = lambda h, w, p=0.5, compressed=True: C.rle(rng.rand(h, w) > p, compressed)
    empty = C.rle(np.zeros((24, 40), dtype=bool))
    tracks = [
        [rand(24, 40), None, rand(24, 40), rand(24, 40), None],                              # 0
        [rand(24, 40, 0.3, False), rand(24, 40, 0.3, False), None, rand(24, 40, 0.3, False), None],   # 1: uncompressed, None on its side
        [rand(24, 40), rand(24, 40)],                                                         # 2: shorter
        [empty, empty, None],                                                                 # 3
        [empty, None, empty],                                                                 # 4: with 3: u = 0
        [rand(37, 53)],                                                                       # 5: one frame
        [rand(37, 53, 0.7)],                                                                  # 6
        [rand(6, 8) if f % 7 else None for f in range(65)],                                   # 7: 65 frames
        [rand(6, 8, 0.4) if f % 5 else None for f in range(65)],                              # 8
        [rand(6, 8) for f in range(130)],                                                     # 9: 130 frames, more than two passes of the lanes
        [rand(6, 8, 0.6, False) if f % 11 else None for f in range(130)],                     # 10
        [None, None],                                                                         # 11: nothing at all
    ]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 1), (3, 4), (5, 6), (7, 8), (9, 10), (10, 9), (9, 8), (0, 0), (9, 9), (10, 10), (5, 5), (11, 0), (11, 11),
             (3, 3)]
    inter, uni, iou = _tube(tracks, pairs)
    for k, (d, g) in enumerate(pairs):
        i, u = R.tube_counts(tracks[d], tracks[g])
        assert (int(inter[k]), int(uni[k])) == (i, u), (d, g)
        want = float(i) / float(u) if u > 0 else 0.0
        assert iou[k] == want and np.float64(iou[k]).tobytes() == np.float64(want).tobytes(), (d, g)
    by = dict(zip(pairs, iou))
    assert by[(3, 4)] == 0.0 and by[(11, 11)] == 0.0 and by[(3, 3)] == 0.0 and uni[pairs.index((3, 4))] == 0
    assert by[(0, 0)] == 1.0 and by[(9, 9)] == 1.0 and by[(10, 10)] == 1.0 and by[(5, 5)] == 1.0


# ---- matching --------------------------------------------------------------------------------------------------------------------------------
def _match(groups):
    """groups: (ious [D, G], dt_area, gt_area, gt_crowd) -> per group (dt_match, dt_ignore, gt_ignore) from the device."""
    D = np.array([len(g[1]) for g in groups], dtype=np.int64)
    G = np.array([len(g[2]) for g in groups], dtype=np.int64)
    off = lambda x: np.concatenate([[0], np.cumsum(x)])
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEV)
    cat = lambda k, dt: np.concatenate([np.asarray(g[k], dtype=dt).reshape(-1) for g in groups])
    dtm, dti, gti = vis_eval.match_groups(up(cat(0, np.float64), np.float64), up(off(D * G), np.int64), up(off(D), np.int32), up(off(G), np.int32),
                                          up(cat(1, np.float64), np.float64), up(cat(2, np.float64), np.float64), up(cat(3, np.int32), np.int32),
                                          int(D.max()), int(G.max()))
    dtm, dti, gti = dtm.cpu().numpy(), dti.cpu().numpy(), gti.cpu().numpy()
    d0, g0 = off(D), off(G)
    return [(dtm[d0[k]:d0[k + 1]], dti[d0[k]:d0[k + 1]], gti[g0[k]:g0[k + 1]]) for k in range(len(groups))]


def _match_groups():
    rng = np.random.RandomState(14)
    thr = R.IOU_THRS
    small, medium, large = 100.0, 20000.0, 70000.0
    named = {
        "no_detections": (np.zeros((0, 2)), [], [small, medium], [0, 0]),
        "no_ground_truth": (np.zeros((3, 0)), [small, medium, large], [], []),
        "equal_ious_later_wins": (np.array([[0.7, 0.7, 0.2]]), [small], [small, small, small], [0, 0, 0]),
        "at_thresholds": (np.diag([0.5, thr[2], thr[8], np.nextafter(0.6, 0)]), [small] * 4, [small] * 4, [0, 0, 0, 0]),
        "gt_outside_range": (np.array([[0.9, 0.1], [0.1, 0.8]]), [small, medium], [small, medium], [0, 0]),
        "matched_to_ignored": (np.array([[0.9]]), [small], [large], [0]),
        "unmatched_outside_range": (np.array([[0.0], [0.95]]), [large, small], [small], [0]),
        "non_ignored_first_break": (np.array([[0.9, 0.6], [0.9, 0.1]]), [small, small], [medium, small], [0, 0]),
        "crowd_first_break": (np.array([[0.9, 0.6]]), [small], [small, small], [1, 0]),
        "rematchable_crowd": (np.array([[0.8], [0.7], [0.6]]), [small] * 3, [small], [1]),
        "taken_not_rematched": (np.array([[0.8], [0.7]]), [small] * 2, [small], [0]),
    }

    def random_group(D, G):
        ious = np.round(rng.rand(D, G) * 20) / 20.0 * (rng.rand(D, G) > 0.5)             # many ties, values on the threshold grid
        return (ious, rng.choice([small, medium, large, 128.0 ** 2, 256.0 ** 2], D), rng.choice([small, medium, large, 128.0 ** 2], G),
                (rng.rand(G) > 0.8).astype(int))

    named["random_lds_40x20"] = random_group(40, 20)
    named["random_global_100x30"] = random_group(100, 30)                                 # 3000 IoUs: read from global memory
    named["random_70_ground_truths"] = random_group(7, 70)                                # more than two words of taken bits
    named["random_100x100"] = random_group(100, 100)
    return named


def test_matching_equals_the_restatement():
    named = _match_groups()
    names = sorted(named)
    got = _match([named[n] for n in names])
    for n, (dtm, dti, gti) in zip(names, got):
        ious, dt_area, gt_area, crowd = named[n]
        w_dtm, w_dti, w_gti = R.match_group(ious, dt_area, gt_area, [bool(c) for c in crowd])
        assert dtm.dtype == np.int32 and dti.dtype == bool and gti.dtype == bool
        assert np.array_equal(dtm, w_dtm), n
        assert np.array_equal(dti, w_dti), n
        assert np.array_equal(gti, w_gti), n
    by = dict(zip(names, got))
    # what the named cases are there for, spelled out (area range 0 = all, 1 = small; threshold 0 = 0.5)
    assert by["equal_ious_later_wins"][0][0, 0, 0] == 1
    at = by["at_thresholds"][0][:, 0, :]
    assert at[0].tolist() == [0] + [-1] * 9 and at[1].tolist() == [1] * 3 + [-1] * 7 and at[2].tolist() == [2] * 9 + [-1] and at[3].tolist() == [3, 3] + [-1] * 8
    assert by["matched_to_ignored"][0][0, 1, 0] == 0 and by["matched_to_ignored"][1][0, 1, 0] and not by["matched_to_ignored"][1][0, 0, 0]
    assert by["unmatched_outside_range"][1][0, 1, 0] and not by["unmatched_outside_range"][1][0, 0, 0]
    assert by["non_ignored_first_break"][0][:, 1, 0].tolist() == [1, 0] and by["non_ignored_first_break"][0][:, 0, 0].tolist() == [0, -1]
    assert by["crowd_first_break"][0][0, 0, 0] == 1
    assert by["rematchable_crowd"][0][:, 0, 0].tolist() == [0, 0, 0] and by["rematchable_crowd"][1][:, 0, 0].all()
    assert by["taken_not_rematched"][0][:, 0, 0].tolist() == [0, -1]
    assert by["no_detections"][0].shape == (0, 4, 10) and by["no_ground_truth"][0].shape == (3, 4, 10) and (by["no_ground_truth"][0] == -1).all()


def test_matching_refuses_groups_beyond_its_limits():
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
    for max_d, max_g in ((101, 1), (1, 1025)):
        with pytest.raises(vis_eval.StmError, match="at most"):
            vis_eval.match_groups(z(1, torch.float64), z(2, torch.int64), z(2, torch.int32), z(2, torch.int32), z(1, torch.float64), z(1, torch.float64),
                                  z(1, torch.int32), max_d, max_g)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_generated_set_ious_and_matches_equal_the_restatement(generated):
    e, groups = generated["pkg"], generated["groups"]
    assert e.cat_ids == generated["cat_ids"]
    assert list(e.ious) == [(g["video_id"], g["category_id"]) for g in groups] and len(e.groups) == len(groups)
    for g, pg in zip(groups, e.groups):
        key = (g["video_id"], g["category_id"])
        assert e.ious[key].shape == g["ious"].shape and e.ious[key].dtype == np.float64
        assert np.array_equal(e.inter[key], g["inter"]) and np.array_equal(e.union[key], g["union"]), key
        assert np.array_equal(e.ious[key], g["ious"]), key
        assert np.array_equal(pg["dt_scores"], g["dt_scores"]), key
        assert np.array_equal(pg["dt_match"], g["dt_match"]) and np.array_equal(pg["dt_ignore"], g["dt_ignore"]), key
        assert np.array_equal(pg["gt_ignore"], g["gt_ignore"]), key
    assert np.array_equal(e.gt_area, np.concatenate([g["gt_area"] for g in groups]))
    assert np.array_equal(e.dt_area, np.concatenate([g["dt_area"] for g in groups]))
    assert e.ious[(5, 1)].shape == (100, 1)                                               # 101 -> 100


def test_generated_set_precision_recall_and_stats(generated, capsys):
    e, ev = generated["pkg"], generated["eval"]
    assert e.eval["precision"].shape == (10, 101, 3, 4, 3) and e.eval["recall"].shape == (10, 3, 4, 3)
    assert np.array_equal(e.eval["precision"], ev["precision"]) and np.array_equal(e.eval["recall"], ev["recall"])
    stats = e.summarize()
    assert stats.dtype == np.float64 and stats.shape == (12,)
    print(stats, generated["stats"])
    assert np.abs(stats - generated["stats"]).max() <= 1e-12
    assert capsys.readouterr().out.splitlines()[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % stats[0]


def test_two_runs_give_identical_bytes(generated):
    first = generated["pkg"]
    again = vis_eval.VisEval(generated["ann"], generated["res"]).evaluate().accumulate()
    for key in first.ious:
        assert first.ious[key].tobytes() == again.ious[key].tobytes()
    for a, b in zip(first.groups, again.groups):
        assert a["dt_match"].tobytes() == b["dt_match"].tobytes() and a["dt_ignore"].tobytes() == b["dt_ignore"].tobytes()
    assert first.eval["precision"].tobytes() == again.eval["precision"].tobytes() and first.eval["recall"].tobytes() == again.eval["recall"].tobytes()


def test_calc_metrics_from_files(tmp_path, capsys):
    import json
    from stmask_amd import eval_utils
    for name, (ann, res, approx, exact) in sorted(C.closed_form_cases().items()):
        a, r, out = tmp_path / f"{name}_ann.json", tmp_path / f"{name}_res.json", tmp_path / f"{name}_out.txt"
        a.write_text(json.dumps(ann))
        r.write_text(json.dumps(res))
        stats = eval_utils.calc_metrics(str(a), str(r), str(out))
        assert isinstance(stats, np.ndarray) and stats.dtype == np.float64 and stats.shape == (12,)
        for i, v in approx.items():
            assert abs(stats[i] - v) <= 1e-12, (name, i, stats[i], v)
        for i, v in exact.items():
            assert stats[i] == v, (name, i)
        assert np.abs(stats - R.stats_of(ann, res)).max() <= 1e-12
        lines = out.read_text().splitlines()
        assert len(lines) == 12 and lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % stats[0]
        assert lines[8] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % stats[8]
        printed = capsys.readouterr().out.splitlines()
        assert printed[:12] == lines and printed[12] == "finish validation"
    # nothing to evaluate launches nothing and scores -1 everywhere
    ann = C.closed_form_cases()["identical"][0]
    empty = vis_eval.VisEval(dict(ann, annotations=[]), []).evaluate().accumulate()
    assert empty.ious == {} and (empty.summarize() == -1).all()
