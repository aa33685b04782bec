"""Video mask AP without a device: the numpy restatement (tests/vis_eval_restate.py, the yardstick of the GPU tests) against cases whose scores are
known on paper, the package's accumulate / summarize fed the restatement's match arrays, and the host's parsing and grouping rules."""
import numpy as np
import pytest

import vis_eval_cases as C
import vis_eval_restate as R
from stmask_amd import eval_utils, vis_eval
from stmask_amd._lib import StmError
from stmask_amd.output_utils import rle_counts_to_string

CASES = C.closed_form_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_cases_through_the_restatement_and_the_package_accumulate(name):
    ann, res, approx, exact = CASES[name]
    cat_ids, groups = R.evaluate(ann, res)
    ev = R.accumulate(groups, cat_ids)
    stats = R.summarize(ev)
    ev_pkg = vis_eval.accumulate_groups(groups, cat_ids)
    stats_pkg, lines = vis_eval.summarize_eval(ev_pkg)
    assert ev_pkg["precision"].shape == (10, 101, 1, 4, 3) and ev_pkg["recall"].shape == (10, 1, 4, 3)
    assert np.array_equal(ev["precision"], ev_pkg["precision"]) and np.array_equal(ev["recall"], ev_pkg["recall"])
    assert stats.dtype == stats_pkg.dtype == np.float64 and stats.shape == stats_pkg.shape == (12,)
    for s in (stats, stats_pkg):
        for i, v in approx.items():
            assert abs(s[i] - v) <= 1e-12, (name, i, s[i], v)
        for i, v in exact.items():
            assert s[i] == v, (name, i, s[i], v)
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % stats[0]
    assert lines[1].startswith(" Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = ")
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = %0.3f" % stats[6]
    assert lines[11].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = ")


def test_identical_detection_has_precision_one_over_one_plus_epsilon():
    ann, res, _, _ = CASES["identical"]
    cat_ids, groups = R.evaluate(ann, res)
    ev = R.accumulate(groups, cat_ids)
    p = ev["precision"][:, :, 0, 0, 2]
    assert np.all(p == 1.0 / (1.0 + 2.0 ** -52)) and np.all(p != 1.0)
    assert np.all(ev["precision"][:, :, 0, 2:, :] == -1) and np.all(ev["recall"][:, 0, 2:, :] == -1)
    assert groups[0]["inter"][0, 0] == groups[0]["union"][0, 0] == 200 and groups[0]["ious"][0, 0] == 1.0


def test_iou_76_over_124_matches_the_first_three_thresholds():
    ann, res, _, _ = CASES["iou_76_124"]
    _, groups = R.evaluate(ann, res)
    g = groups[0]
    assert (g["inter"][0, 0], g["union"][0, 0]) == (76, 124)
    assert g["dt_match"][0, 0, :].tolist() == [0, 0, 0] + [-1] * 7


def test_iou_exactly_at_a_threshold():
    """`iou < best` skips, so an IoU equal to the threshold matches: 1/2 at t = 0.5.  The thresholds are numpy.linspace(.5, .95, 10) bit for bit.
    Its third value is the double nearest 3/5 (0.5 + 2 * (0.45 / 9) rounds to 0.6, not to 0.6000000000000001, which is what 0.5 + 0.05 + 0.05
    gives), so an IoU of exactly 60/100 matches at the third threshold too, as it does in YTVOSeval; the ninth value is 0.8999999999999999, one
    unit in the last place below 9/10."""
    thr = R.IOU_THRS
    assert np.array_equal(thr, vis_eval.IOU_THRS)
    assert thr[0] == 0.5 and thr[2] == 3.0 / 5.0 and thr[2] != 0.5 + 0.05 + 0.05 and thr[8] == np.nextafter(0.9, 0) and thr[5] == 0.75
    gt, half, three_fifths = C.threshold_pairs()
    ann = C._anns([C._video(1, 24, 40, 1)], [1], [C._ann(1, 1, 1, [gt])])
    for det, i, matched in ((half, 50, [0] + [-1] * 9), (three_fifths, 60, [0, 0, 0] + [-1] * 7)):
        _, groups = R.evaluate(ann, [C._res(1, 1, 0.5, [det])])
        g = groups[0]
        assert (g["inter"][0, 0], g["union"][0, 0]) == (i, 100) and g["ious"][0, 0] == i / 100.0
        assert g["dt_match"][0, 0, :].tolist() == matched
    # one unit in the last place decides: a block just under the third threshold stops at the second
    dtm, _, _ = R.match_group(np.array([[np.nextafter(0.6, 0)]]), [100.0], [100.0], [False])
    assert dtm[0, 0, :].tolist() == [0, 0] + [-1] * 8


def test_string_decoder_round_trips_the_package_encoder():
    rng = np.random.RandomState(3)
    lists = [[0, 48], [48], [5, 3, 40], [1, 2, 3, 4, 5, 6, 7, 20], [0, 2 ** 15 + 7, 3, 2 ** 20 + 11, 2 ** 20 + 12, 1, 2 ** 31, 9, 2 ** 32 - 1, 4],
             [70000, 1, 3, 60000, 2, 1], rng.randint(0, 5000, size=301).tolist()]
    for cnts in lists:
        s = rle_counts_to_string(cnts)
        assert R.string_to_counts(s) == cnts and R.string_to_counts(s.decode()) == cnts
    # 4- and 5-character values, negative deltas
    assert len(rle_counts_to_string([2 ** 15])) == 4 and len(rle_counts_to_string([2 ** 20])) == 5
    with pytest.raises(ValueError):
        R.string_to_counts(rle_counts_to_string([5, 3])[:-1] + b"o")          # continuation bit on the last character
    m = np.random.RandomState(4).rand(37, 53) > 0.6
    assert np.array_equal(R.dense(C.rle(m)).reshape(53, 37).T, m) and np.array_equal(R.dense(C.rle(m, compressed=False)).reshape(53, 37).T, m)


def test_generated_set_covers_what_it_is_built_for():
    ann, res = C.generated_set()
    cat_ids, groups, ev, stats = C.check_coverage(ann, res)
    ev_pkg = vis_eval.accumulate_groups(groups, cat_ids)
    assert np.array_equal(ev["precision"], ev_pkg["precision"]) and np.array_equal(ev["recall"], ev_pkg["recall"])
    assert np.abs(vis_eval.summarize_eval(ev_pkg)[0] - stats).max() <= 1e-12
    ann2, res2 = C.generated_set()
    assert ann2 == ann and res2 == res                                        # seeded: the same set every time


def test_grouping_rules():
    ann, res = C.generated_set()
    vid_ids, cat_ids, groups = vis_eval.group_tracks(ann, res)
    ref_cats, ref_groups = R.evaluate(ann, res)
    assert cat_ids == ref_cats == [1, 2, 3] and vid_ids == [1, 2, 3, 4, 5, 6]
    assert [(g["video_id"], g["category_id"]) for g in groups] == [(g["video_id"], g["category_id"]) for g in ref_groups]
    for g, r in zip(groups, ref_groups):
        assert (len(g["dt"]), len(g["gt"])) == r["ious"].shape and len(g["dt"]) <= 100
        assert np.array_equal(g["dt_scores"], r["dt_scores"]) and np.all(np.diff(g["dt_scores"]) <= 0)
        assert [res[i] is d for i, d in zip(g["dt_index"], g["dt"])] == [True] * len(g["dt"])
        ties = [g["dt_index"][i] < g["dt_index"][i + 1] for i in range(len(g["dt"]) - 1) if g["dt_scores"][i] == g["dt_scores"][i + 1]]
        assert all(ties)                                                      # stable: equal scores keep the file's order
    big = [g for g in groups if (g["video_id"], g["category_id"]) == (5, 1)][0]
    assert len(big["dt"]) == 100
    cut = set(i for i, r in enumerate(res) if (r["video_id"], r["category_id"]) == (5, 1)) - set(big["dt_index"])
    assert cut == {len(res) - 1}                                              # the last of the tied tail is the one that is cut
    # an unknown category is dropped, an unknown video is an error
    extra = dict(res[0], category_id=77)
    assert [len(g["dt"]) for g in vis_eval.group_tracks(ann, res + [extra])[2]] == [len(g["dt"]) for g in groups]
    with pytest.raises(ValueError, match="video_id 99"):
        vis_eval.group_tracks(ann, res + [dict(res[0], video_id=99)])
    assert vis_eval.file_avg_area([None, 0, 10, 20]) == 15.0 and vis_eval.file_avg_area([None, 0]) == 0.0 and vis_eval.file_avg_area([]) == 0.0


def test_interface_and_refusals_without_a_device():
    assert eval_utils.calc_metrics is vis_eval.calc_metrics and eval_utils.VisEval is vis_eval.VisEval
    import inspect
    assert list(inspect.signature(vis_eval.calc_metrics).parameters) == ["anno_file", "dt_file", "output_file"]
    ann, res, _, _ = CASES["identical"]
    with pytest.raises(ValueError):
        vis_eval.VisEval({"videos": []}, res)
    with pytest.raises(ValueError):
        vis_eval.VisEval(ann, {"not": "a list"})
    e = vis_eval.VisEval(ann, res, device="cpu")
    with pytest.raises(StmError, match="no CPU fallback"):
        e.evaluate()
    with pytest.raises(StmError):
        e.accumulate()
    with pytest.raises(StmError):
        e.summarize()
    with pytest.raises(StmError, match="no CPU fallback"):
        vis_eval.pack_masks([{"size": [2, 2], "counts": [4]}], device="cpu")
    source = open(vis_eval.__file__).read() + open(eval_utils.__file__).read()
    assert "import pycocotools" not in source and "from pycocotools" not in source and "import cocoapi" not in source
