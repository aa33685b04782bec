"""The fp64 restatement of the temporal-fusion loss (tests/t2s_loss_restate.py) against the reference's own fp32 run of
MultiBoxLoss.track_to_segment_loss (tests/golden/t2s_loss_cases.npz, written by tests/golden/gen_t2s_loss_golden.py), and the documented
deviations and the confusions a wrong implementation would make, on constructed cases.  No GPU: tests/test_gpu_t2s_loss.py holds the kernels to
the same restatement."""
import os

import numpy as np
import pytest
import torch

import oracle
import t2s_loss_restate as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t2s_loss_cases.npz")


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLD) < 1024 * 1024
    return np.load(GOLD)


def _s(a):
    return float(np.asarray(a).reshape(-1)[0])


def _f(z, name, key):
    return torch.from_numpy(np.asarray(z[f"{name}__{key}"]))


@pytest.mark.parametrize("name", list(R.GOLDEN))
def test_restated_targets_match_the_references(gold, name):
    z = gold
    assert _s(z["boxshift_alpha"]) == R.ALPHA_B and _s(z["maskshift_alpha"]) == R.ALPHA_M
    case = R.golden_case(name, int(_s(z[f"{name}__seed"])))
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    rows = torch.nonzero(t["pos"].reshape(-1)).reshape(-1)
    assert rows.tolist() == _f(z, name, "pos_rows").tolist()                          # pos, exactly
    assert rows.numel() == int(_s(z[f"{name}__n"]))
    if rows.numel() == 0:
        assert _s(z[f"{name}__B"]) == 0.0 and _s(z[f"{name}__M"]) == 0.0
        return
    assert t["k_local"].reshape(-1)[rows].tolist() == _f(z, name, "ref_k_local").tolist()     # the next index, exactly
    ref = _f(z, name, "ref_reg")
    assert torch.equal(ref[:, :2], t["reg01"].reshape(-1, 2)[rows])                    # columns 0-1, exactly
    reg64, bound = t["reg"].reshape(-1, 4)[rows][:, 2:], t["reg_bound"].reshape(-1, 4)[rows][:, 2:]
    fin = torch.isfinite(reg64)
    assert torch.equal(ref[:, 2:].double()[~fin], reg64[~fin])
    err = (ref[:, 2:].double() - reg64).abs()[fin]
    frac = float((err / bound[fin]).max())
    print(f"\n{name}: reference reg_t columns 2-3 at {frac:.3f} of the bound (fixture: {_s(z[f'{name}__dev_reg']):.3f})")
    assert frac <= 1.0
    assert bool((t["reg"][~t["pos"]] == 0).all()) and bool((t["k_global"][~t["pos"]] == -1).all())


@pytest.mark.parametrize("name", [n for n in R.GOLDEN if n != "p300_none"])
def test_restated_losses_hold_the_references_within_the_bounds(gold, name):
    z = gold
    spec = R.GOLDEN[name]
    case = R.golden_case(name, int(_s(z[f"{name}__seed"])))
    bs, P = case["ids_t"].shape
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    rows, clip, w, n_i = R.row_weights(t["pos"])
    box_next = torch.cat([b[1] for b in case["gt_bboxes"]])[t["k_global"].reshape(-1)[rows]]
    H, W = spec["HW"]
    r = R.restate_losses(_f(z, name, "ref_bbox_reg"), _f(z, name, "ref_reg"), _f(z, name, "ref_bce"), box_next, w, n_i[clip], bs, H, W,
                         R.ALPHA_B, R.ALPHA_M)
    B, M = _s(z[f"{name}__B"]), _s(z[f"{name}__M"])
    if name == "p300_zero_width":                            # log(0) in the target, a division by zero in the mask term: +inf, as in the reference
        assert B == float("inf") and M == float("inf") and float(r["B"]) == float("inf") and float(r["M"]) == float("inf")
        return
    fb, fm = abs(B - float(r["B"])) / float(r["B_bound"]), abs(M - float(r["M"])) / float(r["M_bound"])
    print(f"\n{name}: reference B_shift at {fb:.3f}, M_shift at {fm:.3f} of the bound")
    assert fb <= 1.0 and fm <= 1.0
    assert r["min_kink"] > R.KINK


@pytest.mark.parametrize("name", ["p37", "p257_b3"])
def test_composition_holds_the_reference_end_to_end(gold, name):
    """The fp64 composition (RoIAlign, stand-in net, mask, BCE, reductions) against the reference's fp32 losses and parameter gradients: the
    deviation stored in the fixture is what this run finds again; it is the yardstick of the GPU test's end-to-end tolerance."""
    z = gold
    spec = R.GOLDEN[name]
    case = R.golden_case(name, int(_s(z[f"{name}__seed"])))
    c = R.compose(case, R.StandInNet(R.C_FEAT, spec["M"], R.NET_SEED).double(), oracle.decode, R.ALPHA_B, R.ALPHA_M)
    dl = max(abs(_s(z[f"{name}__B"]) - float(c["B"])) / abs(float(c["B"])), abs(_s(z[f"{name}__M"]) - float(c["M"])) / abs(float(c["M"])))
    dg = max(float((_f(z, name, "grad_" + k.replace(".", "_")).double() - g).abs().max() / g.abs().max()) for k, g in c["grads"].items())
    assert dl == pytest.approx(_s(z[f"{name}__e2e_loss"]), rel=1e-6, abs=1e-12)
    assert dg == pytest.approx(_s(z[f"{name}__e2e_grad"]), rel=1e-6, abs=1e-12)
    assert dl < 16 * R.EPS and dg < 64 * R.EPS                # fp32 through ~10^2-term sums: a few eps for the losses, more for the gradients


def _encode64(nxt, ref):
    n, r = nxt.double(), ref.double()
    cx, cy, w, h = (r[2] + r[0]) / 2, (r[3] + r[1]) / 2, r[2] - r[0], r[3] - r[1]
    return torch.stack([((n[0] + n[2]) / 2 - cx) / (R.V0 * w), ((n[1] + n[3]) / 2 - cy) / (R.V0 * h), torch.log((n[2] - n[0]) / w) / R.V1,
                        torch.log((n[3] - n[1]) / h) / R.V1])


@pytest.mark.parametrize("name", ["tiles_259", "images_300"])
def test_list_cases_put_the_shift_positives_where_pos_loss_restate_lists_them(name):
    """The two constructed specs for the target kernel's own tile counts: more than 256 tiles of 256 priors, 2 to 3 boxes per frame; the
    shift-positives are exactly the list case's positives (what each reaches is pinned in tests/test_pos_loss_cpu.py); priors with an id that
    one frame lacks, and with a negative id, stand beside them."""
    import pos_loss_restate as PR
    spec = R.constructed_cases()[name]
    B, P, per_image = PR.list_positives(name)
    assert len(spec["clips"]) == B and spec["P"] == P and B * -(-P // 256) > 256
    assert all(2 <= len(c["ref"]) <= 3 and 2 <= len(c["nxt"]) <= 3 for c in spec["clips"])
    case = R.draw_case(spec, spec["seed"])
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    assert [row.nonzero()[:, 0].tolist() for row in t["pos"]] == per_image
    assert torch.equal(t["pos"], PR.list_targets(name) > 0)
    other = (case["ids_t"] != 0) & ~t["pos"]
    assert bool((case["ids_t"][other] > 0).any()) and bool((case["ids_t"][other] < 0).any())
    kg = t["k_global"][t["pos"]]
    assert len(set(kg.tolist())) > B // 2 and bool(torch.isfinite(t["reg"]).all())


def test_duplicate_ids_resolve_to_the_last_reference_and_the_first_next_index():
    case = R.draw_case(R.constructed_cases()["duplicates"], 41001)          # ref ids [4, 6, 4], next ids [6, 4, 6]
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    br, bn = case["gt_bboxes"][0]
    for p in range(37):
        idv = int(case["ids_t"][0, p])
        if idv == 4:
            assert int(t["k_local"][0, p]) == 1 and torch.equal(t["reg"][0, p], _encode64(bn[1], br[2]))        # ref index 2, not 0
        elif idv == 6:
            assert int(t["k_local"][0, p]) == 0 and torch.equal(t["reg"][0, p], _encode64(bn[0], br[1]))        # next index 0, not 2
        else:
            assert not bool(t["pos"][0, p])
    assert int(t["pos"].sum()) == 6


def test_a_positive_id_absent_from_the_reference_frame_is_not_shift_positive():
    case = R.draw_case(R.constructed_cases()["absent_in_ref"], 41002)        # ref ids [3], next ids [9, 3]
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    assert int((case["ids_t"] == 9).sum()) == 4 and not bool(t["pos"][case["ids_t"] == 9].any())
    assert bool(t["pos"][case["ids_t"] == 3].all()) and int(t["pos"].sum()) == 2
    assert set(t["k_global"][case["ids_t"] == 3].tolist()) == {1}


def test_reference_and_next_frame_are_not_interchangeable():
    case = R.draw_case(R.constructed_cases()["swap"], 41003)                 # ref ids [2, 1], next ids [1, 5]
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    ids = case["ids_t"]
    assert bool(t["pos"][ids == 1].all()) and not bool(t["pos"][ids == 2].any()) and not bool(t["pos"][ids == 5].any())
    br, bn = case["gt_bboxes"][0]
    want = _encode64(bn[0], br[1])
    assert all(torch.equal(row, want) for row in t["reg"][ids == 1]) and set(t["k_local"][ids == 1].tolist()) == {0}
    sw = R.restate_targets(ids, [[bn, br]], [[case["gt_ids"][0][1], case["gt_ids"][0][0]]])
    assert torch.equal(sw["pos"], t["pos"])                                  # the same priors ...
    assert set(sw["k_local"][ids == 1].tolist()) == {1}                      # ... but the other index
    assert float((sw["reg"][ids == 1] - t["reg"][ids == 1]).abs().min()) > 1e-3          # ... and the opposite shift


def test_the_mean_runs_over_the_rows_of_a_clip_then_over_the_clips():
    case = R.draw_case(R.constructed_cases()["uneven"], 41004)               # 1 shift-positive in clip 0, 6 in clip 1
    t = R.restate_targets(case["ids_t"], case["gt_bboxes"], case["gt_ids"])
    rows, clip, w, n_i = R.row_weights(t["pos"])
    assert n_i.tolist() == [1, 6] and w.tolist() == [1.0] + [1.0 / 6] * 6
    g = torch.Generator().manual_seed(5)
    bbox_reg, bce = torch.randn(7, 4, generator=g), 50 * torch.rand(7, generator=g)
    box = torch.cat([b[1] for b in case["gt_bboxes"]])[t["k_global"].reshape(-1)[rows]]
    r = R.restate_losses(bbox_reg, t["reg"].reshape(-1, 4)[rows], bce, box, w, n_i[clip], 2, 24, 40, 5.0, 6.125)
    d = (bbox_reg.double() - t["reg"].reshape(-1, 4)[rows]).abs()
    rowB = torch.where(d < 1, 0.5 * d * d, d - 0.5).sum(1)
    by_clip = 5.0 / 2 * (rowB[0] + rowB[1:].mean())
    by_rows = 5.0 * rowB.mean()
    assert float(r["B"]) == pytest.approx(float(by_clip), rel=1e-14)
    assert abs(float(by_rows) - float(by_clip)) > 1e-3 * float(by_clip)
    bd = box.double()
    term = bce.double() / ((bd[:, 2] - bd[:, 0]) * 40) / ((bd[:, 3] - bd[:, 1]) * 24)
    assert float(r["M"]) == pytest.approx(float(6.125 / 2 * (term[0] + term[1:].mean())), rel=1e-14)
    # the adjoint is the derivative of the forward (central differences in double)
    e = 1e-6
    for (i, c) in ((0, 1), (3, 2)):
        up, dn = bbox_reg.double().clone(), bbox_reg.double().clone()
        up[i, c] += e
        dn[i, c] -= e
        args = (t["reg"].reshape(-1, 4)[rows], bce, box, w, n_i[clip], 2, 24, 40, 5.0, 6.125)
        num = (R.restate_losses(up, *args)["B"] - R.restate_losses(dn, *args)["B"]) / (2 * e)
        assert float(r["grad_reg"][i, c]) == pytest.approx(float(num), rel=1e-6)
    assert torch.allclose(r["grad_bce"], 6.125 / 2 * w / ((bd[:, 2] - bd[:, 0]) * 40) / ((bd[:, 3] - bd[:, 1]) * 24), rtol=1e-14)
