"""The geometry cases of tests/geometry_cases.py on the CPU: the oracle (the GPU tests' yardstick for forward values) against the fp64 four-corner
restatement at every case, the inputs' position classes, and the proof that each case can tell a swapped axis -- so that test_gpu_geometry.py
stands on references that agree with each other at unequal stride / padding / dilation pairs, and on inputs that would expose the bug it is for."""
import pytest
import torch

import autograd_restate as R
import geometry_cases as G
import oracle


def _bound_ok(got, ref, mag):
    """test_gpu_autograd_edges._check_forward's bound: |y - y64| <= 1e-5 * sum|terms| + 1e-6 (the oracle accumulates in double, returns fp32)."""
    return ((got.double() - ref).abs() / (1e-5 * mag + 1e-6)).max().item()


@pytest.mark.parametrize("c", G.DEFORM_CASES, ids=G.case_id)
def test_oracle_matches_the_fp64_restatement(c):
    for with_mask in (True, False):
        x, off, mask, w, b, _ = G.deform_inputs(c, with_mask=with_mask)
        am = None if mask is None else mask.abs()
        args = (c["st"], c["pad"], c["dl"], c["dg"])
        y = oracle.deform_conv(x, off, mask, w, b, *args)
        ref = R.deform_conv_corners(x.double(), off.double(), None if mask is None else mask.double(), w.double(), b.double(), *args)
        mag = R.deform_conv_corners(x.double().abs(), off.double(), None if am is None else am.double(), w.double().abs(), b.double().abs(), *args)
        assert y.shape == ref.shape == (c["B"], c["O"], *G.out_hw(c))
        worst = _bound_ok(y, ref, mag)
        assert worst <= 1.0, f"deform_conv mask={with_mask}: worst |y - y64| / bound = {worst:.3f}"
        cols = oracle.deform_im2col(x, off, mask, c["k"], c["st"], c["pad"], c["dl"], c["dg"])
        # the restatement's columns: its convolution with one unit weight per (channel, tap)
        CK = c["C"] * c["k"][0] * c["k"][1]
        eye = torch.eye(CK, dtype=torch.float64).view(CK, c["C"], *c["k"])
        ref_c = R.deform_conv_corners(x.double(), off.double(), None if mask is None else mask.double(), eye, None, *args).flatten(2)
        mag_c = R.deform_conv_corners(x.double().abs(), off.double(), None if am is None else am.double(), eye, None, *args).flatten(2)
        assert cols.shape == ref_c.shape
        worst = _bound_ok(cols, ref_c, mag_c)
        assert worst <= 1.0, f"deform_im2col mask={with_mask}: worst |col - col64| / bound = {worst:.3f}"
        assert torch.equal(G.columns_fp64(c, x, off, mask), ref_c)          # the swap model below starts from the same columns


@pytest.mark.parametrize("c", G.DEFORM_TABLE, ids=G.case_id)
def test_fixed_table_offsets_reach_every_position_class(c):
    _, off, _, _, _, _ = G.deform_inputs(c)
    for axis, shares in zip("yx", G.position_shares(c, off)):
        assert min(shares.values()) >= 0.01, (axis, shares)
    assert off.std() > 1.0


@pytest.mark.parametrize("c", G.DEFORM_CASES, ids=G.case_id)
def test_every_unequal_pair_is_told_apart(c):
    """For each pair with unequal values: (1) the reference with that pair transposed has another output shape or differs by more than 1e-2
    somewhere; (2) the columns computed on the TRUE output grid with the transposed pair in the sample positions -- what a kernel with sh for sw
    would write, sizes unchanged -- differ by more than 1e-2 too."""
    x, off, mask, w, b, _ = G.deform_inputs(c)
    args = (c["st"], c["pad"], c["dl"], c["dg"])
    ref = R.deform_conv_corners(x.double(), off.double(), mask.double(), w.double(), b.double(), *args)
    cols = G.columns_fp64(c, x, off, mask)
    for which in G.unequal_pairs(c):
        t = G.transposed(c, which)
        if G.out_hw(t) == G.out_hw(c):
            other = R.deform_conv_corners(x.double(), off.double(), mask.double(), w.double(), b.double(), t["st"], t["pad"], t["dl"], t["dg"])
            assert (other - ref).abs().max().item() > 1e-2, which
        assert (G.columns_fp64(c, x, off, mask, positions=t) - cols).abs().max().item() > 1e-2, which


def test_the_table_covers_what_it_claims():
    T = G.DEFORM_TABLE
    assert len(T) >= 14 and len(G.DEFORM_DRAWS) == 40
    assert len({c["name"] for c in G.DEFORM_CASES}) == len(G.DEFORM_CASES)
    hw = [G.out_hw(c) for c in T]
    same = lambda c: tuple(d * (k - 1) // 2 for d, k in zip(c["dl"], c["k"]))
    assert any(c["st"][0] > c["st"][1] for c in T) and any(c["st"][0] < c["st"][1] for c in T)
    assert any(c["dl"][0] > c["dl"][1] for c in T) and any(c["dl"][0] < c["dl"][1] for c in T)
    assert any(0 in c["pad"] for c in T) and any(c["pad"] == (0, 0) for c in T)
    assert any(c["pad"][0] > same(c)[0] or c["pad"][1] > same(c)[1] for c in T)
    assert any(c["k"][0] == c["k"][1] and c["pad"][0] != c["pad"][1] for c in T)
    assert {(1, 1), (1, 3), (3, 1), (3, 3), (3, 5), (5, 3), (7, 7)} <= {c["k"] for c in T}
    assert {1, 2, 4} <= {c["dg"] for c in T}
    assert any(h == 1 for h, _ in hw) and any(w == 1 for _, w in hw)
    assert any(h * w % 4 == 0 for h, w in hw) and any(h * w % 4 != 0 for h, w in hw)
    assert all(c["H"] != c["W"] for c in T) and sum(c["B"] >= 2 for c in T) > len(T) // 2
    for c in T:
        assert G.auto_route(c) == c["route"], c["name"]
    assert {"direct", "v2", "v3", "v3s2"} <= {c["route"] for c in T}
    assert all(4 * c["B"] * c["C"] * c["k"][0] * c["k"][1] * h * w <= 6 << 20 for c, (h, w) in zip(T, hw))      # columns: a few MB at most
    # the draws reach unequal pairs of every kind too
    D = G.DEFORM_DRAWS
    for which in ("st", "pad", "dl"):
        assert sum(c[which][0] > c[which][1] for c in D) >= 3 and sum(c[which][0] < c[which][1] for c in D) >= 3, which


def test_roi_and_correlation_tables():
    for scale in G.ROI_SCALES:
        r = G.rois(scale)
        assert set(r[:, 0].tolist()) == {0.0, 1.0, 2.0} and r[:, 0].tolist() != sorted(r[:, 0].tolist())
        m = r[:, 1:] * scale                                                   # map coordinates
        assert ((m[:, 2] - m[:, 0]) <= 2 * G.ROI_W).all() and ((m[:, 3] - m[:, 1]) <= 2 * G.ROI_H).all() and torch.isfinite(r).all()
        assert (m[:, 0] < 0).any() and (m[:, 1] < 0).any() and (m[:, 2] > G.ROI_W).any() and (m[:, 3] > G.ROI_H).any()
        assert ((m[:, 2] == m[:, 0]) & (m[:, 3] == m[:, 1])).any()
    cases = G.roi_cases()
    assert {c["scale"] for c in cases} == set(G.ROI_SCALES) and {c["out"] for c in cases} == set(G.ROI_OUTS)
    assert {c["C"] for c in cases} == set(G.ROI_CHANNELS) and {(c["sr"], c["aligned"]) for c in cases} == {(s, a) for s in range(5) for a in (True, False)}
    assert {(c["scale"], c["out"]) for c in cases} == {(s, o) for s in G.ROI_SCALES for o in G.ROI_OUTS}
    C = G.CORR_CASES
    assert {c["P"] for c in C} == {1, 3, 9, 13, 21} and {c["dil"] for c in C} == {1, 2, 3} and all(c["B"] >= 2 for c in C)
    for key in ("W", "C"):
        assert any(c[key] % 4 == 0 for c in C) and any(c[key] % 4 for c in C)
    # the RoI oracle and the restatement agree on these RoIs (the GPU test's forward and backward yardsticks): the forward bound, 1e-5
    feat = torch.randn(G.ROI_B, 3, G.ROI_H, G.ROI_W, generator=torch.Generator().manual_seed(5))
    for c in cases[:10]:
        r = G.rois(c["scale"])
        a = oracle.roi_align(feat, r, c["out"], c["scale"], c["sr"], "avg", c["aligned"])
        b = R.roi_align(feat.double(), r, c["out"], c["scale"], c["sr"], c["aligned"])
        assert (a.double() - b).abs().max().item() < 1e-5, c["name"]
