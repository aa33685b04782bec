"""CPU checks of the OHEM class-confidence loss (no kernel runs): the fp64 restatement of the conventions (tests/conf_loss_restate.py) against
the reference's own fp32 outputs (tests/golden/conf_loss_cases.npz), hand-worked and constructed cases of the conventions, and the API surface.
tests/test_gpu_conf_loss.py holds the kernels to the same restatement."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import conf_loss_restate as R
from conftest import ROOT
from stmask_amd import _lib, autograd, layers, ops

Z = np.load(os.path.join(ROOT, "tests", "golden", "conf_loss_cases.npz"))
RATIO, ALPHA = int(R.scalar(Z["ratio"])), R.scalar(Z["conf_alpha"])
GOLDEN = [str(n) for n in Z["case_names"]]
CASES = R.constructed_cases()


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_the_reference(name):
    """The selected set exactly; the reference's fp32 loss and gradient within the derived bounds (the observed fraction of the bound is printed;
    the largest over the cases is in INTEGRATION.md section 14)."""
    conf, conf_t = R.golden_case(Z, name)
    assert R.scalar(Z[f"{name}__margin"]) > 1e-4
    r = R.restate(conf, conf_t, RATIO, ALPHA, "reference")
    assert abs(r["margin"] - R.scalar(Z[f"{name}__margin"])) < 1e-6
    neg = torch.from_numpy(np.unpackbits(Z[f"{name}__neg"])[:r["N"]].astype(bool))
    assert torch.equal(neg, r["neg"])
    kept = torch.from_numpy(Z[f"{name}__kept"].astype(np.int64))
    assert torch.equal(kept, r["keep"].nonzero()[:, 0])
    dev_loss = float((torch.from_numpy(Z[f"{name}__loss"]).double() - r["loss"]).abs() / r["loss_bound"])
    dev_grad = float(((torch.from_numpy(Z[f"{name}__grad_kept"]).double() - r["grad"][kept]).abs() / r["grad_bound"][kept, None]).max())
    print(f"{name}: reference fp32 / bound: loss {dev_loss:.3f}, gradient {dev_grad:.3f}")
    assert dev_loss <= 1.0 and dev_grad <= 1.0
    # the aligned form is another number (about 1e-4 .. 1e-2 relative), except where every image has the same number of positives
    ra = R.restate(conf, conf_t, RATIO, ALPHA, "aligned")
    assert torch.equal(ra["neg"], r["neg"])
    assert abs(float(ra["loss"] / r["loss"]) - R.scalar(Z[f"{name}__aligned_over_reference"])) < 1e-12


def test_hand_worked_six_rows():
    """B = 2, P = 3, C = 2, logits [0, d].  Image 0 has one positive (weight 1), image 1 two (weight 1/2 each); all three negatives are selected
    (k = min(9, 5)), w_neg = 3 * 2 / 3 = 2.  Kept rows in index order: n p n | p p n.
    reference: weights [1, 1/2, 1/2, 2, 2, 2] by position;  aligned: [2, 1, 2, 1/2, 1/2, 2]."""
    ln = math.log
    d = torch.tensor([0.0, ln(3), 0.0, 0.0, ln(3), ln(3)], dtype=torch.float64)
    conf = torch.stack([torch.zeros(6, dtype=torch.float64), d], 1).view(2, 3, 2)
    conf_t = torch.tensor([[0, 1, 0], [1, 1, 0]])
    ce = [ln(2), ln(4 / 3), ln(2), ln(2), ln(4 / 3), ln(4)]
    ref = R.restate(conf, conf_t, 3, 1.0, "reference")
    ali = R.restate(conf, conf_t, 3, 1.0, "aligned")
    assert ref["k"] == 5 and ref["num_neg"] == 3 and ref["neg"].tolist() == [True, False, True, False, False, True]
    assert ref["w"].tolist() == [1, 0.5, 0.5, 2, 2, 2] and ali["w"].tolist() == [2, 1, 2, 0.5, 0.5, 2]
    assert abs(float(ref["loss"]) - sum(w * c for w, c in zip([1, 0.5, 0.5, 2, 2, 2], ce)) / 4) < 1e-14
    assert abs(float(ref["loss"]) - (7.5 * ln(2) + 2.5 * ln(4 / 3)) / 4) < 1e-14
    assert abs(float(ali["loss"]) - (8.5 * ln(2) + 1.5 * ln(4 / 3)) / 4) < 1e-14
    # row 1: positive of class 1 with softmax (1/4, 3/4): gradient w * (p - onehot) / 4
    assert torch.allclose(ref["grad"][1], torch.tensor([0.25, -0.25], dtype=torch.float64) * 0.5 / 4, atol=1e-15)
    assert torch.allclose(ali["grad"][1], torch.tensor([0.25, -0.25], dtype=torch.float64) * 1.0 / 4, atol=1e-15)


def test_restatement_gradient_is_autograd_of_its_loss():
    conf, conf_t = CASES["k_exceeds"]
    for mode in ("reference", "aligned"):
        r = R.restate(conf, conf_t, RATIO, ALPHA, mode, g=0.7)
        x = conf.double().view(-1, conf.shape[-1]).requires_grad_(True)
        kept = r["keep"].nonzero()[:, 0]
        ce = torch.nn.functional.cross_entropy(x[kept], conf_t.view(-1)[kept], reduction="none")
        loss = ALPHA * (r["w"][kept] * ce).sum() / (RATIO + 1)
        assert abs(float(loss.detach()) - float(r["loss"])) < 1e-12
        (0.7 * loss).backward()
        assert torch.allclose(x.grad, r["grad"], atol=1e-14)


def test_ties_at_the_cut_go_to_the_lower_index():
    conf, conf_t = CASES["ties"]
    r = R.restate(conf, conf_t, RATIO, ALPHA)
    s = r["score"]
    assert r["k"] == 12 and r["margin"] == 0.0 and s[255] == s[256] == s[299] == s[300]
    assert int((s > s[255]).sum()) == 10
    assert r["neg"][[255, 256, 299, 300]].tolist() == [True, True, False, False] and r["num_neg"] == 12


# name -> what the case exists for: (scan chunk over its tiles, scan chunk over its images, rows the score kernel stages at a time)
SCAN_PATHS = {"rows_chunk2": (2, 1, 256), "rows_chunk4": (4, 1, 256), "images_300": (1, 2, 256), "c81": (1, 1, 128), "c60": (1, 1, 192),
              "ties_across_chunks": (2, 1, 256), "ties_cut_at_tile_end": (2, 1, 256)}


@pytest.mark.parametrize("name", list(SCAN_PATHS))
def test_scan_cases_reach_what_they_exist_for(name):
    """More than 256 tiles or images, or a staging count of 128 / 192; a margin at the cut for the drawn cases; positives at both ends."""
    conf, conf_t = CASES[name]
    r = R.restate(conf, conf_t, RATIO, ALPHA)
    tiles = -(-r["N"] // R.TILE)
    assert (R.scan_chunk(tiles), R.scan_chunk(r["B"]), R.stage_rows(r["C"])) == SCAN_PATHS[name]
    assert (tiles > 256) == (SCAN_PATHS[name][0] > 1) and (r["B"] > 256) == (SCAN_PATHS[name][1] > 1)
    assert 0 < r["k"] < r["N"] and r["num_neg"] == r["k"]
    if name in R.SCAN_DRAWS:
        assert r["margin"] > R.MARGIN
    pos_tile = torch.unique(r["pos"].nonzero()[:, 0] // R.TILE)
    npos_img = r["pos"].view(r["B"], r["P"]).sum(1)
    if name in ("rows_chunk2", "rows_chunk4"):                          # the kept rows' ranks matter to the last tile
        assert int(pos_tile[0]) == 0 and int(pos_tile[-1]) == tiles - 1
        last_of_image = (torch.arange(1, r["B"] + 1) * r["P"] - 1) // R.TILE
        assert all(int(v) in pos_tile.tolist() for v in last_of_image[-2:])
        assert int((npos_img == 0).sum()) >= 1 and len(set(npos_img.tolist())) > 4             # the two weight modes differ
        ra = R.restate(conf, conf_t, RATIO, ALPHA, "aligned")
        assert not torch.equal(ra["w"], r["w"])
        kept = r["keep"].nonzero()[:, 0]                                # ... and the rank decides the weight past the 256th tile
        assert int(kept[r["num_pos"] - 1]) // R.TILE > 256 and int((kept[:r["num_pos"]] // R.TILE > 256).sum()) > 20
    if name == "images_300":
        assert int((npos_img == 0).sum()) * 3 >= r["B"] and int(npos_img[256:].sum()) > 0 and int(npos_img[:256].sum()) > 0
    if name == "c60":                                                   # a whole tile: stages of 192 and 64; the last tile partial
        assert r["N"] > R.TILE and r["N"] % R.TILE not in (0, 192) and R.TILE - R.stage_rows(60) == 64


@pytest.mark.parametrize("name", list(R.TIE_TAKEN))
def test_tie_cases_cut_where_they_say(name):
    """770 identical true negatives in five tiles, strictly between two neighbouring drawn scores; both tiles of scan thread 50's chunk (100,
    101) hold some, as do tiles of other threads before and behind; k cuts TIE_TAKEN ties deep and the lower indices are taken."""
    conf, conf_t = CASES[name]
    r = R.restate(conf, conf_t, RATIO, ALPHA)
    s, t = r["score"], conf_t.view(-1)
    tied = torch.tensor(R.tie_rows())
    v = s[tied[0]]
    eq = s == v
    assert r["margin"] == 0.0 and R.scan_chunk(-(-r["N"] // R.TILE)) == 2
    assert torch.equal(eq.nonzero()[:, 0], tied) and tied.numel() >= 600 and bool((t[tied] == 0).all())
    higher, lower = s[s > v].min(), s[s < v].max()
    assert float(higher) > float(v) > float(lower)
    assert int(((s < higher) & (s > lower)).sum()) == tied.numel()       # nothing else between the two neighbours
    per_tile = torch.bincount(tied // R.TILE, minlength=300)
    assert {int(i): int(per_tile[i]) for i in per_tile.nonzero()[:, 0]} == R.TIE_TILES
    assert {100, 101} <= set(R.TIE_TILES) and any(i // 2 != 50 and i < 100 for i in R.TIE_TILES) and any(i // 2 > 50 for i in R.TIE_TILES)
    krem = r["k"] - int((s > v).sum())
    assert krem == R.TIE_TAKEN[name] and 0 < krem < tied.numel()
    before = torch.cumsum(per_tile, 0) - per_tile                        # ties in the tiles before each tile
    cut = [int(i) for i in per_tile.nonzero()[:, 0] if int(before[i]) < krem < int(before[i] + per_tile[i])]
    if name == "ties_across_chunks":                                    # cut inside the second tile of a chunk, ties before it and behind it
        assert cut == [101] and cut[0] % 2 == 1 and int(before[101]) > 0 and int(per_tile[102:].sum()) > 0
    else:                                                               # exactly behind tile 100: no tile is cut, tile 101 takes nothing
        assert cut == [] and int(before[101]) == krem and int(per_tile[101]) > 0
    taken = r["neg"][tied]
    assert int(taken.sum()) == krem and bool(taken[:krem].all()) and not bool(taken[krem:].any())
    assert r["num_neg"] == r["k"]
    # the count of kept rows carried from tile 160 to tile 161 (one thread's chunk) decides weights: none of tile 160's ties is taken; tile 161's
    # kept rows rank below num_pos and carry a positive's weight, and would rank above it, with the negatives' weight, were those ties counted
    kept = r["keep"].nonzero()[:, 0]
    rank = torch.arange(kept.numel())
    in161 = kept // R.TILE == 161
    assert int(in161.sum()) >= 3 and int(per_tile[160]) > 0 and not bool(r["neg"][tied[tied // R.TILE == 160]].any())
    assert int(rank[in161].max()) < r["num_pos"] <= int(rank[in161].min()) + int(per_tile[160])
    w_neg = RATIO * r["B"] / r["num_neg"]
    assert bool((r["w"][kept[in161]] != w_neg).all()) and bool((r["w"][kept[rank >= r["num_pos"]]] == w_neg).all())


def test_no_positive_selects_nothing():
    conf, conf_t = CASES["no_pos"]
    for mode in ("reference", "aligned"):
        r = R.restate(conf, conf_t, RATIO, ALPHA, mode)
        assert r["k"] == 0 and not r["neg"].any() and float(r["loss"]) == 0.0 and float(r["grad"].abs().max()) == 0.0


def test_fewer_negatives_than_k():
    conf, conf_t = CASES["k_exceeds"]
    r = R.restate(conf, conf_t, RATIO, ALPHA)
    assert r["k"] == 36 and r["num_neg"] == 17 and torch.equal(r["neg"], conf_t.view(-1) == 0)
    ra = R.restate(conf, conf_t, RATIO, ALPHA, "aligned")
    assert torch.allclose(ra["w"][ra["neg"]], torch.full((17,), 3.0 / 17, dtype=torch.float64))


def test_zero_score_negatives_rank_with_the_positives_by_index():
    conf, conf_t = CASES["zero_score"]
    r = R.restate(conf, conf_t, RATIO, ALPHA)
    assert r["score"][3] == 0 and r["score"][590] == 0 and conf_t.view(-1)[3] == 0 and conf_t.view(-1)[590] == 0
    assert bool(r["neg"][3]) and not bool(r["neg"][590]) and r["num_neg"] == 439 and r["k"] == 480


def test_no_negative_with_positives_present_is_finite():
    conf, conf_t = CASES["num_neg0"]
    for mode in ("reference", "aligned"):
        r = R.restate(conf, conf_t, RATIO, ALPHA, mode)
        assert r["num_neg"] == 0 and r["num_pos"] == 30 and bool(torch.isfinite(r["loss"])) and bool(torch.isfinite(r["grad"]).all())
        assert float(r["loss"]) > 0


def test_label_outside_the_classes_is_nan_for_its_row_only():
    conf, conf_t = CASES["wide"]
    conf_t = conf_t.clone()
    row = int((conf_t.view(-1) > 0).nonzero()[0])
    conf_t.view(-1)[row] = conf.shape[-1]
    r = R.restate(conf, conf_t, RATIO, ALPHA)
    assert bool(torch.isnan(r["loss"])) and bool(torch.isnan(r["grad"][row]).all())
    others = torch.ones(r["N"], dtype=torch.bool)
    others[row] = False
    assert bool(torch.isfinite(r["grad"][others]).all())


def test_layers_fail_loudly_on_cpu_tensors():
    """No CPU fallback: the new layer functions exist and refuse CPU tensors."""
    conf, conf_t = CASES["k_exceeds"]
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.ohem_conf_loss(conf, conf_t)
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.select_neg_bboxes(conf, conf_t)
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.ohem_conf_loss(conf.clone().requires_grad_(True), conf_t, weights="aligned")
    assert issubclass(autograd.OhemConfLossFunction, torch.autograd.Function)


def test_binding_refuses_bad_targets_and_modes_before_the_device():
    conf, conf_t = CASES["k_exceeds"]
    with pytest.raises(_lib.StmError, match="int64"):
        ops.ohem_conf_loss(conf, conf_t.int())
    with pytest.raises(_lib.StmError, match="int64"):
        ops.ohem_select_neg(conf, conf_t[:, :-1])
    with pytest.raises(_lib.StmError, match="reference"):
        ops.ohem_conf_loss(conf, conf_t, weights="per-class")
    with pytest.raises(_lib.StmError, match="negpos_ratio"):
        ops.ohem_conf_loss(conf, conf_t, negpos_ratio=0)


def test_entry_points_refuse_shapes_before_any_launch():
    """STM_EINVAL / STM_EUNSUPPORTED from the shapes alone (NULL pointers: nothing is launched, no GPU is needed)."""
    lib = _lib.lib()
    c_i, c_sz, c_d = ctypes.c_int, ctypes.c_size_t, ctypes.c_double

    def loss(B, P, C, ratio=3, mode=0):
        return lib.stm_ohem_conf_loss_f32(None, None, None, None, None, c_i(B), c_i(P), c_i(C), c_i(ratio), c_d(1.0), c_i(mode), None, c_sz(0), None)

    assert loss(2, 300, 1) == -5 and b"C=1" in lib.stm_last_error_string()
    assert loss(2, 300, 129) == -5
    assert loss(4, (1 << 20) + 1, 41) == -5 and b"rows" in lib.stm_last_error_string()
    assert loss(0, 300, 41) == -1 and loss(2, 0, 41) == -1 and loss(2, 300, 41, ratio=0) == -1
    assert loss(2, 300, 41) == -2                                      # the shapes pass; the pointers are NULL
    assert lib.stm_ohem_select_neg_f32(None, None, None, c_i(2), c_i(300), c_i(200), c_i(3), None, c_sz(0), None) == -5
    assert lib.stm_ohem_conf_loss_backward_f32(None, None, None, None, None, None, c_i(2), c_i(300), c_i(1), c_i(3), c_d(1.0), None) == -5
    assert lib.stm_ohem_conf_workspace_bytes(c_i(2), c_i(300), c_i(41)) >= 4 * 4 * 600
