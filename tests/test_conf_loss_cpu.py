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
