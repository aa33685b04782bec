"""The batched mask term and the criterion module without a GPU: tests/mbox_loss_restate.py (the fp64 restatement the GPU tests hold the
kernels to) is held to the REFERENCE's own fp32 run (tests/golden/mbox_loss_cases.npz, written by tests/golden/gen_mbox_loss_golden.py from
MultiBoxLoss.lincomb_mask_loss and the whole MultiBoxLoss.forward) within the derived bounds; the module has the reference's constructor and
forward signature; everything the new entry points refuse is refused from the shapes, before any device call."""
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import conf_loss_restate as CR
import layer_grad_restate as LR
import mask_loss_restate as ML
import mbox_loss_restate as R
import oracle
import pos_loss_restate as PR
import t2s_loss_restate as T2S
from stmask_amd import layers
from stmask_amd._lib import StmError

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mbox_loss_cases.npz"))
NAMES = list(R.GOLDEN)


def _t(name, key):
    return torch.from_numpy(np.asarray(GOLD[f"{name}__{key}"]))


@functools.lru_cache(maxsize=None)
def golden(name):
    """(case, fp64 composition of g * M with g = 1 / B): drawn once, shared, never modified."""
    case = R.draw_case(R.GOLDEN[name], int(R.scalar(GOLD[f"{name}__seed"])))
    B = case["conf_t"].shape[0]
    comp = R.compose(case["loc"], case["mask_coeff"], case["proto"], case["priors"], case["conf_t"], case["idx_t"], sum(case["gt_masks"], []),
                     oracle.decode, R.MASK_ALPHA, 1.0 / B)
    return case, comp


def test_fixture_lists_the_cases_and_the_reference_stayed_inside_every_bound():
    assert list(GOLD["names"]) == NAMES and int(R.scalar(GOLD["net_seed"])) == R.NET_SEED
    assert all(R.scalar(GOLD[k]) == v for k, v in R.ALPHAS.items())
    for name in NAMES:
        devs = {k.split("__")[1]: R.scalar(GOLD[k]) for k in GOLD.files if k.startswith(f"{name}__dev_")}
        assert len(devs) >= 14 and all(0.0 <= v <= 1.0 for v in devs.values()), (name, devs)
        assert R.scalar(GOLD[f"{name}__min_edge"]) >= R.EDGE
    B, P, M, h, w, H, W = (int(v) for v in GOLD["blocks__shape"])
    assert (B, P, M, h, w, H, W) == (4, 700, 32, 24, 40, 96, 160) and tuple(int(v) for v in GOLD["tiny__shape"][:3]) == (2, 300, 8)
    assert int((_t("blocks", "conf_t").view(B, P) > 0).sum(1).max()) >= 17                  # the 16-row chunk is crossed


@pytest.mark.parametrize("name", NAMES)
def test_targets_and_crop_boxes_are_the_reference_s(name):
    case, comp = golden(name)
    for k in ("conf_t", "idx_t", "ids_t"):
        assert torch.equal(_t(name, k).long(), case[k].reshape(-1)), k                       # match_restate assigned what the reference assigned
    assert comp["n"] == int(R.scalar(GOLD[f"{name}__n"])) and comp["pred_ok"] and comp["min_edge"] >= R.EDGE
    assert torch.equal(_t(name, "ref_box"), comp["box"])                                     # :559-563, bit for bit


@pytest.mark.parametrize("name", NAMES)
def test_restatement_holds_the_reference_s_mask_term(name):
    case, comp = golden(name)
    B = case["conf_t"].shape[0]
    H, W = R.GOLDEN[name]["HW"]
    M_ref, bce_ref = _t(name, "M_unbound").double(), _t(name, "ref_bce")
    red = R.restate_reduce(bce_ref, comp["box"], comp["w"], comp["n_b"][comp["img"]], H, W, R.MASK_ALPHA)
    f_red = float((M_ref - red["M"]).abs() / red["M_bound"])                                 # the reduction, given the reference's own rows
    f_bce = ML.worst_ratio(bce_ref, comp["bce"], comp["bce_mag"])
    f_in = float((M_ref - comp["M"]).abs() / comp["M_bound"])                                # ... and from the inputs
    M_fwd = _t(name, "loss_M").double()
    f_fwd = float((M_fwd - comp["M"] / B).abs() / (comp["M_bound"] / B + R.EPS * comp["M"].abs() / B))
    print(f"\n{name}: M {float(M_ref):.6f} (restated {float(comp['M']):.6f}): reduction {f_red:.3f}, bce rows {f_bce:.3f}, from the inputs {f_in:.3f}, "
          f"after / B {f_fwd:.3f} of the bounds")
    assert max(f_red, f_bce, f_in, f_fwd) <= 1.0
    assert abs(f_red - R.scalar(GOLD[f"{name}__dev_M"])) < 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_restatement_holds_the_reference_s_gradients(name):
    case, comp = golden(name)
    B, P = case["conf_t"].shape
    Md = R.GOLDEN[name]["M"]
    rows = comp["rows"]
    gc = torch.zeros(B * P, Md)
    gc[rows] = _t(name, "grad_mask_coeff_pos")
    rc = LR.worst_ratio(gc.view(B, P, Md), comp["grad_coeff"], comp["grad_coeff_mag"])
    rp = LR.worst_ratio(_t(name, "grad_proto"), comp["grad_proto"], comp["grad_proto_mag"])
    print(f"\n{name}: reference's grad mask_coeff {rc:.3f}, grad proto {rp:.3f} of 1e-5 * sum|terms| + 1e-7")
    assert rc <= 1.0 and rp <= 1.0
    assert bool(comp["grad_coeff"].abs().sum() > 0) and bool(comp["grad_proto"].abs().sum() > 0)
    # a wrong weight (1 / n instead of 1 / n_b) or a missing 1.2 would show: both move M by far more than the bound
    n_b = comp["n_b"][comp["img"]].double()
    wrong = R.restate_reduce(comp["bce"], comp["box"], torch.full_like(comp["w"], 1.0 / comp["n"]), n_b, *R.GOLDEN[name]["HW"], R.MASK_ALPHA)
    assert float((wrong["M"] - comp["M"]).abs() / comp["M_bound"]) > 100.0


@pytest.mark.parametrize("name", NAMES)
def test_the_other_terms_of_the_golden_forward_keep_their_own_bounds(name):
    case, _ = golden(name)
    B = case["conf_t"].shape[0]
    inv, e = 1.0 / B, R.EPS
    bx = PR.restate_box(case["loc"], case["priors"], case["gt_boxes_t"], case["conf_t"], case["centerness"], R.ALPHAS["bboxiou_alpha"],
                        R.ALPHAS["center_alpha"], inv, inv)
    cf = CR.restate(case["conf"], case["conf_t"], R.RATIO, R.ALPHAS["conf_alpha"], "reference", inv)
    tr = PR.restate_track(case["track"], case["conf_t"], case["ids_t"], R.ALPHAS["track_alpha"], 1.0)
    fr = dict(BIoU=float((_t(name, "loss_BIoU").double() - bx["biou"] * inv).abs() / (bx["biou_bound"] * inv + e * bx["biou"].abs() * inv)),
              center=float((_t(name, "loss_center").double() - bx["center"] * inv).abs() / (bx["center_bound"] * inv + e * bx["center"].abs() * inv)),
              C=float((_t(name, "loss_C").double() - cf["loss"] * inv).abs() / (cf["loss_bound"] * inv + e * cf["loss"].abs() * inv)),
              T=float((_t(name, "loss_T").double() - tr["loss"]).abs() / tr["loss_bound"]))
    print(f"\n{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()) + " of the bounds")
    assert max(fr.values()) <= 1.0
    assert torch.equal(_t(name, "conf_rows").long(), torch.nonzero(cf["keep"]).reshape(-1))


@pytest.mark.parametrize("name", NAMES)
def test_the_other_gradients_and_the_shift_losses_of_the_golden_forward(name):
    """What gen_mbox_loss_golden.py asserted when it wrote the fixture, recomputed from the stored arrays: the reference's autograd gradients of
    the sum of all terms w.r.t. loc, centerness, conf and track within the bounds of pos_loss_restate / conf_loss_restate (incoming gradient
    1 / B for the terms multibox_loss() divides, 1 for T), and B_shift, M_shift and the stand-in's parameter gradients against the fp64
    composition of t2s_loss_restate at the relative deviation the fixture stores (the yardstick of the GPU tests' end-to-end tolerance)."""
    case, comp = golden(name)
    B, P = case["conf_t"].shape
    inv = 1.0 / B
    rows = comp["rows"]
    bx = PR.restate_box(case["loc"], case["priors"], case["gt_boxes_t"], case["conf_t"], case["centerness"], R.ALPHAS["bboxiou_alpha"],
                        R.ALPHAS["center_alpha"], inv, inv)
    cf = CR.restate(case["conf"], case["conf_t"], R.RATIO, R.ALPHAS["conf_alpha"], "reference", inv)
    tr = PR.restate_track(case["track"], case["conf_t"], case["ids_t"], R.ALPHAS["track_alpha"], 1.0)
    pos = bx["pos"]
    assert torch.equal(torch.nonzero(pos).reshape(-1), rows) and torch.equal(torch.nonzero(tr["pos"]).reshape(-1), rows)

    def dense(key, width):                                                               # the stored rows back in place; zeros elsewhere
        out = torch.zeros(B * P, width, dtype=torch.float64)
        out[rows] = _t(name, key).double().reshape(-1, width)
        return out

    gl, gcn, gtr = dense("grad_loc_pos", 4), dense("grad_centerness_pos", 1)[:, 0], dense("grad_track_pos", R.EMBED)
    kept = _t(name, "conf_rows").long()
    gconf = _t(name, "grad_conf_rows").double()
    fr = dict(loc=float(((gl - bx["grad_loc"]).abs()[pos] / bx["grad_loc_bound"][pos]).max()),
              centerness=float(((gcn - bx["grad_cent"]).abs()[pos] / bx["grad_cent_bound"][pos]).max()),
              conf=float(((gconf - cf["grad"][kept]).abs().max(1).values / cf["grad_bound"][kept]).max()),
              track=float(((gtr - tr["grad"]).abs()[tr["pos"]] / tr["grad_bound"][tr["pos"]]).max()))
    print(f"\n{name}: reference's gradients " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()) + " of the bounds")
    assert max(fr.values()) <= 1.0
    for k, want in (("loc", "dev_grad_loc"), ("centerness", "dev_grad_cent"), ("conf", "dev_grad_conf"), ("track", "dev_grad_track")):
        assert abs(fr[k] - R.scalar(GOLD[f"{name}__{want}"])) < 1e-6, k                   # the figures the fixture stores are these
    # the shift losses and the stand-in's parameter gradients
    t2s = T2S.compose(R.t2s_case(case), R.stand_in_net(R.GOLDEN[name]["M"], double=True).TemporalNet, oracle.decode, R.ALPHAS["boxshift_alpha"],
                      R.ALPHAS["maskshift_alpha"])
    assert t2s["n"] > 0 and t2s["min_kink"] > T2S.KINK
    e_loss = max(float((_t(name, "loss_B_shift").double() - t2s["B"]).abs() / t2s["B"].abs()),
                 float((_t(name, "loss_M_shift").double() - t2s["M"]).abs() / t2s["M"].abs()))
    e_grad = max(float((_t(name, "grad_net_" + k.replace(".", "_")).double() - g).abs().max() / g.abs().max()) for k, g in t2s["grads"].items())
    print(f"{name}: B_shift / M_shift {e_loss:.2e}, the stand-in's parameter gradients {e_grad:.2e} relative to the fp64 composition")
    assert sorted("grad_net_" + k.replace(".", "_") for k in t2s["grads"]) == sorted(k.split("__")[1] for k in GOLD.files
                                                                                       if k.startswith(f"{name}__grad_net_"))
    # the stored deviation IS this recomputed one (the CPU's fp32 is deterministic), and it lies inside the end-to-end tolerance
    # tests/test_gpu_t2s_loss.py already uses: 8 x the reference's fp32 deviation stored in the temporal-fusion fixture
    assert abs(e_loss - R.scalar(GOLD[f"{name}__e2e_loss"])) <= 1e-9 and abs(e_grad - R.scalar(GOLD[f"{name}__e2e_grad"])) <= 1e-9
    t2s_gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t2s_loss_cases.npz"))
    with_rows = ["p37", "p256_b2", "p257_b3"]
    assert e_loss <= 8 * max(R.scalar(t2s_gold[f"{n}__e2e_loss"]) for n in with_rows)
    assert e_grad <= 8 * max(R.scalar(t2s_gold[f"{n}__e2e_grad"]) for n in with_rows)


@pytest.mark.parametrize("name", list(R.CONSTRUCTED))
def test_constructed_case_lies_above_both_scan_lines_and_meets_the_input_conditions(name):
    """The module-level case that no run of the reference backs: more than 256 OHEM tiles of 256 flattened rows, more than 256 list tiles with an
    odd number per image (images begin inside a scan thread's chunk of 2), and the input conditions the generator of the golden cases demands
    of a seed -- the bounds the GPU tests apply are derived under them."""
    spec = R.CONSTRUCTED[name]
    case = R.draw_case(spec, spec["seed"])
    B, P = case["conf_t"].shape
    assert (B, P, spec["M"], spec["proto"], spec["HW"], spec["G"]) == (6, 11520, 8, (12, 20), (48, 80), (2, 3, 1, 2, 2, 1)) and len(spec["scales"]) == 3
    ohem_tiles, tpi = -(-B * P // CR.TILE), -(-P // PR.TILE)
    assert (ohem_tiles, tpi, B * tpi) == (270, 45, 270) and CR.scan_chunk(ohem_tiles) == 2 and -(-B * tpi // PR.TILE) == 2 and tpi % 2 == 1
    n_b = (case["conf_t"] > 0).sum(1)
    assert int(n_b.min()) >= 1 and case["match_margin"] > R.INPUT_CONDITIONS["match_margin"]
    tile = torch.unique(torch.nonzero(case["conf_t"].reshape(-1) > 0).reshape(-1) // CR.TILE)
    assert int(tile[-1]) >= (B - 1) * P // CR.TILE and int((tile % 2 == 1).sum()) > 0 and int((tile % 2 == 0).sum()) > 0    # ... into the last image
    assert CR.margin(case["conf"], case["conf_t"], R.RATIO) > R.INPUT_CONDITIONS["ohem_margin"]
    comp = R.compose(case["loc"], case["mask_coeff"], case["proto"], case["priors"], case["conf_t"], case["idx_t"], sum(case["gt_masks"], []),
                     oracle.decode, R.MASK_ALPHA, 1.0 / B)
    assert comp["n"] == int(n_b.sum()) and comp["pred_ok"] and comp["min_edge"] >= R.EDGE
    tr = PR.restate_track(case["track"], case["conf_t"], case["ids_t"], R.ALPHAS["track_alpha"], 1.0)
    assert tr["min_v"] > R.INPUT_CONDITIONS["track_min_v"]
    t2s = T2S.compose(R.t2s_case(case), R.stand_in_net(spec["M"], double=True).TemporalNet, oracle.decode, R.ALPHAS["boxshift_alpha"],
                      R.ALPHAS["maskshift_alpha"], want_grads=False)
    assert t2s["n"] > 0 and t2s["min_kink"] > T2S.KINK


def test_module_has_the_reference_s_constructor_and_forward():
    assert layers.modules.MultiBoxLoss is layers.MultiBoxLoss and issubclass(layers.MultiBoxLoss, torch.nn.Module)
    init = list(inspect.signature(layers.MultiBoxLoss.__init__).parameters)
    assert init[:5] == ["self", "num_classes", "pos_threshold", "neg_threshold", "negpos_ratio"]
    assert list(inspect.signature(layers.MultiBoxLoss.forward).parameters) == ["self", "net", "predictions", "gt_bboxes", "gt_labels", "gt_masks",
                                                                               "gt_ids"]
    crit = layers.MultiBoxLoss(41, 0.5, 0.4, 3)
    assert {k: getattr(crit, k) for k in R.ALPHAS} == R.ALPHAS and crit.temporal_fusion and crit.max_pos is None
    assert layers.MultiBoxLoss(41, 0.5, 0.4, 3, max_pos=64, temporal_fusion=False, use_boxiou_loss=True).max_pos == 64
    for flag in (dict(use_boxiou_loss=False), dict(use_focal_loss=True), dict(use_sigmoid_focal_loss=True), dict(use_class_balanced_conf=True),
                 dict(use_semantic_segmentation_loss=True), dict(use_maskiou=True), dict(mask_proto_loss="l1")):
        with pytest.raises(NotImplementedError):
            layers.MultiBoxLoss(41, 0.5, 0.4, 3, **flag)
    with pytest.raises(TypeError):
        layers.MultiBoxLoss(41, 0.5, 0.4, 3, no_such_flag=1)
    with pytest.raises(ValueError):
        layers.MultiBoxLoss(41, 0.5, 0.4, 3, max_pos=0)
    params = inspect.signature(layers.lincomb_mask_loss).parameters
    assert list(params)[:10] == ["loc_data", "mask_data", "proto_data", "priors", "conf_t", "idx_t", "gt_masks", "mask_alpha", "max_pos", "want_status"]
    assert params["mask_alpha"].default == 1.0 and params["max_pos"].default is None and params["want_status"].default is False


def _cpu_args(B=2, P=300, M=8, sizes=((48, 80), (48, 80))):
    """CPU tensors: a call that got as far as the device would fail with "need tensors on the MI355X" instead of the refusal under test."""
    z = lambda *s: torch.zeros(1).expand(*s)                                                # noqa: E731  (no memory behind the big shapes)
    zl = lambda *s: torch.zeros(1, dtype=torch.int64).expand(*s)                            # noqa: E731
    masks = [torch.zeros(1, *sizes[b % len(sizes)], dtype=torch.uint8) for b in range(B)]
    return [z(B, P, 4), z(B, P, M), z(B, 12, 20, M), z(P, 4), zl(B, P), zl(B, P), masks]


def test_refusals_come_from_the_shapes_before_any_device_call():
    with pytest.raises(StmError, match="mask_dim 16"):
        layers.lincomb_mask_loss(*_cpu_args(M=16))
    with pytest.raises(StmError, match="B\\*P"):
        layers.lincomb_mask_loss(*_cpu_args(B=2049, P=2048))
    with pytest.raises(StmError, match="65536 rows"):
        layers.lincomb_mask_loss(*_cpu_args(), max_pos=65536)
    with pytest.raises(ValueError, match="max_pos"):
        layers.lincomb_mask_loss(*_cpu_args(), max_pos=0)
    with pytest.raises(ValueError, match="one size"):
        layers.lincomb_mask_loss(*_cpu_args(sizes=((48, 80), (48, 81))))
    with pytest.raises(ValueError):
        layers.lincomb_mask_loss(*_cpu_args()[:6], [torch.zeros(1, 48, 80, dtype=torch.uint8)])       # one mask tensor for two images
    with pytest.raises(ValueError):
        layers.lincomb_mask_loss(torch.zeros(0, 300, 4), *_cpu_args()[1:])                             # B below 1 shows as a shape mismatch
    for flag in (dict(mask_proto_crop=False), dict(mask_proto_crop_with_pred_box=False), dict(mask_activation="relu"),
                 dict(interpolation_mode="nearest"), dict(use_maskiou=True), dict(use_maskiou_loss=True),
                 dict(mask_proto_coeff_diversity_loss=True), dict(use_mask_scoring=True)):
        with pytest.raises(NotImplementedError):
            layers.lincomb_mask_loss(*_cpu_args(), **flag)
    with pytest.raises(StmError, match="MI355X"):                                                      # a legal call on CPU tensors does reach the device check
        layers.lincomb_mask_loss(*_cpu_args())
