"""CPU checks of the positive-prior loss terms (no kernel runs): the fp64 restatements of the conventions (tests/pos_loss_restate.py) against the
reference's own fp32 outputs (tests/golden/pos_loss_cases.npz), the findings about the reference that are part of the contract, hand-worked and
constructed cases, and the API surface.  tests/test_gpu_pos_loss.py holds the kernels to the same restatements."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import pos_loss_restate as R
from conftest import ROOT
from stmask_amd import _lib, autograd, layers, ops

Z = np.load(os.path.join(ROOT, "tests", "golden", "pos_loss_cases.npz"))
AB, AC, AT = R.scalar(Z["bboxiou_alpha"]), R.scalar(Z["center_alpha"]), R.scalar(Z["track_alpha"])
G_B, G_C, G_T = R.scalar(Z["g_b"]), R.scalar(Z["g_c"]), R.scalar(Z["g_t"])
BOX = [str(n) for n in Z["box_names"]]
TRACK = [str(n) for n in Z["track_names"]]


def frac(err, bound):
    live = bound > 0
    assert bool((err[~live] == 0).all())
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def box_deviation(name, **kw):
    loc, pri, gt, conf_t, cent = R.golden_box_case(Z, name)
    r = R.restate_box(loc, pri, gt, conf_t, cent, AB, AC, G_B, G_C, **kw)
    pos = r["pos"]
    gl = torch.from_numpy(Z[f"box_{name}__grad_loc_pos"]).double()
    gc = torch.from_numpy(Z[f"box_{name}__grad_cent_pos"]).double()
    return dict(biou=abs(R.scalar(Z[f"box_{name}__biou"]) - float(r["biou"])) / float(r["biou_bound"]),
                center=abs(R.scalar(Z[f"box_{name}__center"]) - float(r["center"])) / float(r["center_bound"]),
                grad_loc=frac((gl - r["grad_loc"][pos]).abs(), r["grad_loc_bound"][pos]),
                grad_cent=frac((gc - r["grad_cent"][pos]).abs(), r["grad_cent_bound"][pos]))


@pytest.mark.parametrize("name", BOX)
def test_box_restatement_reproduces_the_reference(name):
    """The reference's fp32 BIoU, center and both gradients within the derived bounds; the observed fraction is the one the generator stored."""
    dev = box_deviation(name)
    print(f"{name}: reference fp32 / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in dev.items()))
    assert all(v <= 1.0 for v in dev.values()), dev
    for k, key in (("biou", "dev_biou"), ("center", "dev_center"), ("grad_loc", "dev_grad_loc"), ("grad_cent", "dev_grad_cent")):
        assert abs(dev[k] - R.scalar(Z[f"box_{name}__{key}"])) < 1e-6


@pytest.mark.parametrize("name", BOX)
def test_center_target_is_not_detached_in_the_reference(name):
    """The finding: with smooth-L1's target detached the losses and grad_centerness still agree, grad_loc does NOT -- losses['center'] sends
    gradient to loc_data."""
    dev = box_deviation(name, detach_target=True)
    assert dev["biou"] <= 1.0 and dev["center"] <= 1.0 and dev["grad_cent"] <= 1.0
    assert dev["grad_loc"] > 100.0, dev


@pytest.mark.parametrize("name", TRACK)
def test_track_restatement_reproduces_the_reference(name):
    x, conf_t, ids = R.golden_track_case(Z, name)
    r = R.restate_track(x, conf_t, ids, AT, G_T)
    assert r["min_v"] > 2e-3 and abs(r["min_v"] - R.scalar(Z[f"track_{name}__min_v"])) < 1e-9      # no pair near a clamp: conditioning < 500
    pos = r["pos"]
    dev_loss = abs(R.scalar(Z[f"track_{name}__loss"]) - float(r["loss"])) / float(r["loss_bound"])
    dev_grad = frac((torch.from_numpy(Z[f"track_{name}__grad_pos"]).double() - r["grad"][pos]).abs(), r["grad_bound"][pos])
    print(f"{name}: n={r['n']} reference fp32 / bound: loss {dev_loss:.3f}, gradient {dev_grad:.3f}")
    assert dev_loss <= 1.0 and dev_grad <= 1.0
    assert abs(dev_loss - R.scalar(Z[f"track_{name}__dev_loss"])) < 1e-6 and abs(dev_grad - R.scalar(Z[f"track_{name}__dev_grad"])) < 1e-6


def reference_style_box(loc, pri, gt, conf_t, cent, dtype=torch.float64):
    """The reference's chain (:164-172, :450-455, :227-245) in torch ops, for autograd."""
    B, P = conf_t.shape
    pos = conf_t > 0
    w = R._weights(conf_t)[1].to(dtype)
    l = loc.to(dtype).requires_grad_(True)
    c = cent.to(dtype).requires_grad_(True)
    p = (pri if pri.dim() == 3 else pri[None].expand(B, P, 4)).to(dtype)[pos]
    lp = l[pos]
    v0, v1 = float(np.float32(0.1)), float(np.float32(0.2))
    boxes = torch.cat((p[:, :2] + lp[:, :2] * v0 * p[:, 2:], p[:, 2:] * torch.exp(lp[:, 2:] * v1)), 1)
    x1y1 = boxes[:, :2] - boxes[:, 2:] / 2
    pred = torch.cat((x1y1, boxes[:, 2:] + x1y1), 1)
    g = gt.to(dtype)[pos]
    inter = (torch.min(g[:, 2:], pred[:, 2:]) - torch.max(g[:, :2], pred[:, :2])).clamp(min=0).prod(1)
    iou = inter / ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) + (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1]) - inter)
    xl = torch.cat([pred[:, ::2], g[:, ::2]], 1)
    yl = torch.cat([pred[:, 1::2], g[:, 1::2]], 1)
    c2 = ((xl.max(1)[0] - xl.min(1)[0]) ** 2 + (yl.max(1)[0] - yl.min(1)[0]) ** 2).clamp(min=1e-10)
    d2 = ((pred[:, :2] / 2 + pred[:, 2:] / 2 - (g[:, :2] / 2 + g[:, 2:] / 2)) ** 2).sum(1)
    diou = iou - d2 / c2
    biou = (w * (1 - diou)).sum() * AB
    center = AC * (w * torch.nn.functional.smooth_l1_loss(c.view(-1)[pos.view(-1)], diou, reduction="none")).sum()
    return l, c, biou, center


def test_box_restatement_gradient_is_autograd_of_the_reference_chain():
    loc, pri, gt, conf_t, cent = R.golden_box_case(Z, "ragged")
    r = R.restate_box(loc, pri, gt, conf_t, cent, AB, AC, G_B, G_C)
    l, c, biou, center = reference_style_box(loc, pri, gt, conf_t, cent)
    assert abs(float(biou.detach()) - float(r["biou"])) < 1e-12 and abs(float(center.detach()) - float(r["center"])) < 1e-12
    (G_B * biou + G_C * center).backward()
    assert torch.allclose(l.grad.view(-1, 4), r["grad_loc"], atol=1e-12, rtol=1e-10)
    assert torch.allclose(c.grad.view(-1), r["grad_cent"], atol=1e-13)


def test_enclosing_box_ties_go_to_the_first_element():
    """pred = [0.375, 0.375, 0.625, 0.625], gt = [0.375, 0.25, 0.75, 0.625]: min x is pred.x1 == gt.x1 and max y is pred.y2 == gt.y2; torch's
    max / min over cat([pred, gt]) give the tie to pred (the first), and so does the restatement.  The intersection's ties (min(x2), max(x1) of
    jaccard) go to the ground truth instead (this repository's jaccard convention; torch.min / torch.max of two tensors would split a tie in
    halves)."""
    loc, pri, gt, conf_t, cent = R.constructed_box_cases()["enclosing_ties"]
    row = 7
    pred = torch.tensor([[0.375, 0.375, 0.625, 0.625]], dtype=torch.float64).requires_grad_(True)
    g = gt[0, row].double()[None]
    xl = torch.cat([pred[:, ::2], g[:, ::2]], 1)
    yl = torch.cat([pred[:, 1::2], g[:, 1::2]], 1)
    c2 = (xl.max(1)[0] - xl.min(1)[0]) ** 2 + (yl.max(1)[0] - yl.min(1)[0]) ** 2
    c2.sum().backward()
    ex, ey = 0.75 - 0.375, 0.625 - 0.25
    assert pred.grad.tolist() == [[-2 * ex, 0.0, 0.0, 2 * ey]]                 # torch: first minimal (pred.x1), first maximal (pred.y2)
    r = R.restate_box(loc, pri, gt, conf_t, None, 1.0, 1.0, 1.0, 1.0)
    assert torch.equal(r["pred"][0], pred.detach()[0])
    _, J, q = R._diou_and_jacobian(pred.detach(), g)
    # the same boxes with the ground truth moved off the ties by 2^-20 (outwards): the enclosing box's gradient leaves pred.x1 / pred.y2, and the
    # intersection's, which the tie gave to the ground truth, arrives there instead
    g2 = g.clone()
    g2[0, 0] -= 2.0 ** -20
    g2[0, 3] += 2.0 ** -20
    _, J2, _ = R._diou_and_jacobian(pred.detach(), g2)
    gext_x, gext_y = float(q["q"] / q["c2"] * 2 * ex), float(q["q"] / q["c2"] * 2 * ey)
    gmx, gmy = float(q["gi"] * q["my"]), float(q["gi"] * q["mx"])
    assert gext_x > 0.01 and gext_y > 0.01                           # far above the 1e-4 that the comparison allows
    assert abs(float(J[0, 0] - J2[0, 0]) - (-gext_x + gmx)) < 1e-4 and abs(float(J[0, 3] - J2[0, 3]) - (gext_y - gmy)) < 1e-4


def test_degenerate_row_has_zero_terms():
    """The predicted box equals the ground truth: IoU 1, d2 = 0, 1 - DIoU = 0 exactly."""
    loc, pri, gt, conf_t, cent = R.constructed_box_cases()["degenerate"]
    r = R.restate_box(loc, pri, gt, conf_t, cent, 1.0, 1.0)
    assert torch.equal(r["pred"][0].float(), gt[0, 5]) and float(r["diou"][0]) == 1.0
    only = R.restate_box(loc, pri, gt, R.targets_at(1, 37, [5]), None, 1.0, 1.0)
    assert float(only["biou"]) == 0.0 and only["center"] is None and only["grad_cent"] is None


def test_image_without_positives_contributes_nothing():
    loc, pri, gt, conf_t, cent = R.golden_box_case(Z, "ragged")
    r = R.restate_box(loc, pri, gt, conf_t, cent, AB, AC)
    assert r["npos"].tolist() == [7, 0, 3]
    assert float(r["grad_loc"][300:600].abs().max()) == 0.0 and float(r["grad_cent"][300:600].abs().max()) == 0.0
    none = R.restate_box(loc, pri, gt, torch.zeros_like(conf_t), cent, AB, AC)
    assert float(none["biou"]) == 0.0 and float(none["center"]) == 0.0 and float(none["grad_loc"].abs().max()) == 0.0


def test_fewer_than_two_positives_deviates_from_the_reference():
    """The reference's chain divides by loss_weights.sum() == 0 and returns NaN; the restatement (and the kernel) give exactly 0."""
    cases = R.constructed_track_cases()
    for name in ("n0", "n1"):
        x, conf_t, ids = cases[name]
        pos = conf_t > 0
        xp, idp = x[pos], ids[pos]
        w = torch.ones(int(pos.sum())) / max(int(pos.sum()), 1)
        lw = (w.view(-1, 1) @ w.view(1, -1)).triu_(diagonal=1)
        cos = ((xp @ xp.t() + 1) / 2).triu_(diagonal=1)
        eq = (idp.view(-1, 1) == idp.view(1, -1)).float()
        lm = (-1 * (eq * cos.clamp(min=1e-10).log() + (1 - eq) * (1 - cos).clamp(min=1e-10).log())).triu_(diagonal=1)
        assert bool(torch.isnan((lm * lw).sum() * AT / lw.sum()))
        r = R.restate_track(x, conf_t, ids, AT)
        assert r["n"] == (0 if name == "n0" else 1) and float(r["loss"]) == 0.0 and float(r["grad"].abs().max()) == 0.0


def test_clamp_case():
    """Rows e1, -e1, e1, e2, ids 1, 1, 2, 3, equal weights, track_alpha = 5: both clamped pairs give -log(1e-10) and pass exactly zero gradient;
    the reference's fp32 chain gives 40.10928."""
    x, conf_t, ids = R.clamp_case()
    r = R.restate_track(x, conf_t, ids, 5.0, 1.0)
    expect = 5.0 * (2 * -math.log(1e-10) + 3 * math.log(2.0)) / 6
    assert abs(float(r["loss"]) - expect) < 1e-12 and abs(expect - 40.10928) < 1e-5
    assert abs(R.scalar(Z["clamp_loss_alpha5"]) - expect) < 1e-5
    # d/dx_0: pairs (0,1) and (0,2) are cut; (0,3): different ids, s = 1/2, +1 / (1 - s) * e2 / 2 = 2 * e2 / 2
    c = 5.0 / 6
    assert torch.allclose(r["grad"][0], torch.tensor([0.0, c, 0.0, 0.0], dtype=torch.float64), atol=1e-15)
    # d/dx_1 = -e1: (1,2) different ids, s = 0: 1 / (1 - 0) * e1 / 2; (1,3): e2
    assert torch.allclose(r["grad"][1], torch.tensor([c / 2, c, 0.0, 0.0], dtype=torch.float64), atol=1e-15)
    ref = torch.from_numpy(Z["clamp_grad"]).double() / R.scalar(Z["g_t"])
    assert torch.allclose(ref, r["grad"], atol=1e-6)


def test_ids_are_compared_for_equality_only():
    x, conf_t, ids = R.constructed_track_cases()["cross_image"]
    assert set(ids.unique().tolist()) == {-7, 0, 1 << 40}
    relabel = {-7: 1, 0: 2, 1 << 40: 3}
    ids2 = ids.clone().apply_(lambda v: relabel[v])
    a, b = R.restate_track(x, conf_t, ids, AT), R.restate_track(x, conf_t, ids2, AT)
    assert float(a["loss"]) == float(b["loss"]) and torch.equal(a["grad"], b["grad"])
    pos = conf_t.view(-1) > 0
    img = (torch.arange(900) // 300)[pos]
    idp = ids.view(-1)[pos]
    cross = (idp[:, None] == idp[None, :]) & (img[:, None] != img[None, :])
    assert bool(cross.any()) and sorted(img.unique().tolist()) == [0, 2]


# name -> (tiles per image, tiles, the scan's chunk, more than 256 images?)
LIST_PATHS = {"tiles_259": (37, 259, 2, False), "tiles_900": (3, 900, 4, True), "images_300": (1, 300, 2, True)}


@pytest.mark.parametrize("name", list(R.LIST_CASES))
def test_list_cases_reach_what_they_exist_for(name):
    """More than 256 tiles (the scan's carry inside a thread's chunk), images that begin inside a chunk, more than 256 images; few positives per
    image and many images without; positives in an image's first and last row and on both sides of a tile border inside a chunk and of one
    between two chunks."""
    B, P, per_image = R.list_positives(name)
    conf_t = R.list_targets(name)
    tpi = -(-P // R.TILE)
    nT = B * tpi
    chunk = -(-nT // R.TILE)
    assert (tpi, nT, chunk, B > 256) == LIST_PATHS[name] and nT > 256
    pos = conf_t > 0
    assert [row.nonzero()[:, 0].tolist() for row in pos] == per_image and bool((conf_t < 0).any())
    counts = pos.sum(1)
    assert int(counts.max()) <= 6 and int((counts == 0).sum()) * 4 >= B and int(counts.sum()) <= 500
    if B > 256:
        assert int(counts[256:].sum()) > 0 and int((counts[256:] == 0).sum()) > 0
    if name == "tiles_259":                                             # prefix[b] is read from the middle of another thread's chunk
        assert tpi % 2 == 1 and any((b * tpi) % chunk and int(counts[b]) for b in range(B))
    assert bool(pos[:, 0].any()) and bool(pos[:, P - 1].any())
    tile = (torch.arange(B)[:, None] * tpi + torch.arange(P)[None, :] // R.TILE)[pos]     # the tile of every positive, in list order
    rows = pos.reshape(-1).nonzero()[:, 0]
    prior = rows % P
    last_of_tile = (prior % R.TILE == R.TILE - 1) | (prior == P - 1)
    first_of_tile = prior % R.TILE == 0
    inside, between = 0, 0                                              # borders i | i + 1 with a positive in the last row of i and the first of i + 1
    for i in tile[last_of_tile].tolist():
        if bool((first_of_tile & (tile == i + 1)).any()):
            if (i + 1) % chunk:
                inside += 1
            else:
                between += 1
    assert inside > 0 and between > 0, (inside, between)
    x, t, ids = R.constructed_track_cases()[name]
    assert torch.equal(t, conf_t) and x.shape == (B, P, 8)
    r = R.restate_track(x, t, ids, AT, G_T)
    assert r["n"] == int(counts.sum()) >= 20 and r["min_v"] > 2e-3       # no pair near a clamp, as on the golden cases
    w = 1.0 / counts.clamp(min=1).double()
    s1, s2 = (counts * w).sum(), (counts * w * w).sum()
    assert abs(float((s1 * s1 - s2) / 2) - float(r["W"])) < 1e-9 * float(r["W"])             # W as the kernel forms it, over all B images


def test_layers_fail_loudly_on_cpu_tensors():
    """No CPU fallback: the new layer functions exist and refuse CPU tensors."""
    loc, pri, gt, conf_t, cent = R.golden_box_case(Z, "p37")
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.box_center_loss(loc, pri, gt, conf_t, cent)
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.box_center_loss(loc.clone().requires_grad_(True), pri, gt, conf_t)
    x, conf_t, ids = R.clamp_case()
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.track_loss(x, conf_t, ids)
    with pytest.raises(_lib.StmError, match="no CPU fallback"):
        layers.track_loss(x.clone().requires_grad_(True), conf_t, ids, track_alpha=5.0)
    assert issubclass(autograd.BoxCenterLossFunction, torch.autograd.Function) and issubclass(autograd.TrackLossFunction, torch.autograd.Function)


def test_bindings_refuse_bad_shapes_before_the_device():
    loc, pri, gt, conf_t, cent = R.golden_box_case(Z, "p37")
    with pytest.raises(_lib.StmError, match="int64"):
        ops.box_center_loss(loc, pri, gt, conf_t.int())
    with pytest.raises(_lib.StmError, match="priors"):
        ops.box_center_loss(loc, pri[:-1], gt, conf_t)
    with pytest.raises(_lib.StmError, match="gt_boxes_t"):
        ops.box_center_loss(loc, pri, gt[:, :-1], conf_t)
    with pytest.raises(_lib.StmError, match="centerness_data"):
        ops.box_center_loss(loc, pri, gt, conf_t, cent[:, :-1])
    x, conf_t, ids = R.clamp_case()
    with pytest.raises(_lib.StmError, match="ids_t"):
        ops.track_loss(x, conf_t, ids.int())
    with pytest.raises(_lib.StmError, match="conf_t"):
        ops.track_loss(x, conf_t[:, :-1], ids)
    with pytest.raises(_lib.StmError, match=r"\[B,P,D\]"):
        ops.track_loss(x[0], conf_t, ids)


def test_entry_points_refuse_shapes_before_any_launch():
    """STM_EINVAL / STM_EUNSUPPORTED from the shapes alone (NULL pointers: nothing is launched, no GPU is needed)."""
    lib = _lib.lib()
    c_i, c_sz, c_d = ctypes.c_int, ctypes.c_size_t, ctypes.c_double

    def box(B, P, per=0):
        return lib.stm_box_center_loss_f32(None, None, c_i(per), None, None, None, None, None, None, c_i(B), c_i(P), c_d(1.0), c_d(1.0), None,
                                           c_sz(0), None)

    def track(B, P, D):
        return lib.stm_track_loss_f32(None, None, None, None, c_i(B), c_i(P), c_i(D), c_d(1.0), None, c_sz(0), None)

    def track_bwd(B, P, D):
        return lib.stm_track_loss_backward_f32(None, None, None, None, None, c_i(B), c_i(P), c_i(D), c_d(1.0), None, c_sz(0), None)

    assert box(0, 300) == -1 and box(2, 0) == -1 and box(2, 300, per=2) == -1
    assert box(4, (1 << 20) + 1) == -5 and b"rows" in lib.stm_last_error_string()
    assert box(2, 300) == -2                                           # the shapes pass; the pointers are NULL
    assert lib.stm_box_center_loss_backward_f32(None, None, None, None, c_i(0), None, None, None, None, None, None, c_i(2), c_i(0), c_d(1.0),
                                                c_d(1.0), None) == -1
    assert track(2, 300, 0) == -5 and b"D=0" in lib.stm_last_error_string()
    assert track(2, 300, 513) == -5 and track_bwd(2, 300, 513) == -5
    assert track(0, 300, 8) == -1 and track(4, (1 << 20) + 1, 8) == -5
    assert track(2, 300, 512) == -2 and track_bwd(2, 300, 5) == -2
    assert lib.stm_box_center_workspace_bytes(c_i(2), c_i(300)) >= 4 * 20
    assert lib.stm_track_loss_workspace_bytes(c_i(2), c_i(300), c_i(128)) >= 2 * 4 * 600
