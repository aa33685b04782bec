"""The positive-prior loss kernels (csrc/pos_loss.hip) behind layers.box_center_loss / layers.track_loss on the MI355X, held to the fp64
restatements of the conventions (tests/pos_loss_restate.py): every loss and every gradient element within the derived bounds (forward error
times eps = 2^-24, conditioned by 1 / union and 1 / c2 for DIoU, by 1 / max(s, 1e-10) resp. 1 / max(1 - s, 1e-10) and D for the track loss; the
margin over them is the one that holds the reference's own fp32 result, 1).  The observed fraction of each bound is printed; the largest over the
cases is in INTEGRATION.md section 14."""
import math
import os

import numpy as np
import pytest
import torch

import pos_loss_restate as R
from conftest import ROOT
from stmask_amd import _lib, layers, ops

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(ROOT, "tests", "golden", "pos_loss_cases.npz"))
AB, AC, AT = R.scalar(Z["bboxiou_alpha"]), R.scalar(Z["center_alpha"]), R.scalar(Z["track_alpha"])
G_B, G_C, G_T = R.scalar(Z["g_b"]), R.scalar(Z["g_c"]), R.scalar(Z["g_t"])          # the incoming gradients (exact in fp32)
BOX_GOLDEN = [str(n) for n in Z["box_names"]]
TRACK_GOLDEN = [str(n) for n in Z["track_names"]]
BOX_CONSTRUCTED = R.constructed_box_cases()
TRACK_CONSTRUCTED = R.constructed_track_cases()
_box, _track = {}, {}


def box_case(name):
    if name not in _box:
        _box[name] = R.golden_box_case(Z, name) if name in BOX_GOLDEN else BOX_CONSTRUCTED[name]
    return _box[name]


def track_case(name):
    if name not in _track:
        inputs = R.golden_track_case(Z, name) if name in TRACK_GOLDEN else TRACK_CONSTRUCTED[name]
        _track[name] = (inputs, R.restate_track(*inputs, AT, G_T))
    return _track[name]


def frac(err, bound):
    """Largest err / bound; where the bound is 0 the value must be exact."""
    live = bound > 0
    assert bool((err[~live] == 0).all())
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


class no_host_sync:
    """Every host synchronisation is an error while the launches are made."""

    def __enter__(self):
        self.old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.old)


def run_box(loc, pri, gt, conf_t, cent):
    lg = loc.clone().requires_grad_(True)
    cg = cent.clone().requires_grad_(True) if cent is not None else None
    with no_host_sync():
        biou, center = layers.box_center_loss(lg, pri, gt, conf_t, cg, AB, AC)
        total = G_B * biou if center is None else G_B * biou + G_C * center
        total.backward()
    return biou, center, lg.grad, (cg.grad if cg is not None else None)


@pytest.mark.parametrize("name,with_cent", [(n, True) for n in BOX_GOLDEN + list(BOX_CONSTRUCTED)] +
                         [("p37", False), ("ragged", False), ("degenerate", False)])
def test_box_center_loss_and_gradients(name, with_cent):
    loc, pri, gt, conf_t, cent = box_case(name)
    if not with_cent:
        cent = None
    r = R.restate_box(loc, pri, gt, conf_t, cent, AB, AC, G_B, G_C)
    d = [t.cuda() if t is not None else None for t in (loc, pri, gt, conf_t, cent)]
    N, pos = r["N"], r["pos"]

    plain_b, plain_c, npos = ops.box_center_loss(*d[:4], d[4], AB, AC)
    assert npos.dtype == torch.int32 and npos.cpu().tolist() == r["npos"].tolist()
    with torch.no_grad():
        qb, qc = layers.box_center_loss(d[0].clone().requires_grad_(True), *d[1:4], d[4], AB, AC)
    assert qb.grad_fn is None and not qb.requires_grad and torch.equal(qb, plain_b)
    assert (qc is None) == (cent is None) and (qc is None or (qc.grad_fn is None and torch.equal(qc, plain_c)))

    biou, center, gl, gc = run_box(*d)
    assert biou.dim() == 0 and biou.dtype == torch.float32 and biou.grad_fn is not None
    assert torch.equal(biou.detach(), plain_b)                          # the forward through autograd is the plain launch
    biou2, center2, gl2, gc2 = run_box(*d)
    assert torch.equal(biou2.detach(), biou.detach()) and torch.equal(gl2, gl)             # bit-identical run to run
    if cent is None:
        assert center is None and plain_c is None and gc is None
    else:
        assert center.dim() == 0 and torch.equal(center.detach(), plain_c) and torch.equal(center2.detach(), center.detach())
        assert torch.equal(gc2, gc) and tuple(gc.shape) == tuple(cent.shape)

    assert tuple(gl.shape) == tuple(loc.shape)
    gl = gl.cpu().double().view(N, 4)
    assert bool(torch.isfinite(gl).all())
    fr = dict(biou=abs(float(biou) - float(r["biou"])) / float(r["biou_bound"]) if float(r["biou_bound"]) > 0 else 0.0,
              grad_loc=frac((gl - r["grad_loc"]).abs(), r["grad_loc_bound"]))
    if float(r["biou_bound"]) == 0:
        assert float(biou) == float(r["biou"])
    if cent is not None:
        gc = gc.cpu().double().view(N)
        fr["center"] = abs(float(center) - float(r["center"])) / float(r["center_bound"])
        fr["grad_cent"] = frac((gc - r["grad_cent"]).abs(), r["grad_cent_bound"])
        assert float(gc[~pos].abs().max()) == 0.0
    print(f"{name} cent={with_cent}: n={r['n']} BIoU {float(biou):.6f} (restated {float(r['biou']):.6f}), kernel / bound: " +
          ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert all(v <= 1.0 for v in fr.values()), fr
    assert float(gl[~pos].abs().max()) == 0.0                           # rows of priors that are not positive are exact zeros
    if name in BOX_GOLDEN and with_cent:                                # and the reference's own fp32 numbers, through the two bounds
        assert abs(float(biou) - R.scalar(Z[f"box_{name}__biou"])) <= 2 * float(r["biou_bound"])
        assert abs(float(center) - R.scalar(Z[f"box_{name}__center"])) <= 2 * float(r["center_bound"])
        ref = torch.from_numpy(Z[f"box_{name}__grad_loc_pos"]).double()
        assert bool(((gl[pos] - ref).abs() <= 2 * r["grad_loc_bound"][pos]).all())


def test_box_degenerate_row_is_exactly_zero():
    """The predicted box equals the ground truth: IoU 1, d2 = 0, 1 - DIoU = 0 in fp32 as in double."""
    loc, pri, gt, _, _ = box_case("degenerate")
    biou, center = layers.box_center_loss(loc.cuda(), pri.cuda(), gt.cuda(), R.targets_at(1, 37, [5]).cuda())
    assert center is None and float(biou) == 0.0


def test_box_empty_batch_and_single_gradients():
    """No positive at all: exact zeros everywhere.  A gradient asked for one input alone is the one of the joint backward, bit for bit."""
    loc, pri, gt, conf_t, cent = (t.cuda() for t in box_case("ragged"))
    lg, cg = loc.clone().requires_grad_(True), cent.clone().requires_grad_(True)
    biou, center = layers.box_center_loss(lg, pri, gt, torch.zeros_like(conf_t), cg, AB, AC)
    (biou + center).backward()
    assert float(biou) == 0.0 and float(center) == 0.0 and float(lg.grad.abs().max()) == 0.0 and float(cg.grad.abs().max()) == 0.0
    _, _, gl, gc = run_box(loc, pri, gt, conf_t, cent)
    cg = cent.clone().requires_grad_(True)
    biou, center = layers.box_center_loss(loc, pri, gt, conf_t, cg, AB, AC)
    (G_B * biou + G_C * center).backward()
    assert torch.equal(cg.grad, gc)
    lg = loc.clone().requires_grad_(True)
    biou, center = layers.box_center_loss(lg, pri, gt, conf_t, cent, AB, AC)
    (G_B * biou + G_C * center).backward()
    assert torch.equal(lg.grad, gl)
    # center alone still reaches loc_data (the target is not detached)
    lg = loc.clone().requires_grad_(True)
    layers.box_center_loss(lg, pri, gt, conf_t, cent, AB, AC)[1].backward()
    assert float(lg.grad.abs().max()) > 0.0


def test_box_inputs_of_other_layouts():
    """centerness as [B,P]; priors expanded per image; a view that is not 16-byte aligned; fp16 inputs -- the same kernels, the same bits."""
    loc, pri, gt, conf_t, cent = (t.cuda() for t in box_case("p37"))
    base = ops.box_center_loss(loc, pri, gt, conf_t, cent, AB, AC)
    again = layers.box_center_loss(loc, pri[None].expand(1, 37, 4), gt, conf_t, cent.view(1, 37), AB, AC)
    assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
    buf = torch.empty(loc.numel() + 1, device="cuda")
    shifted = buf[1:].view_as(loc)
    shifted.copy_(loc)
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(layers.box_center_loss(shifted, pri, gt, conf_t, cent, AB, AC)[0], base[0])
    half = layers.box_center_loss(loc.half(), pri, gt, conf_t, cent.half(), AB, AC)
    want = ops.box_center_loss(loc.half().float(), pri, gt, conf_t, cent.half().float(), AB, AC)
    assert torch.equal(half[0], want[0]) and torch.equal(half[1], want[1])


def run_track(x, conf_t, ids, alpha=AT):
    xg = x.clone().requires_grad_(True)
    with no_host_sync():
        loss = layers.track_loss(xg, conf_t, ids, alpha)
        (G_T * loss).backward()
    return loss, xg.grad


@pytest.mark.parametrize("name", TRACK_GOLDEN + [n for n in TRACK_CONSTRUCTED if n != "clamp"])
def test_track_loss_and_gradient(name):
    (x, conf_t, ids), r = track_case(name)
    d = (x.cuda(), conf_t.cuda(), ids.cuda())
    N, D, pos = r["N"], r["D"], r["pos"]

    plain = ops.track_loss(*d, AT)
    with torch.no_grad():
        quiet = layers.track_loss(d[0].clone().requires_grad_(True), d[1], d[2], AT)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)
    loss, grad = run_track(*d)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None
    assert torch.equal(loss.detach(), plain)                            # the forward through autograd is the plain launch
    loss2, grad2 = run_track(*d)
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(grad2, grad)         # bit-identical run to run

    assert tuple(grad.shape) == tuple(x.shape)
    grad = grad.cpu().double().view(N, D)
    assert bool(torch.isfinite(grad).all()) and math.isfinite(float(loss))
    err_loss = abs(float(loss) - float(r["loss"]))
    frac_loss = err_loss / float(r["loss_bound"]) if float(r["loss_bound"]) > 0 else 0.0
    frac_grad = frac((grad - r["grad"]).abs(), r["grad_bound"])
    print(f"{name}: n={r['n']} D={D} T {float(loss):.6f} (restated {float(r['loss']):.6f}), kernel / bound: loss {frac_loss:.3f}, "
          f"gradient {frac_grad:.3f}")
    assert err_loss <= float(r["loss_bound"]) and frac_grad <= 1.0
    if bool((~pos).any()):
        assert float(grad[~pos].abs().max()) == 0.0                     # rows of priors that are not positive are exact zeros
    if r["n"] < 2:                                                      # the deviation from the reference's NaN
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    if name in TRACK_GOLDEN:                                            # and the reference's own fp32 numbers, through the two bounds
        assert abs(float(loss) - R.scalar(Z[f"track_{name}__loss"])) <= 2 * float(r["loss_bound"])
        ref = torch.from_numpy(Z[f"track_{name}__grad_pos"]).double()
        assert bool(((grad[pos] - ref).abs() <= 2 * r["grad_bound"][pos]).all())


def test_track_clamp_case():
    """Rows e1, -e1, e1, e2 with ids 1, 1, 2, 3 and track_alpha = 5: two pairs sit exactly on the clamp, contribute -log(1e-10) each and pass
    exactly zero gradient; the reference's fp32 chain gives 40.10928."""
    x, conf_t, ids = TRACK_CONSTRUCTED["clamp"]
    r = R.restate_track(x, conf_t, ids, 5.0, G_T)
    loss, grad = run_track(x.cuda(), conf_t.cuda(), ids.cuda(), 5.0)
    grad = grad.cpu().double().view(4, 4)
    print(f"clamp: T {float(loss):.6f} (restated {float(r['loss']):.6f}, the reference {R.scalar(Z['clamp_loss_alpha5']):.6f})")
    assert abs(float(loss) - float(r["loss"])) <= float(r["loss_bound"]) and abs(float(loss) - 40.10928) < 1e-4
    assert frac((grad - r["grad"]).abs(), r["grad_bound"]) <= 1.0
    c = G_T * 5.0 / 6
    assert grad[0].tolist() == [0.0, float(np.float32(c)), 0.0, 0.0]    # pairs (0,1) and (0,2) are cut: only (0,3) reaches row 0
    assert float(grad[3, 2]) == 0.0 and float(grad[3, 3]) == 0.0


def test_track_ids_are_data():
    """Negative, zero and huge ids give the same bits as small ones with the same equalities."""
    (x, conf_t, ids), _ = track_case("cross_image")
    relabel = {-7: 1, 0: 2, 1 << 40: 3}
    ids2 = ids.clone().apply_(lambda v: relabel[v])
    a, ga = run_track(x.cuda(), conf_t.cuda(), ids.cuda())
    b, gb = run_track(x.cuda(), conf_t.cuda(), ids2.cuda())
    assert torch.equal(a.detach(), b.detach()) and torch.equal(ga, gb)
    torch.cuda.synchronize()


def test_double_backward_raises():
    loc, pri, gt, conf_t, cent = (t.cuda() for t in box_case("p37"))
    lg = loc.clone().requires_grad_(True)
    biou, center = layers.box_center_loss(lg, pri, gt, conf_t, cent, AB, AC)
    (g,) = torch.autograd.grad(biou + center, lg, create_graph=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        g.sum().backward()
    (x, conf_t, ids), _ = track_case("n2")
    xg = x.cuda().requires_grad_(True)
    (g,) = torch.autograd.grad(layers.track_loss(xg, conf_t.cuda(), ids.cuda(), AT), xg, create_graph=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        g.sum().backward()


def test_shapes_are_refused_before_any_launch():
    t = torch.zeros(2, 300, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.StmError, match="D=513"):
        layers.track_loss(torch.zeros(2, 300, 513, device="cuda"), t, t)
    with pytest.raises(_lib.StmError, match="int64"):
        layers.track_loss(torch.zeros(2, 300, 8, device="cuda"), t.int(), t)
    with pytest.raises(_lib.StmError, match="priors"):
        layers.box_center_loss(torch.zeros(2, 300, 4, device="cuda"), torch.zeros(299, 4, device="cuda"), torch.zeros(2, 300, 4, device="cuda"), t)
    big = torch.zeros(1, (1 << 22) + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.StmError, match="rows"):
        ops.track_loss(torch.zeros(1, (1 << 22) + 1, 1, device="cuda"), big, big)
