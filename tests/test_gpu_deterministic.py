"""The deterministic mode of the training backward (autograd.set_deterministic, csrc/det_backward.hip) on the MI355X: the two fixed-point scatters
held bit for bit to the numpy restatement of tests/det_restate.py and, within its derived bound, to the float64 oracle there; the gather-form
adjoint of bilinear upsampling against its float64 restatement; the modules and one whole train step under torch.use_deterministic_algorithms(True).

Collisions are what the mode is about, so the inputs make them: the deformable offsets send every tap of the 9 x 9 case into one 2 x 2
neighbourhood (729 adders an address), the RoIs are 64 copies of one box beside 8 distinct ones."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import det_restate as D
import geometry_cases as G
import t2s_loss_restate as TR
from stmask_amd import autograd, layers, ops, synthetic
from stmask_amd.config import get_cfg
from stmask_amd.dcn_v2 import DCN
from stmask_amd.layers.modules import FPN, FeatureAlign, InterpolateModule
from stmask_amd.model import STMask
from stmask_amd.optim import GuardedSGD
from stmask_amd.train import NetLoss, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADA = "STMask_plus_resnet50_ada_config"
SGD = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)


@pytest.fixture(autouse=True)
def mode_as_found():
    """Every test under MIOpen's deterministic solvers (what the bit-for-bit forward tests use); the mode and torch's flag go back to their defaults."""
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        yield
    autograd.set_deterministic(None)
    torch.use_deterministic_algorithms(False)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- deformable col2im -------------------------------------------------------------------------------------------------------------------------
def _colliding():
    """B = 2, C = 16, dg = 2, 9 x 9, 3 x 3: every tap of every output lands in rows 3-4, columns 4-5."""
    c = dict(B=2, C=16, H=9, W=9, k=(3, 3), st=(1, 1), pad=(1, 1), dl=(1, 1), dg=2, seed=71, name="colliding_9x9")
    g = torch.Generator().manual_seed(c["seed"])
    K = 9
    by, bx = G._bases(dict(c, lattice=False))
    target = torch.stack([3.0 + torch.rand(2, 2, K, 9, 9, generator=g), 4.0 + torch.rand(2, 2, K, 9, 9, generator=g)], 3)     # [B, dg, K, 2, Ho, Wo]
    off = target - torch.stack([by.expand(K, 9, 9), bx.expand(K, 9, 9)], 1)
    return c, off.reshape(2, 2 * 2 * K, 9, 9).contiguous()


def _table(pick):
    c = next(c for c in G.DEFORM_CASES if pick(c))
    return c, G.offsets(c, torch.Generator().manual_seed(c["seed"]))


COL2IM = [_colliding(), _table(lambda c: c["st"] == (2, 2)), _table(lambda c: c["st"][0] != c["st"][1])]


def col2im_inputs(case, off, mask_kind):
    """-> gcols, off, mask (None / explicit with values above 1 / logits), numpy copies alongside"""
    g = torch.Generator().manual_seed(case["seed"] + 5)
    Ho, Wo = G.out_hw(case)
    K = case["k"][0] * case["k"][1]
    gcols = torch.randn(case["B"], case["C"] * K, Ho * Wo, generator=g)
    mask = None
    if mask_kind == "explicit":
        mask = torch.randn(case["B"], case["dg"] * K, Ho, Wo, generator=g) * 3.0
    elif mask_kind == "logit":
        mask = torch.randn(case["B"], case["dg"] * K, Ho, Wo, generator=g) * 2.0
    return gcols, off, mask


def run_col2im(case, gcols, off, mask, mask_kind):
    x = torch.empty(case["B"], case["C"], case["H"], case["W"])
    geom = ops._geom(x, case["k"], case["st"], case["pad"], case["dl"], case["dg"])
    if mask_kind == "logit":
        om = torch.cat([off, mask], 1).to(DEV)
        return ops.deform_col2im(gcols.to(DEV), None, None, geom, fused_om=om)
    return ops.deform_col2im(gcols.to(DEV), off.to(DEV), None if mask is None else mask.to(DEV), geom)


def geom_kw(case):
    return {k: case[k] for k in ("B", "C", "H", "W", "k", "st", "pad", "dl", "dg")}


@pytest.mark.parametrize("mask_kind", ["none", "explicit"])
@pytest.mark.parametrize("case,off", COL2IM, ids=[c["name"] for c, _ in COL2IM])
def test_col2im_is_the_fixed_point_restatement_bit_for_bit(case, off, mask_kind):
    gcols, off, mask = col2im_inputs(case, off, mask_kind)
    autograd.set_deterministic(True)
    runs = [run_col2im(case, gcols, off, mask, mask_kind) for _ in range(5)]
    assert all(same_bits(runs[0], r) for r in runs[1:])
    dest, t32, t64 = D.col2im_terms(gcols.numpy(), off.numpy(), None if mask is None else mask.numpy(), **geom_kw(case))
    numel = runs[0].numel()
    bounds = D.col2im_bounds(case["k"], *G.out_hw(case))
    b_bits = D.ONE_BITS if mask is None else D.absmax_bits(mask.numpy())
    want, state, p = D.det_result(dest, t32, numel, D.absmax_bits(gcols.numpy()), b_bits, *bounds)
    got = runs[0].cpu().numpy().ravel()
    adders = np.bincount(dest, minlength=numel).max()
    print(f"\n{case['name']} {mask_kind}: p = {p}, up to {adders} adders an address, {int((D.bits(got) != D.bits(want)).sum())} of {numel} words differ")
    assert state == D.FINITE and np.array_equal(D.bits(got), D.bits(want))
    ref, tol = D.scatter_oracle(dest, t64, numel, p)
    assert (np.abs(got - ref) <= tol).all()
    if case["name"] == "colliding_9x9":
        assert adders >= 500 and (mask is None or float(mask.abs().max()) > 1)
        # the atomic form adds the same terms in fp32: inside the bound once the summation error of `adders` additions is allowed for
        autograd.set_deterministic(False)
        atomic = run_col2im(case, gcols, off, mask, mask_kind).cpu().numpy().ravel()
        mag = np.zeros(numel)
        np.add.at(mag, dest, np.abs(t64))
        assert (np.abs(atomic - ref) <= tol + adders * D.U * mag).all()


@pytest.mark.parametrize("case,off", COL2IM, ids=[c["name"] for c, _ in COL2IM])
def test_col2im_with_a_logit_mask_is_inside_the_bound_of_the_fp64_oracle(case, off):
    gcols, off, mask = col2im_inputs(case, off, "logit")
    autograd.set_deterministic(True)
    runs = [run_col2im(case, gcols, off, mask, "logit") for _ in range(5)]
    assert all(same_bits(runs[0], r) for r in runs[1:])
    dest, _, t64 = D.col2im_terms(gcols.numpy(), off.numpy(), mask.numpy(), mask_logit=True, **geom_kw(case))
    numel = runs[0].numel()
    state, p, _ = D.exponent(D.absmax_bits(gcols.numpy()), D.ONE_BITS, *D.col2im_bounds(case["k"], *G.out_hw(case)))
    ref, tol = D.scatter_oracle(dest, t64, numel, p)
    err = np.abs(runs[0].cpu().numpy().ravel() - ref)
    print(f"\n{case['name']}: at {float((err / np.maximum(tol, 1e-300)).max()):.3f} of the bound")
    assert state == D.FINITE and (err <= tol).all()


def test_col2im_zero_gradient_gives_zeros_and_inf_gives_all_nan():
    case, off = COL2IM[0]
    gcols, off, mask = col2im_inputs(case, off, "explicit")
    autograd.set_deterministic(True)
    out = run_col2im(case, torch.zeros_like(gcols), off, mask, "explicit")
    assert not bool(out.any()) and not bool(torch.signbit(out).any())
    bad = gcols.clone()
    bad[1, 7, 40] = float("inf")
    out = run_col2im(case, bad, off, mask, "explicit")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    bad[1, 7, 40] = float("nan")
    assert bool(torch.isnan(run_col2im(case, bad, off, None, "none")).all())
    bad_mask = mask.clone()
    bad_mask[0, 3, 2, 2] = float("-inf")
    assert bool(torch.isnan(run_col2im(case, gcols, off, bad_mask, "explicit")).all())
    # the atomic form poisons only what the value reaches (the documented difference)
    autograd.set_deterministic(False)
    out = run_col2im(case, bad, off, None, "none")
    assert bool(torch.isnan(out).any()) and not bool(torch.isnan(out).all())


# ---- RoIAlign backward -------------------------------------------------------------------------------------------------------------------------
ROI_B, ROI_C, ROI_H, ROI_W, ROI_P = 2, 8, 12, 20, 7


def roi_inputs():
    g = torch.Generator().manual_seed(29)
    one = torch.tensor([[1.0, 4.3, 2.6, 15.1, 10.2]])
    distinct = torch.tensor([[0, 0.5, 0.5, 6.0, 5.0], [1, -3.0, 1.0, 9.0, 13.5], [0, 8.2, 3.1, 19.9, 11.7], [1, 2.0, 2.0, 2.4, 2.3], [0, 15.0, 7.0, 23.0, 14.0],
                             [1, 0.0, 0.0, 20.0, 12.0], [0, 5.5, 5.5, 5.5, 5.5], [1, 10.0, 4.0, 13.0, 9.0]])
    rois = torch.cat([one.repeat(64, 1), distinct])
    gout = torch.randn(rois.shape[0], ROI_C, ROI_P, ROI_P, generator=g)
    return rois, gout


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("sr", [0, 2])
def test_roi_align_backward_fixed_point(aligned, sr):
    rois, gout = roi_inputs()
    shape = (ROI_B, ROI_C, ROI_H, ROI_W)
    autograd.set_deterministic(True)
    runs = [ops.roi_align_backward(gout.to(DEV), rois.to(DEV), shape, ROI_P, 1.0, sr, aligned) for _ in range(5)]
    assert all(same_bits(runs[0], r) for r in runs[1:])
    dest, t32, t64 = D.roi_terms(gout.numpy(), rois.numpy(), *shape, ROI_P, ROI_P, 1.0, sr, aligned)
    numel = runs[0].numel()
    want, state, p = D.det_result(dest, t32, numel, D.absmax_bits(gout.numpy()), D.ONE_BITS, *D.roi_bounds(rois.shape[0], ROI_P, ROI_P, sr))
    ref, tol = D.scatter_oracle(dest, t64, numel, p)
    got = runs[0].cpu().numpy().ravel()
    err = np.abs(got - ref)
    print(f"\naligned={aligned} sr={sr}: p = {p}, up to {np.bincount(dest, minlength=numel).max()} terms an address, at "
          f"{float((err / np.maximum(tol, 1e-300)).max()):.3f} of the bound, {int((D.bits(got) != D.bits(want)).sum())} words off the restatement")
    assert state == D.FINITE and (err <= tol).all()
    assert np.array_equal(D.bits(got), D.bits(want))
    # a permutation of the RoIs with their rows of grad_out: only an order-independent sum is indifferent to it
    perm = torch.randperm(rois.shape[0], generator=torch.Generator().manual_seed(3))
    again = ops.roi_align_backward(gout[perm].to(DEV), rois[perm].to(DEV), shape, ROI_P, 1.0, sr, aligned)
    assert same_bits(runs[0], again)
    # no RoIs: the output is written all the same
    none = ops.roi_align_backward(gout[:0].to(DEV), rois[:0].to(DEV), shape, ROI_P, 1.0, sr, aligned)
    assert none.shape == shape and not bool(none.any())


# ---- bilinear upsampling, adjoint --------------------------------------------------------------------------------------------------------------
UPSAMPLE_CASES = [((4, 6), (8, 12), None), ((5, 7), (12, 17), None), ((3, 5), (3, 5), None), ((6, 10), None, 2.0), ((1, 1), (4, 4), None),
                  ((2, 3), (5, 4), None)]


@pytest.mark.parametrize("in_hw,size,sf", UPSAMPLE_CASES, ids=[f"{i[0]}x{i[1]}" for i, _, _ in UPSAMPLE_CASES])
def test_upsample_adjoint(in_hw, size, sf):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, *in_hw, generator=g).to(DEV).requires_grad_()
    y = autograd.upsample_bilinear(x, size, sf)
    with torch.no_grad():
        assert same_bits(y, F.interpolate(x, size=size, scale_factor=sf, mode="bilinear", align_corners=False))
    go = torch.randn(y.shape, generator=g)
    (g1,) = torch.autograd.grad(y, x, go.to(DEV), retain_graph=True)
    (g2,) = torch.autograd.grad(y, x, go.to(DEV))
    assert same_bits(g1, g2) and g1.shape == x.shape
    ref, tol = D.upsample_adjoint(go.numpy(), *in_hw, scale_factor=sf)
    err = np.abs(g1.cpu().numpy().astype(np.float64) - ref)
    print(f"\n{in_hw} -> {tuple(y.shape[2:])}: at {float((err / np.maximum(tol, 1e-300)).max()):.3f} of the bound")
    assert (err <= tol).all()


# ---- modules under torch's flag ----------------------------------------------------------------------------------------------------------------
def _fpn_inputs():
    torch.manual_seed(0)
    fpn = FPN([8, 12, 16], get_cfg("STMask_plus_resnet50_config")).to(DEV)
    feats = [torch.randn(2, c, h, w, device=DEV, requires_grad=True) for c, h, w in ((8, 16, 24), (12, 8, 12), (16, 4, 6))]
    return fpn, feats, InterpolateModule(scale_factor=2, mode="bilinear", align_corners=False), torch.randn(1, 4, 6, 10, device=DEV, requires_grad=True)


def test_fpn_and_interpolate_module_run_under_the_flag():
    fpn, feats, up, x = _fpn_inputs()
    with torch.no_grad():
        plain = [o.clone() for o in fpn(feats)] + [up(x)]
    torch.use_deterministic_algorithms(True)
    grads = []
    for _ in range(2):
        outs = fpn(feats) + [up(x)]
        assert all(same_bits(a, b) for a, b in zip(outs, plain))                               # the forward is what it is without the flag
        grads.append(torch.autograd.grad(sum(o.square().sum() for o in outs), feats + [x] + list(fpn.parameters())))
    assert all(same_bits(a, b) for a, b in zip(*grads))


def _two_grads(module, *inputs):
    out = []
    for _ in range(2):
        module.zero_grad(set_to_none=True)
        ins = [t.clone().requires_grad_(t.is_floating_point() and req) for t, req in inputs]
        module(*ins).square().sum().backward()
        out.append([p.grad.clone() for p in module.parameters()] + [t.grad.clone() for t in ins if t.requires_grad])
    return out


def test_dcn_and_feature_align_gradients_are_bit_identical_over_two_runs():
    torch.manual_seed(1)
    torch.use_deterministic_algorithms(True)
    dcn = DCN(16, 16, 3, 1, 1, deformable_groups=2).to(DEV)
    with torch.no_grad():
        dcn.conv_offset_mask.weight.normal_(0, 0.05)            # offsets that move: zero weights would sample the grid itself
    a, b = _two_grads(dcn, (torch.randn(2, 16, 12, 20, device=DEV), True))
    assert len(a) == 5 and all(bool(g.any()) for g in a) and all(same_bits(x, y) for x, y in zip(a, b))
    fa = FeatureAlign(16, 12, kernel_size=(3, 5), deformable_groups=4).to(DEV)
    a, b = _two_grads(fa, (torch.randn(2, 16, 12, 20, device=DEV), True), (torch.randn(2, 4, 12, 20, device=DEV), False))
    assert all(bool(g.any()) for g in a) and all(same_bits(x, y) for x, y in zip(a, b))


def test_track_to_segment_loss_grad_concat_feat_is_bit_identical_over_two_runs():
    spec = TR.GOLDEN["p256_b2"]
    case = TR.draw_case(spec, 41000)
    mv = lambda v: v.to(DEV) if isinstance(v, torch.Tensor) else [[t.to(DEV) for t in pair] for pair in v]     # noqa: E731
    d = {k: mv(v) for k, v in case.items()}
    net = TR.StandInNet(TR.C_FEAT, spec["M"], TR.NET_SEED).to(DEV)
    torch.use_deterministic_algorithms(True)
    grads = []
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for _ in range(2):
            feat = d["concat_feat"].clone().requires_grad_()
            out = layers.track_to_segment_loss(net, feat, d["loc_ref"], d["ids_t"], d["mask_coeff_ref"], d["proto_next"], d["priors"], d["gt_bboxes"],
                                               d["gt_ids"], d["gt_masks"], boxshift_alpha=TR.ALPHA_B, maskshift_alpha=TR.ALPHA_M)
            (gf,) = torch.autograd.grad(out["B_shift"] + out["M_shift"], feat)
            grads.append(gf)
    assert bool(grads[0].any()) and same_bits(*grads)


# ---- one whole train step ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def start(tmp_path_factory):
    """R50 ada as a training run starts it, 2 clips at 128 x 192: the start state of tests/test_gpu_train_loop.py."""
    cfg = get_cfg(ADA)
    net = STMask(cfg)
    sd = synthetic.fill_state_dict(net, seed=0)
    path = os.path.join(str(tmp_path_factory.mktemp("backbone")), "backbone.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("backbone.")}, path)
    torch.manual_seed(0)
    net.init_weights(path)
    net = net.to(DEV).train()
    return cfg, net, synthetic.synthetic_train_batch(2, 128, 192, 0, device=DEV)


def _one_step(start):
    cfg, net, batch = start
    nl = NetLoss(copy.deepcopy(net), layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=64))
    opt = GuardedSGD(nl.net.parameters(), **SGD)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        losses = train_step(nl, opt, batch)
    return losses, nl, opt


def test_train_step_without_the_mode_is_refused_by_torch(start):
    """Under torch's flag with the mode switched off the step must not run: a RuntimeError in torch's words.  On a torch that refuses the atomic
    backward of bilinear F.interpolate it comes from there; torch 2.10 runs that interpolation as a decomposition and refuses nothing, and the
    error then comes from the fp32 atomic scatters of this library, which report under the flag as torch's own operators do
    (ops._alert_not_deterministic)."""
    torch.use_deterministic_algorithms(True)
    autograd.set_deterministic(False)
    with pytest.raises(RuntimeError, match="deterministic"):
        _one_step(start)


def test_train_step_under_the_flag_is_bit_identical_between_two_copies(start):
    torch.use_deterministic_algorithms(True)
    (la, a, opt_a), (lb, b, _) = _one_step(start), _one_step(start)
    assert opt_a.counters() == (1, 0) and len(la) == 7
    assert all(bool(torch.isfinite(v)) for v in la.values())
    assert [k for k in la if not same_bits(la[k], lb[k])] == []
    pa, pb = dict(a.net.named_parameters()), dict(b.net.named_parameters())
    with_grad = [n for n, p in pa.items() if p.grad is not None]
    assert len(with_grad) > 100
    # walking the backward order: the parameters nearest the loss come last in named_parameters()
    assert [n for n in reversed(with_grad) if not same_bits(pa[n].grad, pb[n].grad)] == []
    assert [n for n in pa if not same_bits(pa[n].detach(), pb[n].detach())] == []
    before = dict(start[1].named_parameters())
    moved = [n for n, p in pa.items() if not same_bits(p.detach(), before[n].detach())]
    assert len(moved) > 100
