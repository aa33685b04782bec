"""The mask loss tail on the MI355X -- layers.mask_bce_sum / layers.lincomb_mask_loss_image (stmask_amd/autograd.py and ops.py over
csrc/mask_loss.hip) -- held to the fp64 restatement of tests/mask_loss_restate.py, which test_mask_loss_cpu.py pins to torch's own
F.interpolate + clamp + F.binary_cross_entropy + autograd.

Tolerance everywhere (the project's form, layer_grad_restate.worst_ratio): |x - x64| <= 1e-5 * sum|terms| + 1e-7, sum|terms| being the same sum on
absolute values.  The reference's own fp32 torch chain stays inside it on these inputs (worst 0.016 on the loss, 0.72 on the gradient over the seeds of
test_mask_loss_cpu.py; the kernels' operation order evaluated in fp32 torch on a CPU gives 0.011 and 0.043).

Input condition: every tolerance case asserts that each nonzero prediction lies in [0.05, 0.95].  Within 1e-7 of 1, fp32 rounding decides between
log(1 - p) = -16.6 and the clamp at -100; no tolerance covers that jump and the reference's fp32 chain has it too.  The saturation and clamp cases leave
that range on purpose and are exact by construction instead: scales 2 and 4 with predictions that are small multiples of a power of two, so every
interpolated value -- and with it every decision at 0 and 1 -- is identical in fp32 and fp64.

Every case prints its figures before it asserts (run with -s).
"""
import functools

import pytest
import torch

import layer_grad_restate as LR
import mask_loss_restate as R
from stmask_amd import _lib, layers, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

RANDOM_SHAPES = [(12, 20, 48, 80), (12, 20, 24, 40), (12, 20, 12, 20), (12, 20, 31, 47), (12, 20, 45, 77), (5, 7, 33, 29)]
MULTI_TILE = (40, 72, 160, 288, 3)       # 10 x 3 forward tiles and 5 x 3 adjoint tiles per instance


@functools.lru_cache(maxsize=None)
def _case(h, w, H, W, n, kind="byte", with_idx=True):
    """inputs and the fp64 restatement -- computed once, shared, never modified"""
    pred, target, idx, gl = R.random_case(h, w, H, W, n, seed=1000 + 7 * H + n, kind=kind, with_idx=with_idx)
    return (pred, target, idx, gl), R.restate(pred, target, idx, gl)


def _to(t):
    return None if t is None else t.to(DEV)


def _run(pred, target, idx, gl):
    p = _to(pred).requires_grad_()
    loss = layers.mask_bce_sum(p, _to(target), _to(idx))
    assert loss.grad_fn is not None, "no gradient"
    loss.backward(_to(gl))
    return loss.detach(), p.grad


def _check(name, got_loss, got_grad, ref):
    loss, grad, mag_l, mag_g = ref
    rl, rg = R.worst_ratio(got_loss, loss, mag_l), R.worst_ratio(got_grad, grad, mag_g)
    print(f"\n{name}: worst |x - x64| / (1e-5 * sum|terms| + 1e-7): loss {rl:.4f} grad_pred {rg:.4f}")
    assert rl <= 1.0 and rg <= 1.0, (name, rl, rg)


@pytest.mark.parametrize("n", [1, 7, 65])
@pytest.mark.parametrize("h,w,H,W", RANDOM_SHAPES)
def test_byte_targets_through_an_index_match_fp64(h, w, H, W, n):
    (pred, target, idx, gl), ref = _case(h, w, H, W, n)
    assert R.input_condition(pred) and target.dtype == torch.uint8 and target.shape[0] != n
    if n >= 7:
        assert (pred == 0).any() and idx.unique().numel() < n               # cropped rows and repeated targets are present
    _check(f"{h}x{w} -> {H}x{W} n={n} bytes", *_run(pred, target, idx, gl), ref)


def test_several_workgroups_and_partials_per_instance_match_fp64():
    h, w, H, W, n = MULTI_TILE
    (pred, target, idx, gl), ref = _case(h, w, H, W, n)
    assert R.input_condition(pred)
    _check(f"{h}x{w} -> {H}x{W} n={n} bytes", *_run(pred, target, idx, gl), ref)


@pytest.mark.parametrize("kind", ["bool", "soft"])
@pytest.mark.parametrize("h,w,H,W", [(12, 20, 48, 80), (12, 20, 45, 77), (5, 7, 33, 29)])
def test_bool_and_soft_targets_match_fp64(h, w, H, W, kind):
    (pred, target, idx, gl), ref = _case(h, w, H, W, 7, kind=kind)
    assert R.input_condition(pred) and target.dtype == (torch.bool if kind == "bool" else torch.float32)
    if kind == "soft":
        assert ((target > 0) & (target < 1)).any() and target.min() >= 0 and target.max() <= 1
    _check(f"{h}x{w} -> {H}x{W} n=7 {kind}", *_run(pred, target, idx, gl), ref)


@pytest.mark.parametrize("h,w,H,W", [(12, 20, 48, 80), (12, 20, 31, 47)])
def test_without_an_index_row_i_uses_target_i(h, w, H, W):
    (pred, target, idx, gl), ref = _case(h, w, H, W, 7, with_idx=False)
    assert idx is None and target.shape[0] == 7 and R.input_condition(pred)
    _check(f"{h}x{w} -> {H}x{W} n=7 idx=None", *_run(pred, target, None, gl), ref)
    with pytest.raises(_lib.StmError, match="without idx"):
        ops.mask_bce_upsampled(_to(pred), _to(target)[:5])


def test_no_instances():
    pred, target = torch.zeros(0, 12, 20, device=DEV), torch.zeros(3, 48, 80, dtype=torch.uint8, device=DEV)
    idx = torch.zeros(0, dtype=torch.int64, device=DEV)
    assert layers.mask_bce_sum(pred, target, idx).shape == (0,)
    assert ops.mask_bce_upsampled_backward(torch.zeros(0, device=DEV), pred, target, idx).shape == (0, 12, 20)
    p = pred.clone().requires_grad_()
    layers.mask_bce_sum(p, target, idx).sum().backward()
    assert p.grad.shape == (0, 12, 20)


def test_non_contiguous_prediction_and_unaligned_target_view():
    (pred, target, idx, gl), ref = _case(12, 20, 45, 77, 7)
    wide = torch.zeros(7, 12, 23)
    wide[:, :, 2:22] = pred
    p = wide.to(DEV)[:, :, 2:22].requires_grad_()
    assert not p.is_contiguous()
    base = torch.zeros(target.shape[0] * 45 * 77 + 3, dtype=torch.uint8)
    base[1:-2] = target.flatten()
    t = base.to(DEV)[1:-2].view(target.shape)                              # the bytes start one past a 4-byte boundary
    assert t.data_ptr() % 4 == 1
    loss = layers.mask_bce_sum(p, t, _to(idx))
    (g,) = torch.autograd.grad(loss, p, _to(gl))
    _check("12x20 -> 45x77 n=7 strided pred, target at an odd address", loss.detach(), g, ref)


def _blocks(values, h, w, side, g):
    """[h,w] map made of side x side blocks, each of one value drawn from `values`"""
    pick = torch.randint(0, len(values), ((h + side - 1) // side, (w + side - 1) // side), generator=g)
    return torch.tensor(values)[pick].repeat_interleave(side, 0).repeat_interleave(side, 1)[:h, :w]


@pytest.mark.parametrize("scale", [2, 4])
def test_saturation_is_exact_by_construction(scale):
    """pred in {0, 0.5, 1} in 3 x 3 blocks: the 100s of the loss and the +-1e12 * weight terms of the gradient"""
    g = torch.Generator().manual_seed(50 + scale)
    n, h, w = 5, 12, 20
    H, W = h * scale, w * scale
    pred = torch.stack([_blocks([0.0, 0.5, 1.0], h, w, 3, g) for _ in range(n)]).float()
    target = torch.randint(0, 2, (3, H, W), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, 3, (n,), generator=g)
    gl = torch.randn(n, generator=g)
    up = R.upsample(pred, H, W)
    assert torch.equal(up.float().double(), up) and torch.equal(up, R.torch_chain_upsample32(pred, H, W).double())   # dyadic: fp32 == fp64
    t = target[idx]
    for pc, tv in ((0, 1), (1, 0), (0, 0), (1, 1)):
        assert ((up == pc) & (t == tv)).sum() >= 16, (pc, tv)
    ref = R.restate(pred, target, idx, gl)
    got = _run(pred, target, idx, gl)
    assert got[1].abs().max() >= 1e11
    _check(f"saturation x{scale}", *got, ref)


@pytest.mark.parametrize("scale", [2, 4])
def test_clamp_contributes_the_clamped_loss_and_no_gradient(scale):
    """pred in [-0.2, 1.2] as multiples of 1/16 (the input condition is lifted here): where the upsampled value is below 0 or above 1 the loss is that of
    0 or 1 and the gradient 0; exactly 0 and 1 count as inside"""
    g = torch.Generator().manual_seed(60 + scale)
    n, h, w = 5, 12, 20
    H, W = h * scale, w * scale
    pred = (torch.randint(-3, 20, (n, h, w), generator=g).float() / 16)
    assert pred.min() >= -0.2 and pred.max() <= 1.2 and (pred < 0).any() and (pred > 1).any()
    target = torch.randint(0, 2, (n, H, W), generator=g, dtype=torch.uint8)
    gl = torch.randn(n, generator=g)
    up = R.upsample(pred, H, W)
    assert torch.equal(up.float().double(), up) and torch.equal(up, R.torch_chain_upsample32(pred, H, W).double())
    assert (up < 0).sum() >= 16 and (up > 1).sum() >= 16 and ((up > 0) & (up < 1)).sum() >= 16
    ref = R.restate(pred, target, None, gl)
    got = _run(pred, target, None, gl)
    _check(f"clamp x{scale}", *got, ref)
    # a map that is outside [0, 1] everywhere: the loss of the clamped value, no gradient at all
    out = torch.where(torch.arange(n).view(n, 1, 1) % 2 == 0, torch.full((n, h, w), -0.125), torch.full((n, h, w), 1.125))
    loss, grad = _run(out, target, None, gl)
    assert torch.equal(grad, torch.zeros_like(grad))
    miss = torch.where(torch.arange(n) % 2 == 0, target.sum((1, 2)), H * W - target.sum((1, 2))).double() * 100
    assert ((loss.cpu().double() - miss).abs() <= 1e-5 * miss + 1e-7).all()


def test_two_calls_are_bit_identical():
    h, w, H, W, n = MULTI_TILE
    (pred, target, idx, gl), _ = _case(h, w, H, W, n)
    p, t, i, g = _to(pred), _to(target), _to(idx), _to(gl)
    a, b = ops.mask_bce_upsampled(p, t, i), ops.mask_bce_upsampled(p, t, i)
    ga, gb = ops.mask_bce_upsampled_backward(g, p, t, i), ops.mask_bce_upsampled_backward(g, p, t, i)
    assert torch.equal(a, b) and torch.equal(ga, gb) and torch.isfinite(a).all()


def test_autograd_plumbing():
    (pred, target, idx, gl), ref = _case(12, 20, 48, 80, 7, kind="soft")
    p, t, i = _to(pred), _to(target), _to(idx)
    plain = layers.mask_bce_sum(p, t, i)
    assert plain.grad_fn is None                                             # nothing requires grad: the plain launch
    pr = p.clone().requires_grad_()
    with torch.no_grad():
        assert layers.mask_bce_sum(pr, t, i).grad_fn is None
    loss = layers.mask_bce_sum(pr, t, i)
    assert loss.grad_fn is not None and torch.equal(loss.detach(), plain)    # the forward is the no-grad launch
    tr = t.clone().requires_grad_()
    assert layers.mask_bce_sum(p, tr, i).grad_fn is None                     # the target alone requires grad: no graph
    loss2 = layers.mask_bce_sum(pr, tr, i)
    loss2.backward(_to(gl))
    assert tr.grad is None and pr.grad is not None                           # no gradient to the target
    assert gl[0] == 0 and (gl > 0).any() and (gl < 0).any()                  # grad_loss of mixed signs and zeros
    assert torch.equal(pr.grad[0], torch.zeros_like(pr.grad[0]))
    _check("autograd 12x20 -> 48x80 soft", loss2.detach(), pr.grad, ref)
    pd = p.clone().requires_grad_()
    (gd,) = torch.autograd.grad(layers.mask_bce_sum(pd, t, i), pd, _to(gl), create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gd.sum().backward()


def test_an_index_outside_the_targets_gives_nan_for_that_row_only():
    (pred, target, idx, gl), ref = _case(12, 20, 45, 77, 7)
    G = target.shape[0]
    bad = idx.clone()
    bad[2], bad[5] = G, -1
    p, t = _to(pred), _to(target)
    loss = ops.mask_bce_upsampled(p, t, _to(bad))
    grad = ops.mask_bce_upsampled_backward(_to(gl), p, t, _to(bad))
    torch.cuda.synchronize()                                                 # the call returned normally
    good = torch.tensor([0, 1, 3, 4, 6])
    assert torch.isnan(loss[[2, 5]]).all() and torch.isnan(grad[[2, 5]]).all()
    assert torch.isfinite(loss[good]).all() and torch.isfinite(grad[good]).all()
    want_loss, want_grad = ops.mask_bce_upsampled(p, t, _to(idx)), ops.mask_bce_upsampled_backward(_to(gl), p, t, _to(idx))
    assert torch.equal(loss[good], want_loss[good]) and torch.equal(grad[good], want_grad[good])


# ---- the composite: generate_mask -> mask_bce_sum -> box normalisation -> weighted sum --------------------------------------------------------------
def _composite_case(h, w, n, scale, M, seed):
    proto, coeff, boxes, _ = LR.mask_case(h, w, n, seed, M=M, proto_scale=0.2)
    g = torch.Generator().manual_seed(seed + 1)
    G = n // 2 + 2
    masks_gt = torch.randint(0, 2, (G, h * scale, w * scale), generator=g, dtype=torch.uint8)
    return proto, coeff, boxes, masks_gt, torch.randint(0, G, (n,), generator=g), torch.rand(n, generator=g) + 0.5


def _composite_fp64(proto, coeff, boxes, masks_gt, idx, weights, scale):
    """(loss, grad_proto, grad_coeff, masks, grad_pred) in fp64: R.generate_mask + the restated tail"""
    h, w = proto.shape[:2]
    H, W = masks_gt.shape[1:]
    rect = LR.crop_rect(boxes, h, w)
    b64, w64 = boxes.double(), weights.double()
    if scale == 2:                                                           # torch ops with autograd, as test_gpu_layer_grads.py's composite
        p64, c64 = proto.double().requires_grad_(), coeff.double().requires_grad_()
        masks = LR.generate_mask(p64, c64, rect)
        loss = LR.mask_loss_tail(masks, b64, masks_gt[idx].double(), w64)
        loss.backward()
        return loss.detach(), p64.grad, c64.grad, masks.detach(), None
    masks = LR.generate_mask(proto.double(), coeff.double(), rect)
    bw = torch.clamp((b64[:, 2] - b64[:, 0]) * W, min=1)
    bh = torch.clamp((b64[:, 3] - b64[:, 1]) * H, min=1)
    gl = w64 / bw / bh
    per_inst, grad_pred, _, _ = R.restate(masks, masks_gt, idx, gl)
    gp, gc = LR.generate_mask_grads(proto.double(), coeff.double(), rect, grad_pred)
    return torch.sum(gl * per_inst), gp, gc, masks, grad_pred


@pytest.mark.parametrize("M", [8, 32])
@pytest.mark.parametrize("scale", [2, 4])
def test_lincomb_mask_loss_image_matches_fp64(scale, M):
    """Tolerances of test_gpu_layer_grads.py's composite: the loss within 1e-5 relative, every gradient within 1e-4 of its largest element."""
    h, w, n = 24, 40, 13
    proto, coeff, boxes, masks_gt, idx, weights = _composite_case(h, w, n, scale, M, seed=400 + 10 * scale + M)
    loss64, gp64, gc64, masks64, _ = _composite_fp64(proto, coeff, boxes, masks_gt, idx, weights, scale)
    nz = masks64[masks64 != 0]
    assert ((nz >= 0.05) & (nz <= 0.95)).all(), (nz.min().item(), nz.max().item())          # the input condition, asserted not assumed
    p, c = _to(proto).requires_grad_(), _to(coeff).requires_grad_()
    loss = layers.lincomb_mask_loss_image(p, c, _to(boxes), _to(masks_gt), _to(idx), _to(weights))
    assert loss.grad_fn is not None, "no gradient"
    loss.backward()
    dl = abs(loss.item() - loss64.item()) / abs(loss64.item())
    dp = (p.grad.cpu().double() - gp64).abs().max().item() / gp64.abs().max().item()
    dc = (c.grad.cpu().double() - gc64).abs().max().item() / gc64.abs().max().item()
    print(f"\ncomposite x{scale} M={M}: loss rel {dl:.2e}, grad_proto {dp:.2e} and grad_coeff {dc:.2e} of the largest element")
    assert torch.isfinite(p.grad).all() and torch.isfinite(c.grad).all()
    assert dl <= 1e-5
    assert (p.grad.cpu().double() - gp64).abs().max().item() <= 1e-4 * gp64.abs().max().item() + 1e-9
    assert (c.grad.cpu().double() - gc64).abs().max().item() <= 1e-4 * gc64.abs().max().item() + 1e-9
    with torch.no_grad():
        assert layers.lincomb_mask_loss_image(p, c, _to(boxes), _to(masks_gt), _to(idx), _to(weights)).grad_fn is None


def test_the_huge_gradient_outside_the_crops_does_not_reach_the_prototypes():
    h, w, n, scale = 24, 40, 13, 4
    proto, coeff, boxes, masks_gt, idx, weights = _composite_case(h, w, n, scale, 32, seed=470)
    rect = LR.crop_rect(boxes, h, w).float().to(DEV)
    p, c, b = _to(proto), _to(coeff), _to(boxes)
    masks = layers.generate_mask(p, c, b)
    grad_pred = ops.mask_bce_upsampled_backward(_to(weights), masks, _to(masks_gt), _to(idx))
    outside = grad_pred[rect == 0]
    assert (outside <= -1e11).sum() >= 16                                    # target 1 against an exactly-zero prediction
    gp0, gc0 = ops.lincomb_sigmoid_crop_backward(grad_pred * rect, p, c, b)
    gp1, gc1 = ops.lincomb_sigmoid_crop_backward(grad_pred, p, c, b)
    assert torch.isfinite(gp1).all() and torch.isfinite(gc1).all()
    assert torch.equal(gp0, gp1) and torch.equal(gc0, gc1)
