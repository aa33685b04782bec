"""Gradients of the rebound layer functions on the MI355X -- layers.mask_utils.generate_mask, layers.box_utils.decode and jaccard (stmask_amd/autograd.py
over csrc/lincomb_backward.hip and csrc/mask_backward.hip) -- held to the fp64 restatements of tests/layer_grad_restate.py, which test_layer_grads_cpu.py pins to the reference's own
fp64 autograd.  The tests call only stmask_amd.layers and the restatements: on a tree without the backward kernels every case fails with "no gradient".

Tolerance (the project's form): |g - g64| <= rel * sum|terms| + 1e-7, sum|terms| being the same gradient on absolute values.
  decode, jaccard: short fixed expressions, rel = 1e-5 as it stands.
  generate_mask: the yardstick is the reference's own op chain (tanh, matmul, sigmoid, crop, permute) in fp32 torch on the same inputs, held to the same
    fp64 values.  Measured on a CPU at rel = 1e-5 that chain's worst |g - g64| / bound is 0.15-0.34 at 24x40x37, 0.29-0.41 at 35x29x70, 0.23-0.72 at
    96x160x100 and 2.2 with the prototypes x3: the error is the fp32 rounding of the logit (32 products of O(1)) carried into s (1 - s), and it grows with
    the logit's size.  The kernel's summation order and expf differ from torch's only in rounding, so it gets 2 x the chain's worst at unit scale,
    2 x 0.72 = 1.44, tightened to the project's usual 1.0: the unit-scale cases assert worst <= 1.0 at rel = 1e-5 (a wrong term -- no 1 - t^2, no
    crop -- moves the result by more than 100 x that, test_layer_grads_cpu.py).  The saturated case (prototypes x8) computes the chain's ratio itself
    on the CPU and asserts kernel <= 2 * max(chain, 1).
  Measured on an MI355X at rel = 1e-5 (every case prints its figures before it asserts; run with -s):
      case                      kernel grad_proto   kernel grad_coeff   fp32 torch chain (CPU, worse of the two gradients)
      24x40x37 boxes                 0.036               0.028               0.142
      24x40x37 no boxes              0.018               0.005               0.071
      35x29x70 boxes                 0.020               0.025               0.181
      35x29x70 no boxes              0.012               0.007               0.127
      16x16x1  boxes                 0.040               0.015               0.069
      16x16x1  no boxes              0.055               0.006               0.187
      12x20x33 boxes                 0.029               0.026               0.317
      12x20x33 no boxes              0.023               0.010               0.236
      24x40x37 prototypes x8         0.221               0.192              10.979
    (the kernel's fused-multiply-add logit and its cancellation-free e / (1 + e)^2 and 1 - t^2 = 4 e / (1 + e)^2 forms sit well inside the chain's error)
"""
import copy
import functools

import pytest
import torch

import layer_grad_restate as R
from conftest import load_golden
from stmask_amd import layers
from stmask_amd.layers import box_utils, mask_utils

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(24, 40, 37), (35, 29, 70), (16, 16, 1), (12, 20, 33)]


@functools.lru_cache(maxsize=None)
def _mask_case(h, w, n, with_boxes, proto_scale=1.0):
    """inputs, fp64 gradients, magnitudes and the fp32 chain's worst ratios -- computed once, shared, never modified"""
    proto, coeff, boxes, go = R.mask_case(h, w, n, seed=100 + n, with_boxes=with_boxes, proto_scale=proto_scale)
    ref, mag = R.mask_reference(proto, coeff, boxes, go)
    chain = R.generate_mask_chain_fp32(proto, coeff, boxes, go)
    return (proto, coeff, boxes, go), ref, mag, max(R.worst_ratio(chain[0], ref[0], mag[0]), R.worst_ratio(chain[1], ref[1], mag[1]))


def _run(proto, coeff, boxes, go, need_proto=True, need_coeff=True):
    p, c = proto.to(DEV).requires_grad_(need_proto), coeff.to(DEV).requires_grad_(need_coeff)
    m = mask_utils.generate_mask(p, c, None if boxes is None else boxes.to(DEV))
    m.backward(go.to(DEV))
    return m, p, c


def _ratios(name, p, c, ref, mag, chain):
    assert p.grad is not None and c.grad is not None, f"{name}: no gradient"
    kp, kc = R.worst_ratio(p.grad, ref[0], mag[0]), R.worst_ratio(c.grad, ref[1], mag[1])
    print(f"\n{name}: worst |g - g64| / (1e-5 * sum|terms| + 1e-7): kernel grad_proto {kp:.3f} grad_coeff {kc:.3f} | fp32 torch chain (CPU) {chain:.3f}")
    return max(kp, kc)


@pytest.mark.parametrize("with_boxes", [True, False], ids=["boxes", "no_boxes"])
@pytest.mark.parametrize("h,w,n", SHAPES)
def test_generate_mask_gradients_match_fp64(h, w, n, with_boxes):
    inputs, ref, mag, chain = _mask_case(h, w, n, with_boxes)
    m, p, c = _run(*inputs)
    assert m.grad_fn is not None, "no gradient"
    worst = _ratios(f"{h}x{w}x{n} {'boxes' if with_boxes else 'no boxes'}", p, c, ref, mag, chain)
    assert worst <= 1.0, worst
    if with_boxes:
        rect = R.crop_rect(inputs[2], h, w)
        assert ((m.detach().cpu() == 0) | (rect == 1)).all()         # the forward cropped with the same rectangles
        if n >= 33:
            assert (rect.sum((1, 2)) <= 16).any() and (rect.sum((1, 2)) == h * w).any()     # tiny and whole-frame rows are present


@pytest.mark.parametrize("M", [8, 64])
def test_generate_mask_gradients_at_the_other_mask_dims(M):
    """the forward's other two instantiations (M = 32 is every other case): 4 and 32 pixel groups in the grad_coeff layout"""
    proto, coeff, boxes, go = R.mask_case(12, 20, 33, seed=140 + M, M=M)
    ref, mag = R.mask_reference(proto, coeff, boxes, go)
    chain = R.generate_mask_chain_fp32(proto, coeff, boxes, go)
    _, p, c = _run(proto, coeff, boxes, go)
    worst = _ratios(f"12x20x33 M={M}", p, c, ref, mag, max(R.worst_ratio(chain[0], ref[0], mag[0]), R.worst_ratio(chain[1], ref[1], mag[1])))
    assert worst <= 1.0, worst


def test_generate_mask_saturated_prototypes_stay_finite_and_within_the_chains_error():
    inputs, ref, mag, chain = _mask_case(24, 40, 37, True, 8.0)
    _, p, c = _run(*inputs)
    assert torch.isfinite(p.grad).all() and torch.isfinite(c.grad).all()
    worst = _ratios("24x40x37 prototypes x8", p, c, ref, mag, chain)
    assert worst <= 2 * max(chain, 1.0), (worst, chain)


def test_generate_mask_does_not_read_grad_out_outside_the_crop():
    """-1e12 everywhere outside the rectangles (the reference's BCE gradient where the target is 1 and the cropped mask 0) must give gradients
    bit-identical to zeros there."""
    (proto, coeff, boxes, go), _, _, _ = _mask_case(24, 40, 37, True)
    rect = R.crop_rect(boxes, 24, 40).float()
    _, p0, c0 = _run(proto, coeff, boxes, go * rect)
    _, p1, c1 = _run(proto, coeff, boxes, go * rect + (1 - rect) * -1e12)
    assert p0.grad is not None and torch.isfinite(p1.grad).all()
    assert torch.equal(p0.grad, p1.grad) and torch.equal(c0.grad, c1.grad)


def test_generate_mask_autograd_plumbing():
    (proto, coeff, boxes, go), ref, mag, _ = _mask_case(35, 29, 70, True)
    m, p, c = _run(proto, coeff, boxes, go)
    with torch.no_grad():
        m0 = mask_utils.generate_mask(proto.to(DEV), coeff.to(DEV), boxes.to(DEV))
    assert m0.grad_fn is None and m.grad_fn is not None and torch.equal(m0, m.detach())     # the forward is the no-grad launch
    assert mask_utils.generate_mask(proto.to(DEV), coeff.to(DEV), boxes.to(DEV)).grad_fn is None
    _, p2, c2 = _run(proto, coeff, boxes, go)
    assert torch.equal(p.grad, p2.grad) and torch.equal(c.grad, c2.grad)                    # run to run bit-identical
    _, p3, c3 = _run(proto, coeff, boxes, go, need_coeff=False)
    assert c3.grad is None and torch.equal(p3.grad, p.grad)
    _, p4, c4 = _run(proto, coeff, boxes, go, need_proto=False)
    assert p4.grad is None and torch.equal(c4.grad, c.grad)
    # two calls on one proto accumulate
    pa = proto.to(DEV).requires_grad_()
    ca, cb = coeff[:40].to(DEV).requires_grad_(), coeff[40:].to(DEV).requires_grad_()
    (mask_utils.generate_mask(pa, ca, boxes[:40].to(DEV)) * go[:40].to(DEV)).sum().backward()
    (mask_utils.generate_mask(pa, cb, boxes[40:].to(DEV)) * go[40:].to(DEV)).sum().backward()
    assert R.worst_ratio(pa.grad, ref[0], mag[0]) <= 1.0
    assert R.worst_ratio(torch.cat((ca.grad, cb.grad)), ref[1], mag[1]) <= 1.0
    # no double backward
    pd, cd = proto.to(DEV).requires_grad_(), coeff.to(DEV).requires_grad_()
    (g,) = torch.autograd.grad(mask_utils.generate_mask(pd, cd, boxes.to(DEV)), pd, go.to(DEV), create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        g.sum().backward()
    # the empty early return stays as it is
    assert mask_utils.generate_mask(pd, cd[:0], boxes[:0].to(DEV)).shape == (0, 35, 29)


@pytest.mark.parametrize("n", [1, 257])
def test_decode_gradients_match_fp64(n, golden_priors):
    g = torch.Generator().manual_seed(200 + n)
    loc, pri, gb = torch.randn(n, 4, generator=g), golden_priors["p_48x80"][:n].float(), torch.randn(n, 4, generator=g)
    lg, pg = loc.to(DEV).requires_grad_(), pri.to(DEV).requires_grad_()
    with torch.no_grad():
        d0 = box_utils.decode(loc.to(DEV), pri.to(DEV))
    d = box_utils.decode(lg, pg)
    assert d.grad_fn is not None and torch.equal(d0, d.detach()), "no gradient"
    d.backward(gb.to(DEV))
    l64, p64 = loc.double().requires_grad_(), pri.double().requires_grad_()
    R.decode(l64, p64).backward(gb.double())
    mag_l, mag_p = R.decode_grad_magnitude(loc.double(), pri.double(), gb.double())
    assert R.worst_ratio(lg.grad, l64.grad, mag_l) <= 1.0
    assert R.worst_ratio(pg.grad, p64.grad, mag_p) <= 1.0
    l2 = loc.to(DEV).requires_grad_()                              # loc only: the usual call (priors are constants)
    box_utils.decode(l2, pri.to(DEV)).backward(gb.to(DEV))
    assert torch.equal(l2.grad, lg.grad)
    with pytest.raises(RuntimeError, match="double backward"):
        l3 = loc.to(DEV).requires_grad_()
        torch.autograd.grad(box_utils.decode(l3, pri.to(DEV)), l3, gb.to(DEV), create_graph=True)[0].sum().backward()


def _jaccard_ref(a, b, go):
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    R.jaccard(a64, b64).backward(go.double())
    return (a64.grad, b64.grad), R.jaccard_grad_magnitude(a.double(), b.double(), go.double())


@pytest.mark.parametrize("A,B", [(1, 1), (37, 37), (5, 300)])
def test_jaccard_gradients_match_fp64(A, B):
    a, b = R.jaccard_boxes(A, B, seed=300 + B)
    assert R.jaccard_ties(a, b) == 0
    iou = R.jaccard(a.double(), b.double())
    if A > 1:
        assert (iou == 0).any() and (iou > 0.3).any()              # disjoint and overlapping pairs
    g = torch.Generator().manual_seed(301)
    full = torch.randn(A, B, generator=g)
    diag = torch.zeros(A, B)
    diag.diagonal().copy_(torch.randn(min(A, B), generator=g))
    with torch.no_grad():
        j0 = box_utils.jaccard(a.to(DEV), b.to(DEV))
    for name, go in (("full", full), ("diag", diag)):
        ag, bg = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
        j = box_utils.jaccard(ag, bg)
        assert j.grad_fn is not None and torch.equal(j0, j.detach()), "no gradient"
        if name == "diag":
            j.diag().backward(go.diagonal().to(DEV))               # the use in get_DIoU
        else:
            j.backward(go.to(DEV))
        ref, mag = _jaccard_ref(a, b, go)
        assert R.worst_ratio(ag.grad, ref[0], mag[0]) <= 1.0, name
        assert R.worst_ratio(bg.grad, ref[1], mag[1]) <= 1.0, name
    a1 = a.to(DEV).requires_grad_()                                # one side only
    box_utils.jaccard(a1, b.to(DEV)).backward(full.to(DEV))
    ref, mag = _jaccard_ref(a, b, full)
    assert R.worst_ratio(a1.grad, ref[0], mag[0]) <= 1.0


def test_jaccard_batched_form_and_refusals():
    a0, b0 = R.jaccard_boxes(7, 19, seed=310)
    a1, b1 = R.jaccard_boxes(7, 19, seed=311)
    a, b = torch.stack((a0, a1)), torch.stack((b0, b1))
    go = torch.randn(2, 7, 19, generator=torch.Generator().manual_seed(312))
    ag, bg = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    j = box_utils.jaccard(ag, bg)
    assert j.shape == (2, 7, 19) and j.grad_fn is not None, "no gradient"
    j.backward(go.to(DEV))
    for i, (x, y) in enumerate(((a0, b0), (a1, b1))):
        ref, mag = _jaccard_ref(x, y, go[i])
        assert R.worst_ratio(ag.grad[i], ref[0], mag[0]) <= 1.0 and R.worst_ratio(bg.grad[i], ref[1], mag[1]) <= 1.0
    with pytest.raises(NotImplementedError):
        box_utils.jaccard(ag[0], bg[0], iscrowd=True)
    assert box_utils.jaccard(ag[0][:0], bg[0]).shape == (0, 19)


def test_mask_loss_tail_trains_as_the_fp64_restatement():
    """The tail of lincomb_mask_loss on the 24x40 fixture through layers.generate_mask (the torch ops after it in fp32 on the GPU), 3 SGD steps from the
    fixture's weights on the GPU and in fp64 on the CPU.  Stated tolerances (those of test_gpu_autograd.py): every gradient within 1e-4 of its largest
    element, every parameter within 1e-5 * (1 + its largest element) after each step, the loss within 1e-5 relative."""
    gold = load_golden("layer_grads.npz")
    net64 = R.TinyMaskHead(4, 6, 8).double()
    with torch.no_grad():
        for p, k in ((net64.proto.weight, "tail_proto_w"), (net64.proto.bias, "tail_proto_b"), (net64.coef.weight, "tail_coef_w"), (net64.coef.bias, "tail_coef_b")):
            p.copy_(gold[k])
    netg = copy.deepcopy(net64).float().to(DEV)
    x, feats, boxes, mask_t, wts = gold["tail_x"], gold["tail_feats"], gold["tail_boxes"], gold["tail_mask_t"], gold["tail_weights"]
    rect = R.crop_rect(boxes, 24, 40)
    opt, opt64 = torch.optim.SGD(netg.parameters(), lr=0.05), torch.optim.SGD(net64.parameters(), lr=0.05)
    losses = []
    for step in range(3):
        opt.zero_grad()
        opt64.zero_grad()
        loss = netg(x.to(DEV), feats.to(DEV), boxes.to(DEV), mask_t.float().to(DEV), wts.to(DEV), layers.generate_mask)
        loss64 = net64(x.double(), feats.double(), boxes.double(), mask_t.double(), wts.double(), lambda p, c, b: R.generate_mask(p, c, rect))
        loss.backward()
        loss64.backward()
        if step == 0:
            assert abs(loss64.item() - gold["tail_loss"].item()) <= 1e-12 * gold["tail_loss"].item()
        assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item()), step
        for (n, p), (_, p64) in zip(netg.named_parameters(), net64.named_parameters()):
            assert p.grad is not None, f"step {step}: {n} has no gradient"
            d = (p.grad.cpu().double() - p64.grad).abs().max().item()
            assert d <= 1e-4 * p64.grad.abs().max().item() + 1e-9, f"step {step}: {n}.grad differs by {d}"
        opt.step()
        opt64.step()
        for (n, p), (_, p64) in zip(netg.named_parameters(), net64.named_parameters()):
            d = (p.detach().cpu().double() - p64.detach()).abs().max().item()
            assert d <= 1e-5 * (1 + p64.detach().abs().max().item()), f"step {step}: {n} differs by {d} after the update"
        losses.append(loss64.item())
    assert losses[2] < losses[1] < losses[0], losses
