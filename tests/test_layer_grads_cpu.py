"""CPU checks behind test_gpu_layer_grads.py (no GPU): the fp64 restatements of generate_mask, decode and jaccard (tests/layer_grad_restate.py)
reproduce the reference's own fp64 outputs and autograd gradients (tests/golden/layer_grads.npz, written by tests/golden/gen_layer_grad_golden.py),
pass torch's gradcheck, and move by far more than the GPU test's bound under each of the mistakes a backward kernel could make -- so a GPU
gradient within the bound of the restatement is the reference's gradient.

Tolerances: 1e-12 relative on outputs, 1e-10 * magnitude (the gradient's sum of absolute terms) on gradients.
"""
import pytest
import torch

import layer_grad_restate as R
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("layer_grads.npz")


def _close_out(x, ref):
    assert x.shape == ref.shape and ((x - ref).abs() <= 1e-12 * ref.abs()).all()


def _close_grad(g, ref, mag):
    assert g.shape == ref.shape and ((g - ref).abs() <= 1e-10 * mag + 1e-300).all()


@pytest.mark.parametrize("tag", ["box", "nobox"])
def test_generate_mask_restatement_matches_the_reference(gold, tag):
    proto, coeff, go = gold["gm_proto"].double().requires_grad_(), gold["gm_coeff"].double().requires_grad_(), gold["gm_grad_out"].double()
    rect = R.crop_rect(gold["gm_boxes"], *proto.shape[:2]) if tag == "box" else None
    m = R.generate_mask(proto, coeff, rect)
    _close_out(m.detach(), gold[f"gm_{tag}_out"])
    m.backward(go)
    mag_p, mag_c = R.generate_mask_grads(proto.detach(), coeff.detach(), rect, go, absolute=True)
    _close_grad(proto.grad, gold[f"gm_{tag}_grad_proto"], mag_p)
    _close_grad(coeff.grad, gold[f"gm_{tag}_grad_coeff"], mag_c)
    gp, gc = R.generate_mask_grads(proto.detach(), coeff.detach(), rect, go)          # the closed form the magnitude is built on
    _close_grad(gp, gold[f"gm_{tag}_grad_proto"], mag_p)
    _close_grad(gc, gold[f"gm_{tag}_grad_coeff"], mag_c)
    if tag == "box":
        assert (gold["gm_box_out"] == 0).any() and (rect.sum((1, 2)) > 0).all()


def test_decode_restatement_matches_the_reference(gold):
    loc, pri, gb = gold["dec_loc"].double().requires_grad_(), gold["dec_priors"].double().requires_grad_(), gold["dec_grad_boxes"].double()
    d = R.decode(loc, pri)
    _close_out(d.detach(), gold["dec_out"])
    d.backward(gb)
    mag_l, mag_p = R.decode_grad_magnitude(loc.detach(), pri.detach(), gb)
    _close_grad(loc.grad, gold["dec_grad_loc"], mag_l)
    _close_grad(pri.grad, gold["dec_grad_priors"], mag_p)
    assert (mag_l >= loc.grad.abs() * (1 - 1e-12)).all() and (mag_p >= pri.grad.abs() * (1 - 1e-12)).all()


def test_jaccard_restatement_matches_the_reference(gold):
    a, b, gd = gold["jac_a"].double().requires_grad_(), gold["jac_b"].double().requires_grad_(), gold["jac_grad_diag"].double()
    assert R.jaccard_ties(a.detach(), b.detach()) == 0
    j = R.jaccard(a, b).diag()
    _close_out(j.detach(), gold["jac_diag"])
    j.backward(gd)
    mag_a, mag_b = R.jaccard_grad_magnitude(a.detach(), b.detach(), torch.diag(gd))
    _close_grad(a.grad, gold["jac_grad_a"], mag_a)
    _close_grad(b.grad, gold["jac_grad_b"], mag_b)
    assert (mag_a >= a.grad.abs() * (1 - 1e-12)).all() and (mag_b >= b.grad.abs() * (1 - 1e-12)).all()
    assert (gold["jac_diag"] == 0).any() and (gold["jac_diag"] > 0.3).any()           # disjoint and overlapping pairs


def _tail_run(gold, steps):
    """The composite case in fp64: TinyMaskHead from the fixture's weights, `steps` SGD steps; returns the net, the first loss and first gradients."""
    net = R.TinyMaskHead(4, 6, 8).double()
    with torch.no_grad():
        for p, k in ((net.proto.weight, "tail_proto_w"), (net.proto.bias, "tail_proto_b"), (net.coef.weight, "tail_coef_w"), (net.coef.bias, "tail_coef_b")):
            p.copy_(gold[k])
    boxes = gold["tail_boxes"]
    rect = R.crop_rect(boxes, 24, 40)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = net(gold["tail_x"].double(), gold["tail_feats"].double(), boxes.double(), gold["tail_mask_t"].double(), gold["tail_weights"].double(),
                   lambda p, c, b: R.generate_mask(p, c, rect))
        loss.backward()
        if first is None:
            first = (loss.item(), [p.grad.clone() for p in net.parameters()])
        opt.step()
    return net, first


def test_loss_tail_restatement_matches_the_reference(gold):
    _, (loss, grads) = _tail_run(gold, 1)
    assert abs(loss - gold["tail_loss"].item()) <= 1e-12 * abs(gold["tail_loss"].item())
    for g, k in zip(grads, ("tail_grad_proto_w", "tail_grad_proto_b", "tail_grad_coef_w", "tail_grad_coef_b")):
        assert ((g - gold[k]).abs() <= 1e-10 * gold[k].abs().max()).all(), k
    assert gold["tail_mask_t"].double().mul(1 - R.crop_rect(gold["tail_boxes"], 48, 80, padding=2)).sum() > 0   # targets of 1 outside the crop


def test_restatements_pass_gradcheck():
    g = torch.Generator().manual_seed(5)
    proto, coeff = torch.relu(torch.randn(3, 4, 5, generator=g)).double() + 0.01, torch.randn(3, 5, generator=g).double()
    rect = R.crop_rect(torch.tensor([[0.1, 0.2, 0.8, 0.9], [0.6, 0.1, 0.2, 0.5], [0.0, 0.0, 1.0, 1.0]]), 3, 4)
    assert torch.autograd.gradcheck(lambda p, c: R.generate_mask(p, c, rect), (proto.requires_grad_(), coeff.requires_grad_()))
    loc = torch.randn(4, 4, generator=g).double().requires_grad_()
    pri = (torch.rand(4, 4, generator=g).double() + 0.1).requires_grad_()
    assert torch.autograd.gradcheck(R.decode, (loc, pri))
    a, b = R.jaccard_boxes(3, 4, seed=6)
    assert R.jaccard_ties(a, b) == 0
    assert torch.autograd.gradcheck(R.jaccard, (a.double().requires_grad_(), b.double().requires_grad_()))


# ---- each GPU case would expose its own bug: the mistaken gradient is further than 100 x the GPU bound from the right one ------------------
def test_a_dropped_tanh_factor_or_an_ignored_crop_moves_the_mask_gradients_far_beyond_the_gpu_bound():
    for h, w, n in ((24, 40, 37), (35, 29, 70), (16, 16, 1), (12, 20, 33)):
        proto, coeff, boxes, go = R.mask_case(h, w, n, seed=100 + n)
        (gp, gc), (mag_p, mag_c) = R.mask_reference(proto, coeff, boxes, go)
        rect = R.crop_rect(boxes, h, w)
        _, gc_no_tanh = R.generate_mask_grads(proto.double(), coeff.double(), rect, go.double(), drop_tanh_factor=True)
        assert R.worst_ratio(gc_no_tanh, gc, mag_c) > 100, (h, w, n)
        gp_no_crop, gc_no_crop = R.generate_mask_grads(proto.double(), coeff.double(), None, go.double())
        assert R.worst_ratio(gp_no_crop, gp, mag_p) > 100 and R.worst_ratio(gc_no_crop, gc, mag_c) > 100, (h, w, n)


def test_a_decode_backward_that_forgets_the_in_place_step_moves_far_beyond_the_gpu_bound(golden_priors):
    """The mistake: d x2 / d w = 1 and d x2 / d cx = 0, i.e. `boxes[:, 2:] += boxes[:, :2]` differentiated with the updated x1 taken as a constant.
    (x2 = w + x1 and x2 = cx + w / 2 are the same function of cx and w and have the same derivative: that rewriting is checked to change nothing.)"""
    for n in (1, 257):
        g = torch.Generator().manual_seed(200 + n)
        loc, pri, gb = torch.randn(n, 4, generator=g).double(), golden_priors["p_48x80"][:n].double(), torch.randn(n, 4, generator=g).double()
        grads = {}
        for form in ("inplace", "centre", "detached_x1"):
            l = loc.clone().requires_grad_()
            R.decode(l, pri, form).backward(gb)
            grads[form] = l.grad
        mag_l, _ = R.decode_grad_magnitude(loc, pri, gb)
        assert R.worst_ratio(grads["centre"], grads["inplace"], mag_l) <= 1e-6
        assert R.worst_ratio(grads["detached_x1"], grads["inplace"], mag_l) > 100, n
