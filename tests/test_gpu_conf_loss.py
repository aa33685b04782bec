"""The OHEM class-confidence loss kernels (csrc/conf_loss.hip) behind layers.select_neg_bboxes / layers.ohem_conf_loss on the MI355X, held to
the fp64 restatement of the conventions (tests/conf_loss_restate.py): the selected set exactly -- against the reference's own set on the golden
cases, which keep a margin at the cut -- and loss and gradient within the derived bounds
    |C - C64| <= 16 eps alpha / (ratio + 1) sum_i w_i (max_c |x_ic| + |ce_i|),
    |grad - grad64| <= |g| alpha / (ratio + 1) w_i eps (8 + max_c |x_ic - lse_i|)   per element,   eps = 2^-24.
The observed fraction of each bound is printed; the largest over the cases is in INTEGRATION.md section 14."""
import os

import numpy as np
import pytest
import torch

import conf_loss_restate as R
from conftest import ROOT
from stmask_amd import _lib, layers, ops

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(ROOT, "tests", "golden", "conf_loss_cases.npz"))
RATIO, ALPHA = int(R.scalar(Z["ratio"])), R.scalar(Z["conf_alpha"])
GOLDEN = [str(n) for n in Z["case_names"]]
CONSTRUCTED = R.constructed_cases()
G = 0.75                                 # the incoming gradient (exact in fp32)
_inputs, _restated = {}, {}


def case(name):
    if name not in _inputs:
        _inputs[name] = R.golden_case(Z, name) if name in GOLDEN else CONSTRUCTED[name]
    return _inputs[name]


def restated(name, mode):
    if (name, mode) not in _restated:
        _restated[name, mode] = R.restate(*case(name), RATIO, ALPHA, mode, g=G)
    return _restated[name, mode]


def run_forward_backward(x, t, mode):
    """(loss, grad) through autograd, with every host synchronisation turned into an error while the launches are made."""
    xg = x.clone().requires_grad_(True)
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = layers.ohem_conf_loss(xg, t, RATIO, ALPHA, weights=mode)
        (G * loss).backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    return loss, xg.grad


@pytest.mark.parametrize("mode", ["reference", "aligned"])
@pytest.mark.parametrize("name", GOLDEN + list(CONSTRUCTED))
def test_selection_loss_and_gradient(name, mode):
    conf, conf_t = case(name)
    r = restated(name, mode)
    x, t = conf.cuda(), conf_t.cuda()
    N, C = r["N"], r["C"]

    neg = layers.select_neg_bboxes(x.clone().requires_grad_(True), t, RATIO)
    assert neg.dtype == torch.float32 and tuple(neg.shape) == (N,) and neg.grad_fn is None and not neg.requires_grad
    assert bool(((neg == 0) | (neg == 1)).all())
    assert torch.equal(neg.cpu() > 0, r["neg"])
    if name in GOLDEN:                   # the reference's own selection
        assert torch.equal(neg.cpu() > 0, torch.from_numpy(np.unpackbits(Z[f"{name}__neg"])[:N].astype(bool)))

    plain, lse, w = ops.ohem_conf_loss(x, t, RATIO, ALPHA, mode)
    assert torch.equal(w.cpu() != 0, r["keep"])
    assert float((w.cpu().double() - r["w"]).abs().max()) <= float(r["w"].max()) * R.EPS
    assert float(((lse.cpu().double() - r["lse"]).abs() / r["lse"].abs().clamp(min=1.0)).max()) <= R.EPS * (1 + 1e-6)
    with torch.no_grad():
        quiet = layers.ohem_conf_loss(x.clone().requires_grad_(True), t, RATIO, ALPHA, weights=mode)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)

    loss, grad = run_forward_backward(x, t, mode)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None
    assert torch.equal(loss.detach(), plain)                            # the forward through autograd is the plain launch
    loss2, grad2 = run_forward_backward(x, t, mode)
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(grad2, grad)     # bit-identical run to run

    assert tuple(grad.shape) == tuple(x.shape)
    grad = grad.cpu().double().view(N, C)
    err_loss = abs(float(loss) - float(r["loss"]))
    err_grad = (grad - r["grad"]).abs()
    kept = r["keep"].nonzero()[:, 0]
    frac_loss = err_loss / float(r["loss_bound"]) if float(r["loss_bound"]) > 0 else 0.0
    frac_grad = float((err_grad[kept] / r["grad_bound"][kept, None]).max()) if kept.numel() else 0.0
    print(f"{name} {mode}: loss {float(loss):.6f} (restated {float(r['loss']):.6f}), kernel / bound: loss {frac_loss:.3f}, gradient {frac_grad:.3f}")
    assert bool(torch.isfinite(grad).all()) and np.isfinite(float(loss))
    assert err_loss <= float(r["loss_bound"])
    assert bool((err_grad <= r["grad_bound"][:, None]).all())
    if bool((~r["keep"]).any()):                                        # rows that weigh nothing are written as exact zeros
        assert float(grad[~r["keep"]].abs().max()) == 0.0
    if r["k"] == 0:
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    if name in GOLDEN and mode == "reference":                          # and the reference's own fp32 numbers, through the two bounds
        assert abs(float(loss) - float(R.scalar(Z[f"{name}__loss"]))) <= 2 * float(r["loss_bound"])


def test_double_backward_raises():
    conf, conf_t = case("p37")
    xg = conf.cuda().requires_grad_(True)
    loss = layers.ohem_conf_loss(xg, conf_t.cuda(), RATIO, ALPHA)
    (gx,) = torch.autograd.grad(loss, xg, create_graph=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        gx.sum().backward()


def test_label_outside_the_classes_is_nan_for_its_row_only():
    conf, conf_t = case("wide")
    conf_t = conf_t.clone()
    row = int((conf_t.view(-1) > 0).nonzero()[0])
    conf_t.view(-1)[row] = conf.shape[-1]
    r = R.restate(conf, conf_t, RATIO, ALPHA, "aligned", g=G)
    loss, grad = run_forward_backward(conf.cuda(), conf_t.cuda(), "aligned")
    torch.cuda.synchronize()                                            # the call returned normally and so does the device
    grad = grad.cpu().double().view(-1, conf.shape[-1])
    assert bool(torch.isnan(loss)) and bool(torch.isnan(grad[row]).all())
    others = torch.ones(r["N"], dtype=torch.bool)
    others[row] = False
    assert bool(torch.isfinite(grad[others]).all())
    assert bool(((grad[others] - r["grad"][others]).abs() <= r["grad_bound"][others, None]).all())
    assert torch.equal(layers.select_neg_bboxes(conf.cuda(), conf_t.cuda(), RATIO).cpu() > 0, r["neg"])


def test_flat_unaligned_and_half_inputs():
    """[N, C] with [N] is one image; a view that is not 16-byte aligned and fp16 logits go through the same kernels."""
    conf, conf_t = case("p37")
    x, t = conf.cuda(), conf_t.cuda()
    base = ops.ohem_conf_loss(x, t, RATIO, ALPHA)[0]
    assert torch.equal(layers.ohem_conf_loss(x.view(-1, x.shape[-1]), t.view(-1), RATIO, ALPHA), base)
    buf = torch.empty(x.numel() + 1, device="cuda")
    shifted = buf[1:].view_as(x)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(layers.ohem_conf_loss(shifted, t, RATIO, ALPHA), base)
    half = x.half()
    assert torch.equal(layers.ohem_conf_loss(half, t, RATIO, ALPHA), ops.ohem_conf_loss(half.float(), t, RATIO, ALPHA)[0])
    assert torch.equal(layers.select_neg_bboxes(half, t, RATIO), ops.ohem_select_neg(half.float(), t, RATIO))


def test_shapes_are_refused_before_any_launch():
    t = torch.zeros(2, 300, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.StmError, match="C=129"):
        layers.ohem_conf_loss(torch.zeros(2, 300, 129, device="cuda"), t)
    with pytest.raises(_lib.StmError, match="C=1 "):
        layers.select_neg_bboxes(torch.zeros(2, 300, 1, device="cuda"), t)
    with pytest.raises(_lib.StmError, match="int64"):
        layers.ohem_conf_loss(torch.zeros(2, 300, 41, device="cuda"), t.int())
    with pytest.raises(_lib.StmError, match="int64"):
        layers.ohem_conf_loss(torch.zeros(2, 300, 41, device="cuda"), t[:, :299])
    with pytest.raises(_lib.StmError, match="rows"):
        ops.ohem_select_neg(torch.zeros(1, (1 << 22) + 1, 2, device="cuda"), torch.zeros(1, (1 << 22) + 1, dtype=torch.int64, device="cuda"))
