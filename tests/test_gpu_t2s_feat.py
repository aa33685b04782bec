"""csrc/t2s_feat.hip on the MI355X: T2S_concat_feat and its adjoint (include/stmask_hip_t2s_feat.h) against the fp64 restatement of
tests/t2s_feat_restate.py, which tests/test_t2s_feat_cpu.py holds to the reference; the composed form of layers.t2s_concat_feat on the same inputs."""
import functools

import pytest
import torch

import t2s_feat_restate as R
from stmask_amd import autograd, layers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(R.CASES)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The fp64 forward and gradients of a case, computed once and left unchanged."""
    c = R.draw_case(name)
    out, corr, S = R.feature(c["fpn"], c["t2s"], c["P"])
    g_fpn, g_t2s, mag = R.gradients(c["fpn"], c["t2s"], c["grad_out"], c["P"])
    return dict(out=out, corr=corr, S=S, g_fpn=g_fpn, g_t2s=g_t2s, mag=mag)


def run(name, fused, grad=(True, True)):
    c = R.draw_case(name)
    fpn = c["fpn"].to(DEV).requires_grad_(grad[0])
    t2s = c["t2s"].to(DEV).requires_grad_(grad[1])
    out = layers.t2s_concat_feat(fpn, t2s, patch_size=c["P"], fused=fused)
    if any(grad):
        out.backward(c["grad_out"].to(DEV))
    return out.detach(), fpn.grad, t2s.grad


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_backward_against_fp64(name, fused):
    c, r = R.draw_case(name), restated(name)
    P, C = c["P"], c["fpn"].shape[1]
    PP = P * P
    out, g_fpn, g_t2s = run(name, fused)
    out, g_fpn, g_t2s = out.cpu(), g_fpn.cpu(), g_t2s.cpu()
    assert out.shape == r["out"].shape and out.dtype == torch.float32
    # ---- forward: the correlation channels inside the bound of any fp32 summation order, the copied channels exact
    fb = R.forward_bound(r["S"], C)
    d = (out[:, :PP].double() - r["out"][:, :PP]).abs()
    print(f"\n{name} {'fused' if fused else 'composed'}: forward worst |d| / bound {float((d / fb.clamp_min(1e-300)).max()):.3f}", end="")
    assert bool((d <= fb).all())
    assert torch.equal(out[:, PP:], torch.relu(torch.cat([c["t2s"][::2], c["t2s"][1::2]], 1)))
    assert torch.equal(out[:, :PP] > 0, r["corr"] > 0)                                   # the gate: the margin condition at work
    # ---- backward
    bb = R.backward_bound(r["mag"], C, P)
    d = (g_fpn.double() - r["g_fpn"]).abs()
    print(f"; grad_fpn worst |d| / bound {float((d / bb.clamp_min(1e-300)).max()):.3f}")
    assert bool((d <= bb).all())
    assert torch.equal(g_t2s.double(), r["g_t2s"])                                       # grad_out's two blocks, gated: a selection, exact
    Cu = c["t2s"].shape[1]
    gated = torch.cat([c["grad_out"][:, PP:PP + Cu], c["grad_out"][:, PP + Cu:]], 1).reshape(-1, Cu, *c["t2s"].shape[2:]) * (c["t2s"] > 0)
    assert torch.equal(g_t2s, gated) and not g_t2s[c["t2s"] <= 0].any()
    if R.CASES[name]["bs"] > 1:                                                          # the clip whose next frame is zero: gate closed everywhere
        assert not out[-1, :PP].any() and not g_fpn[-2:].any()
    assert bool((g_fpn[r["mag"] == 0] == 0).all())


@pytest.mark.parametrize("name", NAMES)
def test_same_bits_from_run_to_run_and_only_what_is_asked_for(name):
    a, b = run(name, True), run(name, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    out_f, g_fpn, none = run(name, True, grad=(True, False))
    assert none is None and torch.equal(g_fpn, a[1]) and torch.equal(out_f, a[0])
    out_t, none, g_t2s = run(name, True, grad=(False, True))
    assert none is None and torch.equal(g_t2s, a[2])
    out_n, _, _ = run(name, True, grad=(False, False))                                   # no autograd node at all: the plain launch
    assert torch.equal(out_n, a[0]) and not out_n.requires_grad


def test_no_host_synchronisation_and_no_double_backward():
    c = R.draw_case("odd_clips")
    fpn, t2s, go = c["fpn"].to(DEV).requires_grad_(), c["t2s"].to(DEV).requires_grad_(), c["grad_out"].to(DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = layers.t2s_concat_feat(fpn, t2s, patch_size=c["P"], fused=True)
        out.backward(go)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert isinstance(out.grad_fn, autograd.T2sConcatFeatFunction._backward_cls)
    out = layers.t2s_concat_feat(fpn, t2s, patch_size=c["P"], fused=True)
    (g,) = torch.autograd.grad(out, fpn, go, create_graph=True)
    with pytest.raises(RuntimeError) as e:
        g.sum().backward()
    assert "double backward" in str(e.value)
