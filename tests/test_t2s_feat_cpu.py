"""tests/t2s_feat_restate.py, the fp64 yardstick of tests/test_gpu_t2s_feat.py, held to the reference's own correlate + relu(cat)
(tests/golden/gen_t2s_feat_golden.py), and the margin condition the GPU cases rely on; the composed layers.t2s_concat_feat on the CPU oracle."""
import pytest
import torch

import t2s_feat_restate as R
from conftest import load_golden
from oracle.cpu_path import oracle_ops
from stmask_amd import layers

REF = [n for n, s in R.CASES.items() if s["ref"]]


def test_case_table():
    assert REF == ["smallest", "odd_clips"] and len(R.CASES) == 8
    shapes = [(s["bs"], s["C"], s["Cu"], s["h"], s["w"], s["P"]) for s in R.CASES.values()]
    assert shapes == [(1, 8, 4, 3, 4, 3), (3, 20, 8, 5, 8, 11), (2, 18, 6, 6, 37, 11), (2, 32, 16, 24, 40, 11), (1, 16, 8, 4, 80, 11),
                      (1, 12, 4, 3, 70, 5), (2, 6, 2, 5, 9, 13), (1, 5, 2, 4, 70, 15)]
    for name, s in R.CASES.items():
        c = R.draw_case(name)
        imgs = c["fpn"].flatten(1)
        assert len({tuple(r[:4].tolist()) for r in imgs}) == imgs.shape[0]                # distinct values in every image
        assert (c["t2s"] < 0).any() and (c["t2s"] == 0).any()
        if s["bs"] > 1:
            assert not c["fpn"][-1].any() and c["fpn"][-2].any()


@pytest.mark.parametrize("name", REF)
def test_restatement_against_the_reference(name):
    g = load_golden("t2s_feat_cases.npz")
    c = R.draw_case(name)
    assert float(g[name + "_fpn_sum"]) == float(c["fpn"].double().sum()) and float(g[name + "_t2s_sum"]) == float(c["t2s"].double().sum())
    out, corr, S = R.feature(c["fpn"], c["t2s"], c["P"])
    PP, C = c["P"] ** 2, c["fpn"].shape[1]
    ref = g[name].double()
    assert ref.shape == out.shape
    # the reference sums in its own order, divides by C and applies leaky_relu in fp32: inside the bound of any fp32 order
    bound = R.forward_bound(S, C)
    d = (ref[:, :PP] - out[:, :PP]).abs()
    print(f"\n{name}: worst |ref - fp64| / bound = {float((d / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((d <= bound).all())
    assert torch.equal(ref[:, PP:], out[:, PP:])
    assert torch.equal(g[name][:, PP:], torch.relu(torch.cat([c["t2s"][::2], c["t2s"][1::2]], 1)))
    if R.CASES[name]["bs"] > 1:
        assert not out[-1, :PP].any() and not ref[-1, :PP].any()                          # the clip whose next frame is zero


@pytest.mark.parametrize("name", list(R.CASES))
def test_margin_condition(name):
    """No correlation value sits within the forward bound of 0 without being exactly 0, so fp32 and fp64 agree on the gate of every element."""
    assert R.margin_ok(name)
    c = R.draw_case(name)
    _, corr, _ = R.feature(c["fpn"], c["t2s"], c["P"])
    assert (corr == 0).any() and (corr > 0).any() and (corr < 0).any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_restated_gradients_are_the_contract(name):
    """The restatement's autograd against the formulas of include/stmask_hip_t2s_feat.h written out for one element each."""
    c = R.draw_case(name)
    fpn, t2s, go, P = c["fpn"].double(), c["t2s"].double(), c["grad_out"].double(), c["P"]
    g_fpn, g_t2s, mag = R.gradients(c["fpn"], c["t2s"], c["grad_out"], P)
    out, _, _ = R.feature(fpn, t2s, P)
    n, C, h, w = fpn.shape
    PP, Cu, Rr = P * P, t2s.shape[1], P // 2
    gt = go * (out > 0)
    assert torch.equal(g_t2s[::2], gt[:, PP:PP + Cu]) and torch.equal(g_t2s[1::2], gt[:, PP + Cu:])
    assert not g_t2s[t2s <= 0].any()
    gen = torch.Generator().manual_seed(1)
    for _ in range(6):
        b, ch, y, x = (int(torch.randint(0, m, (1,), generator=gen)) for m in (n // 2, C, h, w))
        e0 = e1 = 0.0
        for i in range(P):
            for j in range(P):
                dy, dx = i - Rr, j - Rr
                if 0 <= y + dy < h and 0 <= x + dx < w:
                    e0 += float(gt[b, i * P + j, y, x] * fpn[2 * b + 1, ch, y + dy, x + dx])
                if 0 <= y - dy < h and 0 <= x - dx < w:
                    e1 += float(gt[b, i * P + j, y - dy, x - dx] * fpn[2 * b, ch, y - dy, x - dx])
        assert abs(e0 / C - float(g_fpn[2 * b, ch, y, x])) < 1e-12 and abs(e1 / C - float(g_fpn[2 * b + 1, ch, y, x])) < 1e-12
    assert bool((mag >= g_fpn.abs() * C * (1 - 1e-12)).all())


@pytest.mark.parametrize("name", REF + ["ragged"])
def test_composed_form_on_the_cpu_oracle(name):
    c = R.draw_case(name)
    with oracle_ops(), torch.no_grad():
        got = layers.t2s_concat_feat(c["fpn"], c["t2s"], patch_size=c["P"])
    out, _, S = R.feature(c["fpn"], c["t2s"], c["P"])
    PP = c["P"] ** 2
    assert bool(((got[:, :PP].double() - out[:, :PP]).abs() <= R.forward_bound(S, c["fpn"].shape[1])).all())
    assert torch.equal(got[:, PP:].double(), out[:, PP:])
    if name in REF:
        ref = load_golden("t2s_feat_cases.npz")[name]            # both within the bound of fp64 (the oracle scales in double, the reference in fp32)
        assert bool(((got[:, :PP] - ref[:, :PP]).abs().double() <= 2 * R.forward_bound(S, c["fpn"].shape[1])).all()) and torch.equal(got[:, PP:], ref[:, PP:])
    with pytest.raises(ValueError):
        layers.t2s_concat_feat(c["fpn"][:1], c["t2s"][:1], patch_size=c["P"])
