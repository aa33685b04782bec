"""The train-mode STMask.forward on the MI355X: the reference's goldens (tests/golden/gen_train_forward_golden.py) in the fused and the composed form
of T2S_concat_feat, gradient reach through NetLoss over layers.MultiBoxLoss, a first-order check of the gradient, and train_step."""
import functools
import os

import pytest
import torch

import t2s_feat_restate as R
from conftest import load_golden
from stmask_amd import layers, model as model_mod, synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.train import NetLoss, train_step
from train_forward_views import CASES, KEYS, golden_input, strided, train_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADA = "STMask_plus_resnet50_ada_config"
TERMS = ["BIoU", "M", "C", "center", "B_shift", "M_shift", "T"]


@pytest.mark.parametrize("name,tag", CASES)
def test_train_forward_against_the_reference_goldens(name, tag, monkeypatch):
    g = load_golden(f"model_train_{tag}.npz")
    net = train_net(name, DEV)
    x = golden_input(g).to(DEV)
    seen = []
    real = model_mod.t2s_concat_feat
    monkeypatch.setattr(model_mod, "t2s_concat_feat", lambda fpn, t2s, **kw: (seen.append((fpn.detach().cpu(), t2s.detach().cpu())), real(fpn, t2s, **kw))[1])
    outs = {}
    # MIOpen's default convolution choices are not bit-reproducible from one call to the next on this device (the FPN alone differs by 1e-7 between
    # two calls on one input); the two forms are compared bit for bit, so both forwards run with its deterministic solvers
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for form, fused in (("fused", True), ("composed", False)):
            net.fused_t2s_feat = fused
            outs[form] = net(x)
    assert net.training and sorted(outs["fused"]) == sorted(outs["composed"]) == KEYS
    worst = {}
    for form, out in outs.items():
        assert list(out["priors"].shape) == g["priors_shape"].tolist()
        for k, v in strided(out).items():
            m = float((v.cpu() - g[k]).abs().max()) / float(g["dev_" + k])
            worst[k] = max(worst.get(k, 0.0), m)
    print(f"\n{tag}: worst |device - golden| in multiples of the reference's own fp32-vs-fp64 deviation: " +
          "  ".join(f"{k} {m:.2f}" for k, m in worst.items()))
    assert all(m <= 8.0 for m in worst.values()), worst
    for k in KEYS:
        if k != "T2S_concat_feat":
            assert torch.equal(outs["fused"][k], outs["composed"][k]), k
    # T2S_concat_feat: both forms inside the kernel bound of the fp64 feature of the very maps the net handed over
    (fpn, t2s), (fpn2, t2s2) = seen
    assert torch.equal(fpn, fpn2) and torch.equal(t2s, t2s2)
    ref, _, S = R.feature(fpn, t2s, 11)
    bound = R.forward_bound(S, fpn.shape[1])
    for form in outs:
        got = outs[form]["T2S_concat_feat"].cpu()
        assert bool(((got[:, :121].double() - ref[:, :121]).abs() <= bound).all()), form
        assert torch.equal(got[:, 121:].double(), ref[:, 121:]), form


def criterion(cfg):
    return layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3)


@functools.lru_cache(maxsize=None)
def batch(seed):
    return synthetic.synthetic_train_batch(2, 128, 192, seed, device=DEV)


def ada_net_loss(tmp_path, freeze_bn=False, fused=True):
    """R50 ada as a training run starts it: init_weights from a backbone file (the seeded synthetic backbone), Xavier heads, zero biases.  (The
    heads of synthetic.fill_state_dict are calibrated for inference -- a background bias of 6.2, unit-variance coefficients: the summed loss starts
    near 70 with |g|^2 near 1e5 and the reference's SGD settings reach NaN in three steps.)"""
    cfg = get_cfg(ADA)
    cfg.freeze_bn = freeze_bn
    net = STMask(cfg)
    sd = synthetic.fill_state_dict(net, seed=0)
    path = os.path.join(str(tmp_path), "backbone.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("backbone.")}, path)
    torch.manual_seed(0)
    net.init_weights(path)
    net = net.to(DEV).train()
    net.fused_t2s_feat = fused
    return NetLoss(net, criterion(cfg))


def test_every_parameter_gets_a_finite_gradient(tmp_path):
    nl = ada_net_loss(tmp_path)
    losses = nl(*batch(0))
    assert sorted(losses) == sorted(TERMS)
    sum(losses.values()).backward()
    missing = [n for n, p in nl.net.named_parameters() if p.grad is None]
    bad = [n for n, p in nl.net.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    dead = [n for n, p in nl.net.named_parameters() if p.grad is not None and not bool(p.grad.any())]
    print(f"\n{len(list(nl.net.parameters()))} parameters; without gradient: {missing}; not finite: {bad}; all-zero: {dead}")
    assert missing == [] and bad == []          # no exceptions: every parameter of R50 ada is on a path to some loss term
    # the gradient paths this item opened: the FCB class branch (its deformable conv, its offset conv) and the heads beside it
    for n in ("prediction_layers.0.conf_layer.0.conv_adaption.weight", "prediction_layers.0.conf_layer.0.conv_offset.weight",
              "prediction_layers.0.conf_extra.0.weight", "TemporalNet.conv1.weight", "fpn.lat_layers.0.weight", "backbone.conv1.weight"):
        assert n not in dead, n
    frozen = ada_net_loss(tmp_path, freeze_bn=True, fused=False)
    sum(frozen(*batch(0)).values()).backward()
    for mod in frozen.net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert not mod.training and mod.weight.grad is None and mod.bias.grad is None
    assert frozen.net.backbone.conv1.weight.grad is not None


def test_first_order_decrease_matches_the_gradient(tmp_path):
    """A plain SGD step of size eps with eps |g|^2 = 1e-3 of the summed loss lowers the loss on the same batch by that much to first order: the
    measured decrease must lie within [0.5, 1.5] of the prediction.  A missing or wrong gradient path shows as a ratio far outside.  Seed 0 of the
    batch; no other seed had to be picked.

    Measured on the MI355X, term by term (measured / predicted decrease of each term along the step): BIoU 1.00, M 0.93, C 1.00, center 1.00,
    B_shift 1.01, T 1.00 and M_shift 7.9; the sum 1.32 (batch seed 1: 1.39).  M_shift is the one term whose value moves without a gradient saying
    so: layers.track_to_segment_loss reads mask_coeff_ref and proto_next detached (its documented behaviour; the reference lets that gradient
    through), and the step moves both through losses['M'].  INTEGRATION.md section 19 records it."""
    nl = ada_net_loss(tmp_path)
    data = batch(0)
    total = lambda: sum(v.double() for v in nl(*data).values())                          # noqa: E731
    loss0 = total()
    loss0.backward()
    loss0 = loss0.detach()
    params = [p for p in nl.net.parameters() if p.grad is not None]
    g2 = float(sum(p.grad.double().pow(2).sum() for p in params))
    eps = 1e-3 * float(loss0) / g2
    with torch.no_grad():
        for p in params:
            p.add_(p.grad, alpha=-eps)
        loss1 = total()
    predicted, measured = eps * g2, float(loss0) - float(loss1)
    print(f"\nloss {float(loss0):.6f} -> {float(loss1):.6f}, |g|^2 {g2:.4e}, eps {eps:.3e}: measured / predicted decrease = {measured / predicted:.4f}")
    assert 0.5 <= measured / predicted <= 1.5


def test_three_train_steps_then_eval(tmp_path):
    nl = ada_net_loss(tmp_path)
    net = nl.net
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)    # reference config.py:402-405
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    for step in range(3):
        losses = train_step(nl, opt, batch(step))
        assert sorted(losses) == sorted(TERMS)
        vals = {k: float(v) for k, v in losses.items()}
        print(f"\nstep {step}: " + "  ".join(f"{k} {v:.4f}" for k, v in vals.items()), end="")
        assert all(torch.isfinite(v) for v in losses.values()) and all(not v.requires_grad for v in losses.values()), vals
    unchanged = [n for n, p in net.named_parameters() if torch.equal(p.detach(), before[n])]
    assert unchanged == [], unchanged
    net.eval()
    frame = synthetic.synthetic_clip(1, 128, 192, seed=0).to(DEV)
    with torch.no_grad():
        det = net(frame, img_meta=[{"is_first": True, "video_id": 0, "frame_id": 0}])[0]["detection"]
    assert "box" in det and bool(torch.isfinite(det["box"]).all())
