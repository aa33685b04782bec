"""The hazard the guarded step exists for, end to end on the MI355X: a batch whose positive lists overflow (max_pos=1: the documented NaN losses
and gradients) through train_step.  With optim.GuardedSGD the weights stay as they were and the step is counted as skipped; with torch.optim.SGD
the same step fills the weights with NaN.  With a sufficient max_pos the step is applied and train.LossLog reads finite terms."""
import copy
import math
import os

import pytest
import torch

from stmask_amd import layers, synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.optim import GuardedSGD
from stmask_amd.train import LossLog, NetLoss, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADA = "STMask_plus_resnet50_ada_config"
TERMS = ["BIoU", "M", "C", "center", "B_shift", "M_shift", "T"]
SGD = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)                   # reference config.py:402-405


@pytest.fixture(scope="module")
def start(tmp_path_factory):
    """R50 ada as a training run starts it (init_weights from the seeded synthetic backbone, Xavier heads), built once; every test takes a copy."""
    cfg = get_cfg(ADA)
    net = STMask(cfg)
    sd = synthetic.fill_state_dict(net, seed=0)
    path = os.path.join(str(tmp_path_factory.mktemp("backbone")), "backbone.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("backbone.")}, path)
    torch.manual_seed(0)
    net.init_weights(path)
    net = net.to(DEV).train()
    batch = synthetic.synthetic_train_batch(2, 128, 192, 0, device=DEV)   # the smallest size the train-forward tests use
    return cfg, net, batch


def net_loss(start, max_pos):
    cfg, net, batch = start
    return NetLoss(copy.deepcopy(net), layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=max_pos)), batch


def test_an_overflowing_batch_is_skipped_and_counted_where_torch_sgd_loses_the_run(start):
    nl, batch = net_loss(start, max_pos=1)
    twin = copy.deepcopy(nl)
    before = {n: p.detach().clone() for n, p in nl.net.named_parameters()}
    opt = GuardedSGD(nl.net.parameters(), **SGD)
    # MIOpen's deterministic solvers, as where the train-forward tests compare bit for bit
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        losses = train_step(nl, opt, batch)
        assert sorted(losses) == sorted(TERMS)
        assert not math.isfinite(float(sum(losses.values())))            # the lists overflowed: the documented NaN
        assert any(not bool(torch.isfinite(p.grad).all()) for p in nl.net.parameters())
        changed = [n for n, p in nl.net.named_parameters() if not torch.equal(p.detach().view(torch.int32), before[n].view(torch.int32))]
        assert changed == []
        assert opt.counters() == (0, 1)
        assert all(not bool(s["momentum_buffer"].any()) for s in opt.state.values())       # the buffers stayed zeros as well
        # the same step with the optimizer the loop used until now: NaN in the weights
        plain = torch.optim.SGD(twin.net.parameters(), **SGD)
        train_step(twin, plain, batch)
    lost = [n for n, p in twin.net.named_parameters() if not bool(torch.isfinite(p).all())]
    print(f"\ntorch.optim.SGD after the overflowing batch: {len(lost)} of {len(before)} parameter tensors hold a value that is not finite")
    assert lost != []


def test_with_room_in_the_lists_the_step_is_applied_and_the_log_reads_finite_terms(start):
    nl, batch = net_loss(start, max_pos=64)                             # the batch has fewer positives: its terms equal those of max_pos=None
    before = {n: p.detach().clone() for n, p in nl.net.named_parameters()}
    opt = GuardedSGD(nl.net.parameters(), **SGD)
    log = None
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for _ in range(2):
            losses = train_step(nl, opt, batch)
            log = log or LossLog(list(losses), capacity=8)
            log.append(losses)
    assert opt.counters() == (2, 0)
    # every tensor moved, but for biases that start at zero (no weight decay to move them) on FPN levels this batch sends no gradient to
    unchanged = {n: p for n, p in nl.net.named_parameters() if torch.equal(p.detach(), before[n])}
    assert len(unchanged) < 8 and all(not bool(p.grad.any()) and not bool(p.any()) for p in unchanged.values()), sorted(unchanged)
    got = log.read()
    print("\n" + "  ".join(f"{k} {v:.4f} (mean {avg:.4f})" for k, (v, avg) in got.items()))
    assert sorted(got) == sorted(TERMS + ["Total"]) and len(log.rows) == 2
    assert all(math.isfinite(v) and math.isfinite(avg) for v, avg in got.values())
    assert got["Total"][0] == pytest.approx(sum(got[k][0] for k in TERMS), rel=1e-5)
