"""optim.DataParallelSGD.step (csrc/optim.hip) on the MI355X: bit-equality with the numpy restatement of tests/dp_restate.py over every path of
the kernel, the gradients and pads left at exactly zero, world == 1 against stm_sgd_step_multi_f32, the guard (which still clears the
gradients), the refusals, and steps without host synchronisation."""
import numpy as np
import pytest
import torch

import dp_restate as D
import optim_restate as R
from stmask_amd import _lib
from stmask_amd._lib import StmError
from stmask_amd.optim import CHUNK, MAX_TENSORS, DataParallelSGD, GuardedSGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (elements, storage offset of the parameter): every size at which the kernel takes another path, then a dense view at storage offset 1 (all
# of its chunks take the 4-byte path, the arena's segments being on the 16-byte grid), then small tensors up to one more than a launch's table
SPECS = ([(n, 0) for n in (2 * CHUNK + 5, 0, 1, 3, 4, CHUNK - 1, CHUNK, CHUNK + 1)] + [(CHUNK + 5, 1), (6, 1)] +
         [(7 + i, 0) for i in range(MAX_TENSORS + 1 - 10)])
assert len(SPECS) == MAX_TENSORS + 1
HYPER = dict(momentum=0.9, weight_decay=1e-4)
LRS = (1e-3, 0.0137)


def view(values, off):
    base = torch.zeros(len(values) + off, dtype=torch.float32, device=DEV)
    base[off:].copy_(torch.from_numpy(values))
    v = base[off:off + len(values)]
    assert v.storage_offset() == off
    return v


def summed_grads(step, world, specs):
    """The fp32 sum over `world` ranks of seeded per-rank gradients (summed in rank order: what the arena holds after the exchange)."""
    out = []
    for i, (n, _) in enumerate(specs):
        s = np.zeros(n, np.float32)
        for r in range(world):
            s = s + R.seeded_values(n, 1000 * (step + 1) + 100 * r + i, scales=(1.0, 1e-4, 1e2))
        out.append(s)
    return out


class Case:
    """The first `count` tensors of SPECS on the device under a DataParallelSGD, beside their numpy twins."""

    def __init__(self, count, world, seed=0, guard="loss", preset_momentum=True):
        self.specs, self.world = SPECS[:count], world
        self.p_np = [R.seeded_values(n, seed + i) for i, (n, _) in enumerate(self.specs)]
        self.m_np = [R.seeded_values(n, seed + 500 + i, scales=(1e-2, 1.0, 1e2)) if preset_momentum else np.zeros(n, np.float32)
                     for i, (n, _) in enumerate(self.specs)]
        self.params = [torch.nn.Parameter(view(v, off)) for v, (_, off) in zip(self.p_np, self.specs)]
        self.opt = DataParallelSGD(self.params, lr=LRS[0], guard=guard, world=world, rank=world - 1, **HYPER)
        for m, v in zip(self.opt.momentum.views, self.m_np):
            m.copy_(torch.from_numpy(v))

    def set_grads(self, values, loss=0.5):
        for v, g in zip(self.opt.grads.views, values):
            v.copy_(torch.from_numpy(g))
        self.opt.grads.write_tail([torch.tensor(loss, dtype=torch.float32, device=DEV)])

    def numpy_step(self, values, lr):
        for i in range(len(self.specs)):
            self.p_np[i], self.m_np[i], _ = D.finish_f32(self.p_np[i], values[i], self.m_np[i], self.world, lr, HYPER["momentum"], HYPER["weight_decay"])

    def assert_bits(self, what):
        for i, p in enumerate(self.params):
            assert np.array_equal(D.bits(p.detach().cpu().numpy()), D.bits(self.p_np[i])), (what, "parameter", i, self.specs[i])
            m = self.opt.state[p]["momentum_buffer"]
            assert m is self.opt.momentum.views[i]
            assert np.array_equal(D.bits(m.cpu().numpy()), D.bits(self.m_np[i])), (what, "momentum", i, self.specs[i])

    def assert_cleared(self, what):
        """Every gradient element is exactly +0.0f, and so is every pad of both arenas."""
        g = self.opt.grads
        assert not bool(g.flat[:g.tail_offset].view(torch.int32).any()), what
        assert not bool(self.opt.momentum.pads().view(torch.int32).any()), what
        assert all(p.grad is v for p, v in zip(self.params, g.views))


# ---- bit-equality --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, MAX_TENSORS, MAX_TENSORS + 1])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_two_steps_bit_equal_to_the_restatement_and_the_gradients_cleared(world, count):
    case = Case(count, world)
    assert count <= 8 or case.params[8].data_ptr() % 16 == 4              # the view at storage offset 1 is off the 16-byte grid
    for step, lr in enumerate(LRS):
        case.opt.param_groups[0]["lr"] = lr
        s = summed_grads(step, world, case.specs)
        case.set_grads(s)
        case.opt.step()
        case.numpy_step(s, lr)
        case.assert_bits(f"step {step}")
        case.assert_cleared(f"step {step}")
        assert float(case.opt.grads.tail[0]) == 0.5                        # the tail is not the kernel's to clear
    assert case.opt.counters() == (2, 0)                                  # counted once per step, one launch or two


def test_one_rank_is_the_single_rank_kernel_bit_for_bit():
    ours, theirs = Case(len(SPECS), 1, seed=7), Case(len(SPECS), 1, seed=7)
    ref = GuardedSGD(theirs.params, lr=LRS[0], guard="loss", **HYPER)
    held = []
    for i, p in enumerate(theirs.params):
        ref.state[p]["momentum_buffer"] = view(theirs.m_np[i], 0)
    for step, lr in enumerate(LRS):
        s = summed_grads(step, 1, SPECS)
        ours.opt.param_groups[0]["lr"] = ref.param_groups[0]["lr"] = lr
        ours.set_grads(s)
        ours.opt.step()
        for p, g in zip(theirs.params, s):
            held.append(torch.from_numpy(g).to(DEV) if g.size else None)      # the tensor without elements sits the reference's step out
            p.grad = held[-1]
        ref.step(torch.tensor(0.5, device=DEV))
        for i, (a, b) in enumerate(zip(ours.params, theirs.params)):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), (step, i)
            assert torch.equal(ours.opt.momentum.views[i].view(torch.int32), ref.state[b]["momentum_buffer"].view(torch.int32)), (step, i)
    assert ours.opt.counters() == ref.counters() == (2, 0)


def test_a_parameter_no_gradient_reached_still_steps():
    """The documented difference from GuardedSGD: g = 0, so weight decay and momentum act."""
    case = Case(5, 2, seed=3)
    zeros = [np.zeros(n, np.float32) for n, _ in case.specs]
    case.opt.grads.write_tail([torch.tensor(1.0, device=DEV)])
    case.opt.step()
    case.numpy_step(zeros, LRS[0])
    case.assert_bits("no gradient")
    assert any(not np.array_equal(D.bits(a), D.bits(R.seeded_values(n, 3 + i))) for i, ((n, _), a) in enumerate(zip(case.specs, case.p_np)))


# ---- the guard ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_reduced_loss_that_is_not_finite_skips_the_step_and_still_clears_the_gradients(bad):
    case = Case(len(SPECS), 2, seed=9)
    s = summed_grads(0, 2, SPECS)
    s[0][-1] = np.float32("nan")                            # what a skipped step usually comes with: it must not survive either
    case.set_grads(s, loss=bad)
    case.opt.step()
    case.assert_bits("skipped")                            # parameters and momentum unchanged bit for bit
    case.assert_cleared("skipped")
    assert case.opt.counters() == (0, 1)
    s = summed_grads(1, 2, SPECS)
    case.set_grads(s, loss=0.25)
    case.opt.step()
    case.numpy_step(s, LRS[0])
    case.assert_bits("applied")
    case.assert_cleared("applied")
    assert case.opt.counters() == (1, 1)


@pytest.mark.parametrize("where", [2, 0, 8], ids=["size-1", "tail-chunk", "odd-offset"])
def test_a_reduced_gradient_that_is_not_finite_skips_the_step_and_is_cleared(where):
    case = Case(len(SPECS), 3, seed=11, guard="grads")
    applied = skipped = 0
    for step, poison in enumerate((float("nan"), None, float("inf"), None)):
        s = summed_grads(step, 3, SPECS)
        if poison is not None:
            s[where][-1] = poison
        case.set_grads(s, loss=1.0)                        # the loss is finite: only the flat gradient check (bad = 1) can stop the step
        case.opt.step()
        if poison is None:
            case.numpy_step(s, LRS[0])
            applied += 1
        else:
            skipped += 1
        case.assert_bits(f"step {step} ({poison})")
        case.assert_cleared(f"step {step} ({poison})")
        assert case.opt.counters() == (applied, skipped)
    case.set_grads(summed_grads(7, 3, SPECS), loss=float("nan"))     # guard="grads" honours the loss too (the tail is part of the reduced arena)
    case.opt.step()
    case.assert_bits("nan loss")
    case.assert_cleared("nan loss")
    assert case.opt.counters() == (applied, skipped + 1)


def test_guard_none_applies_whatever_the_loss():
    case = Case(12, 2, seed=13, guard=None)
    s = summed_grads(0, 2, case.specs)
    case.set_grads(s, loss=float("nan"))
    case.opt.step()
    case.numpy_step(s, LRS[0])
    case.assert_bits("applied")
    case.assert_cleared("applied")
    assert case.opt.counters() == (1, 0)


# ---- refusals and arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,code,text", D.FINISH_REFUSALS, ids=D.REFUSAL_IDS)
def test_finish_refusals_return_their_codes_without_a_launch(change, code, text):
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    kw = dict(counters=counters.data_ptr())
    kw.update(change)
    with pytest.raises(StmError) as e:
        _lib.private_call("stm_dp_sgd_finish_multi_f32", *D.finish_args(**kw))
    assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)
    assert counters.tolist() == [0, 0]                      # nothing ran on the stream


def test_step_refuses_a_rebound_gradient_before_any_launch():
    case = Case(5, 2, seed=15)
    case.params[3].grad = torch.zeros_like(case.params[3])
    with pytest.raises(ValueError, match="parameter 3"):
        case.opt.step()
    with pytest.raises(ValueError, match="no loss and no closure"):
        case.opt.step(torch.tensor(1.0, device=DEV))
    assert case.opt.counters() == (0, 0)


# ---- no host synchronisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", ["loss", "grads"])
def test_three_steps_without_a_host_synchronisation(guard):
    case = Case(len(SPECS), 2, seed=17, guard=guard)
    grads = [summed_grads(s, 2, SPECS) for s in range(3)]
    staged = [[torch.from_numpy(v).to(DEV) for v in g] for g in grads]
    loss = torch.tensor(1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in range(3):
            for v, g in zip(case.opt.grads.views, staged[step]):
                v.copy_(g)
            case.opt.grads.write_tail([loss])
            case.opt.step()
            case.opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for step in range(3):
        case.numpy_step(grads[step], LRS[0])
    case.assert_bits(guard)
    case.assert_cleared(guard)
    assert case.opt.counters() == (3, 0)
