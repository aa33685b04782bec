"""optim.GuardedSGD on the MI355X: bit-equality with the numpy restatement of tests/optim_restate.py over every path of the kernel, torch's SGD on
the device inside the derived bound, the guard (loss, gradients, none), steps without host synchronisation, and resuming from a checkpoint."""
import os

import numpy as np
import pytest
import torch

import optim_restate as R
from stmask_amd import checkpoint
from stmask_amd.optim import CHUNK, MAX_TENSORS, GuardedSGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (elements, storage offset of the parameter, of its gradient, of a preset momentum buffer, has a gradient)
SPECS = ([(n, 0, 0, 0, True) for n in (1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 2)] +
         [(CHUNK + 5, 1, 2, 3, True),         # a view at an odd storage offset: every chunk takes the 4-byte path
          (2 * CHUNK + 3, 0, 1, 0, True),     # only the gradient is off the 16-byte grid
          (300, 4, 8, 12, True),              # views inside their storage, all on the grid
          (77, 0, 0, 0, False)] +             # no gradient: left out of the step
         [(7 + i, 0, 0, 0, True) for i in range(55)])
WITH_GRAD = [i for i, s in enumerate(SPECS) if s[4]]
assert len(WITH_GRAD) > MAX_TENSORS            # one launch's table does not hold them: two launches
SIZE_1, TAIL = 0, 10                           # indices into SPECS: the size-1 tensor, the tensor of three chunks plus 2
LRS = (1e-3, 0.0137, 2.5e-4)                   # a different lr each step


def view(values, off):
    """A device tensor holding `values` at storage offset `off`."""
    base = torch.zeros(len(values) + off, dtype=torch.float32, device=DEV)
    base[off:].copy_(torch.from_numpy(values))
    v = base[off:off + len(values)]
    assert v.storage_offset() == off and v.data_ptr() % 16 == (4 * off) % 16
    return v


def grad_values(step):
    """The gradients of one step, as numpy arrays: seeded normals at three scales with exact zeros."""
    return [R.seeded_values(n, 1000 * (step + 1) + i, scales=(1.0, 1e-4, 1e2)) for i, (n, *_rest) in enumerate(SPECS)]


class Case:
    """The parameter set on the device beside its numpy twin."""

    def __init__(self, seed=0, preset_momentum=False):
        self.p_np = [R.seeded_values(n, seed + i) for i, (n, *_rest) in enumerate(SPECS)]
        self.m_np = [R.seeded_values(n, seed + 500 + i, scales=(1e-2, 1.0, 1e2)) if preset_momentum else np.zeros(n, np.float32)
                     for i, (n, *_rest) in enumerate(SPECS)]
        self.params = [torch.nn.Parameter(view(v, s[1])) for v, s in zip(self.p_np, SPECS)]
        self.holders = [view(np.zeros(s[0], np.float32), s[2]) if s[4] else None for s in SPECS]
        self.preset = [view(m, s[3]) for m, s in zip(self.m_np, SPECS)] if preset_momentum else None

    def preset_into(self, opt):
        for i in WITH_GRAD:
            opt.state[self.params[i]]["momentum_buffer"] = self.preset[i]

    def set_grads(self, values):
        for p, h, v in zip(self.params, self.holders, values):
            if h is not None:
                h.copy_(torch.from_numpy(v))
                p.grad = h

    def numpy_step(self, values, hyper):
        """hyper: index -> (lr, mu, wd)."""
        for i in WITH_GRAD:
            self.p_np[i], self.m_np[i] = R.step_f32(self.p_np[i], values[i], self.m_np[i], *hyper(i))

    def assert_bits(self, opt, what):
        for i, p in enumerate(self.params):
            got = p.detach().cpu().numpy()
            assert np.array_equal(got.view(np.int32), self.p_np[i].view(np.int32)), (what, "parameter", i, SPECS[i])
            if SPECS[i][4]:
                m = opt.state[p]["momentum_buffer"].cpu().numpy()
                assert np.array_equal(m.view(np.int32), self.m_np[i].view(np.int32)), (what, "momentum", i, SPECS[i])
            else:
                assert "momentum_buffer" not in opt.state.get(p, {})


def loss_of(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


# ---- bit-equality --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu,wd", [(0.9, 1e-4), (0.0, 0.0), (0.9, 0.0), (0.0, 1e-4)])
def test_three_steps_bit_equal_to_the_numpy_restatement(mu, wd):
    case = Case()
    opt = GuardedSGD(case.params, lr=LRS[0], momentum=mu, weight_decay=wd, guard="loss")
    for step, lr in enumerate(LRS):
        opt.param_groups[0]["lr"] = lr
        g = grad_values(step)
        case.set_grads(g)
        opt.step(loss_of(0.5))
        case.numpy_step(g, lambda i: (lr, mu, wd))
        case.assert_bits(opt, f"step {step}")
    assert opt.counters() == (3, 0)


def test_two_param_groups_with_their_own_settings():
    case = Case(seed=3)
    cut = 20
    hyp = [(1e-3, 0.9, 1e-4), (0.02, 0.5, 0.0)]
    opt = GuardedSGD([dict(params=case.params[:cut], lr=hyp[0][0], momentum=hyp[0][1], weight_decay=hyp[0][2]),
                      dict(params=case.params[cut:], lr=hyp[1][0], momentum=hyp[1][1], weight_decay=hyp[1][2])], lr=1.0, guard="grads")
    for step in range(3):
        for grp, h in zip(opt.param_groups, hyp):
            grp["lr"] = h[0] * (step + 1)
        g = grad_values(step)
        case.set_grads(g)
        opt.step()
        case.numpy_step(g, lambda i: (hyp[i >= cut][0] * (step + 1), hyp[i >= cut][1], hyp[i >= cut][2]))
        case.assert_bits(opt, f"step {step}")
    assert opt.counters() == (3, 0)                       # one count per step, however many groups and launches


def test_zero_grad_set_to_none_between_steps():
    case = Case(seed=5)
    opt = GuardedSGD(case.params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard=None)
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in case.params)
        g = grad_values(step)
        if step == 1:                                    # the table is read from the tensors at every step: fresh gradient tensors this time
            for i in WITH_GRAD:
                case.params[i].grad = torch.from_numpy(g[i]).to(DEV)
        else:
            case.set_grads(g)
        opt.step()
        case.numpy_step(g, lambda i: (1e-3, 0.9, 1e-4))
        case.assert_bits(opt, f"step {step}")


# ---- torch's SGD on the device ---------------------------------------------------------------------------------------------------------------
def test_one_step_against_torch_sgd_inside_the_bound():
    lr, mu, wd = 1e-3, 0.9, 1e-4
    ours, theirs = Case(seed=7, preset_momentum=True), Case(seed=7, preset_momentum=True)
    g = grad_values(0)
    opt = GuardedSGD(ours.params, lr=lr, momentum=mu, weight_decay=wd, guard="loss")
    ref = torch.optim.SGD(theirs.params, lr=lr, momentum=mu, weight_decay=wd)
    ours.preset_into(opt)
    theirs.preset_into(ref)
    ours.set_grads(g)
    theirs.set_grads(g)
    opt.step(loss_of(1.0))
    ref.step()
    worst = dict(ours_p=0.0, ours_m=0.0, torch_p=0.0, torch_m=0.0, between_p=0.0, between_m=0.0)
    for i in WITH_GRAD:
        p64, m64, err_p, err_m = R.step_f64(ours.p_np[i], g[i], ours.m_np[i], lr, mu, wd)
        a_p, a_m = ours.params[i].detach().cpu().numpy(), opt.state[ours.params[i]]["momentum_buffer"].cpu().numpy()
        b_p, b_m = theirs.params[i].detach().cpu().numpy(), ref.state[theirs.params[i]]["momentum_buffer"].cpu().numpy()
        for key, got, exact, err in (("ours_p", a_p, p64, err_p), ("ours_m", a_m, m64, err_m), ("torch_p", b_p, p64, err_p),
                                     ("torch_m", b_m, m64, err_m), ("between_p", a_p, b_p.astype(np.float64), err_p),
                                     ("between_m", a_m, b_m.astype(np.float64), err_m)):
            worst[key] = max(worst[key], R.worst_fraction(got, exact, err))
    print("\nlargest fraction of the one-step bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst["ours_p"], worst["ours_m"], worst["torch_p"], worst["torch_m"]) <= 1.0, worst
    assert max(worst["between_p"], worst["between_m"]) <= 2.0, worst       # two evaluations, each within the bound of the exact step


# ---- the guard ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_loss_that_is_not_finite_skips_the_step(bad):
    case = Case(seed=9, preset_momentum=True)
    opt = GuardedSGD(case.params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard="loss")
    case.preset_into(opt)
    g = grad_values(0)
    case.set_grads(g)
    opt.step(loss_of(bad))
    case.assert_bits(opt, "skipped")                     # parameters and buffers unchanged bit for bit
    assert opt.counters() == (0, 1)
    opt.step(torch.tensor([0.25], dtype=torch.float32, device=DEV))          # a [1] loss
    case.numpy_step(g, lambda i: (1e-3, 0.9, 1e-4))
    case.assert_bits(opt, "applied")
    assert opt.counters() == (1, 1)


@pytest.mark.parametrize("where", [SIZE_1, TAIL], ids=["size-1", "tail-chunk"])
def test_a_gradient_that_is_not_finite_skips_the_step(where):
    case = Case(seed=11)
    opt = GuardedSGD(case.params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard="grads")
    applied = skipped = 0
    for step, poison in enumerate((float("nan"), None, float("inf"), None, float("-inf"), None)):
        g = grad_values(step)
        if poison is not None:
            g[where][-1] = poison                        # a single value, the last element: of the size-1 tensor / of the tail of three chunks + 2
        case.set_grads(g)
        opt.step(loss_of(1.0))                           # the loss is finite: only the gradient check can stop the step
        if poison is None:
            case.numpy_step(g, lambda i: (1e-3, 0.9, 1e-4))
            applied += 1
        else:
            skipped += 1
        case.assert_bits(opt, f"step {step} ({poison})")  # a clean step after a skipped one is applied: the flag was cleared
        assert opt.counters() == (applied, skipped)
    # guard="grads" honours the loss too
    case.set_grads(grad_values(7))
    opt.step(loss_of(float("nan")))
    case.assert_bits(opt, "nan loss")
    assert opt.counters() == (applied, skipped + 1)


def test_guard_none_applies_whatever_the_loss():
    case = Case(seed=13)
    opt = GuardedSGD(case.params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard=None)
    g = grad_values(0)
    case.set_grads(g)
    opt.step(loss_of(float("nan")))
    case.numpy_step(g, lambda i: (1e-3, 0.9, 1e-4))
    case.assert_bits(opt, "applied")
    assert opt.counters() == (1, 0)


def test_step_arguments():
    case = Case(seed=15)
    opt = GuardedSGD(case.params, lr=1e-3, guard="loss")
    case.set_grads(grad_values(0))
    for loss in (None, 1.0, torch.tensor(1.0), loss_of(1.0).double(), torch.ones(2, device=DEV), torch.ones(1, 1, device=DEV)):
        with pytest.raises(ValueError, match="loss"):
            opt.step(loss)
    with pytest.raises(ValueError, match="closure"):
        opt.step(closure=lambda: 1.0)
    for wrong in (torch.zeros(255, device=DEV, dtype=torch.float64), torch.zeros(254, device=DEV), torch.zeros(510, device=DEV)[::2]):
        opt.state[case.params[4]]["momentum_buffer"] = wrong              # a buffer of another type, size or layout (a loaded state dict)
        with pytest.raises(ValueError, match="parameter 4"):
            opt.step(loss_of(1.0))
    assert opt.counters() == (0, 0)                      # nothing was launched


# ---- no host synchronisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", ["loss", "grads"])
def test_three_steps_without_a_host_synchronisation(guard):
    case = Case(seed=17)
    opt = GuardedSGD(case.params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard=guard)
    grads = [grad_values(s) for s in range(3)]
    staged = [[torch.from_numpy(v).to(DEV) for v in g] for g in grads]
    loss = loss_of(1.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in range(3):
            for p, h, v in zip(case.params, case.holders, staged[step]):
                if h is not None:
                    h.copy_(v)
                    p.grad = h
            opt.step(loss)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for step in range(3):
        case.numpy_step(grads[step], lambda i: (1e-3, 0.9, 1e-4))
    case.assert_bits(opt, guard)
    assert opt.counters() == (3, 0)


# ---- resume ---------------------------------------------------------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    SIZES = (5, 257, CHUNK + 1, 2 * CHUNK)

    def __init__(self, seed):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(R.seeded_values(n, seed + i))) for i, n in enumerate(self.SIZES)])

    def save_weights(self, path):
        torch.save(self.state_dict(), path)

    def load_weights(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))


def run_steps(net, opt, steps):
    for step in steps:
        for i, p in enumerate(net.w):
            p.grad = torch.from_numpy(R.seeded_values(p.numel(), 300 + 10 * step + i)).to(DEV)
        opt.step(loss_of(float("nan") if step == 1 else 1.0))               # step 1 is skipped by the guard: the counters travel too
        opt.param_groups[0]["lr"] *= 0.5


def test_resume_from_a_checkpoint_continues_bit_for_bit(tmp_path):
    straight = Net(0).to(DEV)
    opt_a = GuardedSGD(straight.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    run_steps(straight, opt_a, range(6))
    first = Net(0).to(DEV)
    opt_b = GuardedSGD(first.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    run_steps(first, opt_b, range(3))
    path = checkpoint.save_path("net", 0, 3, str(tmp_path))
    checkpoint.save(path, first, opt_b, 3, 0)
    assert sorted(os.listdir(str(tmp_path))) == ["net_0_3.pth", "net_0_3.pth.state"]
    second = Net(99).to(DEV)                                                 # fresh parameters, a fresh optimizer
    opt_c = GuardedSGD(second.parameters(), lr=123.0, momentum=0.1)
    assert checkpoint.load(path, second, opt_c) == {"iteration": 3, "epoch": 0, "sidecar": True}
    assert opt_c.counters() == (2, 1)
    run_steps(second, opt_c, range(3, 6))
    for a, c in zip(straight.w, second.w):
        assert torch.equal(a, c)
        assert torch.equal(opt_a.state[a]["momentum_buffer"], opt_c.state[c]["momentum_buffer"])
    assert opt_a.counters() == opt_c.counters() == (5, 1)
    assert opt_a.param_groups[0]["lr"] == opt_c.param_groups[0]["lr"]
