"""The optimizer step without a GPU: the two restatements of tests/optim_restate.py against each other and against torch's CPU SGD, the
package-private binding of csrc/optim.h, the refusals of the two entry points (NULL pointers: nothing is launched), GuardedSGD on CPU parameters,
and the compiler's resource report for csrc/optim.hip."""
import ctypes

import numpy as np
import pytest
import torch

import optim_restate as R
from kernel_resources import kernel_resources
from stmask_amd import _lib, optim
from stmask_amd._lib import StmError
from stmask_amd.optim import GuardedSGD

SCALES = [(1.0, 1.0, 1.0), (1e-3, 1.0, 1e3), (1e3, 1e-3, 1.0), (1e-6, 1e-6, 1e-6), (1e4, 1e4, 1e4)]     # of p, g, m
HYPER = [(1e-3, 0.9, 1e-4), (0.0137, 0.9, 0.0), (1e-3, 0.0, 1e-4), (0.3, 0.0, 0.0)]


def triple(n, seed, scales):
    return [R.seeded_values(n, seed + i) * np.float32(s) for i, s in enumerate(scales)]


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("lr,mu,wd", HYPER)
def test_restatements_and_torch_cpu_inside_the_bound(scales, lr, mu, wd):
    p, g, m = triple(4099, 11, scales)
    p32, m32 = R.step_f32(p, g, m, lr, mu, wd)
    p64, m64, err_p, err_m = R.step_f64(p, g, m, lr, mu, wd)
    fp, fm = R.worst_fraction(p32, p64, err_p), R.worst_fraction(m32, m64, err_m)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = torch.optim.SGD([tp], lr=lr, momentum=mu, weight_decay=wd)
    if mu:
        opt.state[tp]["momentum_buffer"] = torch.from_numpy(m.copy())
        opt.step()
        tm = opt.state[tp]["momentum_buffer"].numpy()
        tfm = R.worst_fraction(tm, m64, err_m)
    else:                                   # torch keeps no buffer at momentum 0: the step uses g' itself, which is mu * m + g' at mu = 0
        opt.step()
        tfm = 0.0
    tfp = R.worst_fraction(tp.detach().numpy(), p64, err_p)
    print(f"\nscales {scales} lr {lr} mu {mu} wd {wd}: fraction of the bound  numpy p {fp:.3f} m {fm:.3f}   torch cpu p {tfp:.3f} m {tfm:.3f}")
    assert max(fp, fm, tfp, tfm) <= 1.0


def test_first_step_from_a_zero_buffer_is_torchs_first_step():
    """torch clones the gradient into a fresh buffer; mu * 0 + g' is g' exactly, so starting from zeros gives the same buffer, bit for bit."""
    p, g, _ = triple(1031, 5, (1.0, 1.0, 1.0))
    lr, mu, wd = 1e-3, 0.9, 1e-4
    p32, m32 = R.step_f32(p, g, np.zeros_like(p), lr, mu, wd)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = torch.optim.SGD([tp], lr=lr, momentum=mu, weight_decay=wd)
    opt.step()
    p64, m64, err_p, err_m = R.step_f64(p, g, np.zeros_like(p), lr, mu, wd)
    tm = opt.state[tp]["momentum_buffer"].numpy()
    assert R.worst_fraction(tm, m64, err_m) <= 1.0 and R.worst_fraction(tp.detach().numpy(), p64, err_p) <= 1.0
    assert R.worst_fraction(m32, m64, err_m) <= 1.0 and R.worst_fraction(p32, p64, err_p) <= 1.0
    g1 = g + np.float32(wd) * p
    assert np.array_equal(m32.view(np.int32), g1.view(np.int32))          # mu * 0 + g' == g'


def test_fp64_hyper_parameters_alone_take_a_share_of_the_bound():
    """Why step_f64 rounds lr, mu and wd to fp32 first."""
    p, g, m = triple(4099, 11, (1.0, 1.0, 1.0))
    lr, mu, wd = 1e-3, 0.9, 1e-4
    p64, m64, err_p, err_m = R.step_f64(p, g, m, lr, mu, wd)
    pd, gd, md = p.astype(np.float64), g.astype(np.float64), m.astype(np.float64)
    m_exact = mu * md + (gd + wd * pd)
    frac = np.abs(m_exact - m64)[err_m > 0] / err_m[err_m > 0]
    print(f"\nfp64 mu and wd against their fp32 roundings: up to {frac.max():.3f} of err_m")
    assert frac.max() > 0.1


# ---- the private binding ------------------------------------------------------------------------------------------------------------------
def test_private_call_checks_the_argument_count_and_types():
    with pytest.raises(StmError, match="takes 13 arguments, got 2"):
        _lib.private_call("stm_sgd_step_multi_f32", None, None)
    with pytest.raises(StmError, match="takes 6 arguments, got 7"):
        _lib.private_call("stm_grads_nonfinite_multi_f32", None, None, 1, None, 0, None, None)
    with pytest.raises(ctypes.ArgumentError):
        _lib.private_call("stm_grads_nonfinite_multi_f32", None, None, 1.5, None, 0, None)


def test_private_call_names_a_missing_entry(monkeypatch):
    monkeypatch.setitem(_lib.PRIVATE_SIGNATURES, "stm_not_built_f32", ("i", "p"))
    with pytest.raises(StmError, match=r"lacks stm_not_built_f32: rebuild with .*build\(\)"):
        _lib.private_call("stm_not_built_f32", None)


# ---- refusals: decided from the arguments, before any launch -----------------------------------------------------------------------------------
def ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def counts(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


FAKE = 0x1000   # never dereferenced: every case below is refused first
EINVAL, EUNSUPPORTED = -1, -5


def step_args(**kw):
    a = dict(p=ptrs(FAKE), g=ptrs(FAKE), m=ptrs(FAKE), n=counts(8), count=1, loss=None, bad=None, counters=ctypes.c_void_p(FAKE), first=1,
             lr=1e-3, mu=0.9, wd=1e-4, stream=None)
    a.update(kw)
    return [a[k] for k in ("p", "g", "m", "n", "count", "loss", "bad", "counters", "first", "lr", "mu", "wd", "stream")]


many = optim.MAX_TENSORS + 1
STEP_REFUSALS = [
    (dict(count=0), EINVAL, "count=0"),
    (dict(count=-3), EINVAL, "count=-3"),
    (dict(count=many, p=ptrs(*[FAKE] * many), g=ptrs(*[FAKE] * many), m=ptrs(*[FAKE] * many), n=counts(*[1] * many)), EUNSUPPORTED,
     f"at most {optim.MAX_TENSORS} tensors"),
    (dict(n=counts(-1)), EINVAL, "tensor 0 has n=-1"),
    (dict(p=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL p"),
    (dict(g=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL g"),
    (dict(m=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL m"),
    (dict(count=2, p=ptrs(FAKE, None), g=ptrs(FAKE, FAKE), m=ptrs(FAKE, FAKE), n=counts(0, 5)), EINVAL, "tensor 1 has 5 elements and a NULL p"),
    (dict(p=None), EINVAL, "arrays of pointers"),
    (dict(n=None), EINVAL, "arrays of pointers"),
    (dict(lr=float("nan")), EINVAL, "must be finite"),
    (dict(lr=float("inf")), EINVAL, "must be finite"),
    (dict(mu=float("-inf")), EINVAL, "must be finite"),
    (dict(wd=float("nan")), EINVAL, "must be finite"),
    (dict(counters=None), EINVAL, "counters must be non-NULL"),
]


@pytest.mark.parametrize("change,code,text", STEP_REFUSALS, ids=[f"{i}-{t[2][:24].replace(' ', '_')}" for i, t in enumerate(STEP_REFUSALS)])
def test_sgd_step_refusals(change, code, text):
    with pytest.raises(StmError) as e:
        _lib.private_call("stm_sgd_step_multi_f32", *step_args(**change))
    assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)


GRAD_REFUSALS = [
    (dict(count=0), EINVAL, "count=0"),
    (dict(count=many, g=ptrs(*[FAKE] * many), n=counts(*[1] * many)), EUNSUPPORTED, f"at most {optim.MAX_TENSORS} tensors"),
    (dict(n=counts(-7)), EINVAL, "tensor 0 has n=-7"),
    (dict(g=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL g"),
    (dict(g=None), EINVAL, "arrays of pointers"),
    (dict(bad=None), EINVAL, "bad must be non-NULL"),
]


@pytest.mark.parametrize("change,code,text", GRAD_REFUSALS, ids=[f"{i}-{t[2][:24].replace(' ', '_')}" for i, t in enumerate(GRAD_REFUSALS)])
def test_grads_nonfinite_refusals(change, code, text):
    a = dict(g=ptrs(FAKE), n=counts(8), count=1, bad=ctypes.c_void_p(FAKE), first=1, stream=None)
    a.update(change)
    with pytest.raises(StmError) as e:
        _lib.private_call("stm_grads_nonfinite_multi_f32", *[a[k] for k in ("g", "n", "count", "bad", "first", "stream")])
    assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)


# ---- GuardedSGD on CPU parameters -------------------------------------------------------------------------------------------------------------
def cpu_params(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 1, 3))]


def test_step_on_cpu_parameters_raises():
    params = cpu_params()
    opt = GuardedSGD(params, lr=1e-3)
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(StmError, match="no CPU fallback"):
        opt.step(torch.tensor(1.0))
    with pytest.raises(ValueError, match="closure"):
        opt.step(closure=lambda: 0.0)
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)


def test_constructor_refusals():
    p = cpu_params()
    with pytest.raises(ValueError, match="guard="):
        GuardedSGD(p, lr=1e-3, guard="always")
    with pytest.raises(ValueError, match="lr="):
        GuardedSGD(p, lr=float("nan"))
    with pytest.raises(ValueError, match="momentum="):
        GuardedSGD(p, lr=1e-3, momentum=-0.1)
    with pytest.raises(ValueError, match="parameter 1 is torch.float64"):
        GuardedSGD([p[0], torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(ValueError, match="parameter 1 .*not dense"):
        GuardedSGD([p[0], torch.nn.Parameter(torch.zeros(4, 6)[:, ::2])], lr=1e-3)
    GuardedSGD([torch.nn.Parameter(torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))], lr=1e-3)     # dense in another order


def test_state_dict_goes_to_torch_sgd_and_back():
    params = cpu_params()
    ref = torch.optim.SGD(params, lr=0.02, momentum=0.8, weight_decay=3e-4)
    for p in params[:2]:                     # the third parameter gets no gradient: no buffer in torch's state
        p.grad = torch.randn_like(p)
    ref.step()
    ours = GuardedSGD(cpu_params(1), lr=1e-3)
    ours.load_state_dict(ref.state_dict())
    g = ours.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.02, 0.8, 3e-4)
    own = ours._all_params()
    for i in range(2):
        assert torch.equal(ours.state[own[i]]["momentum_buffer"], ref.state[params[i]]["momentum_buffer"])
    assert "momentum_buffer" not in ours.state.get(own[2], {})             # missing: zeros at the next step
    sd = ours.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1] and list(sd["state"][0]) == ["momentum_buffer"]
    assert set(ref.state_dict()["param_groups"][0]) >= set(sd["param_groups"][0]) >= {"lr", "momentum", "dampening", "weight_decay", "nesterov", "params"}
    back = torch.optim.SGD(cpu_params(2), lr=0.5)
    back.load_state_dict(sd)
    assert back.param_groups[0]["lr"] == 0.02 and back.param_groups[0]["dampening"] == 0 and back.param_groups[0]["nesterov"] is False
    bp = back.param_groups[0]["params"]
    for i in range(2):
        assert torch.equal(back.state[bp[i]]["momentum_buffer"], ref.state[params[i]]["momentum_buffer"])
    for p in bp:
        p.grad = torch.ones_like(p)
    back.step()                                                            # torch runs on the loaded state


def test_load_state_dict_none_buffers_unknown_keys_and_refusals():
    params = cpu_params()
    ref = torch.optim.SGD(params, lr=0.02, momentum=0.0)
    for p in params:
        p.grad = torch.randn_like(p)
    ref.step()                                                             # momentum 0: torch's state holds momentum_buffer None
    sd = ref.state_dict()
    assert all(v["momentum_buffer"] is None for v in sd["state"].values())
    sd["param_groups"][0]["some_future_key"] = 7
    ours = GuardedSGD(cpu_params(1), lr=1e-3)
    ours.load_state_dict(sd)
    assert "some_future_key" not in ours.param_groups[0] and ours.param_groups[0]["momentum"] == 0.0
    assert all("momentum_buffer" not in ours.state.get(p, {}) for p in ours._all_params())
    for key, value in (("dampening", 0.1), ("nesterov", True), ("maximize", True)):
        bad = ref.state_dict()
        bad["param_groups"][0][key] = value
        with pytest.raises(ValueError, match=key):
            ours.load_state_dict(bad)


# ---- the kernels' resources --------------------------------------------------------------------------------------------------------------------
def test_optim_kernels_use_no_scratch_and_no_lds():
    seen = []
    for name, r in kernel_resources("optim.hip").items():
        if "sgd_step_multi_kernel" in name or "grads_nonfinite_multi_kernel" in name:
            seen.append(name)
            assert r.scratch == 0 and r.lds == 0, (name, r.scratch, r.lds)
    assert len(seen) == 2, seen
