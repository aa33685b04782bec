"""The finish of a data-parallel step (dp_sgd_finish_multi_kernel of csrc/optim.hip) restated in numpy float32, one rounding per operation, in the kernel's order:

    g = s * inv_world;   g' = g + wd * p;   m' = mu * m + g';   p' = p - lr * m'

with s the sum of the ranks' gradients and inv_world the fp32 value of 1 / world.  With world == 1, s * 1.0f is s itself, so the finish is
optim_restate.step_f32 bit for bit (tests/test_parallel_cpu.py pins that).  Also the shared argument lists of the refusal tests and a small
worker for the two-process gloo tests.  Not a test module."""
import ctypes

import numpy as np

import optim_restate as R


def inv_world(world):
    return np.float32(1.0) / np.float32(world)


def finish_f32(p, s, m, world, lr, mu, wd):
    """-> (p', m', g after the launch) as float32 arrays; p, s, m float32 arrays of one shape."""
    assert p.dtype == s.dtype == m.dtype == np.float32
    with np.errstate(all="ignore"):
        g = s * inv_world(world)
    assert g.dtype == np.float32
    p1, m1 = R.step_f32(p, g, m, lr, mu, wd)
    return p1, m1, np.zeros_like(s)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- refusals of stm_dp_sgd_finish_multi_f32: decided from the arguments, before any launch -----------------------------------------------------
def ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def counts(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


FAKE = 0x1000   # never dereferenced: every case below is refused first
EINVAL, EUNSUPPORTED = -1, -5
MANY = 65


def finish_args(**kw):
    a = dict(p=ptrs(FAKE), g=ptrs(FAKE), m=ptrs(FAKE), n=counts(8), count=1, loss=None, bad=None, counters=ctypes.c_void_p(FAKE), first=1,
             inv_world=0.5, lr=1e-3, mu=0.9, wd=1e-4, stream=None)
    a.update(kw)
    return [a[k] for k in ("p", "g", "m", "n", "count", "loss", "bad", "counters", "first", "inv_world", "lr", "mu", "wd", "stream")]


FINISH_REFUSALS = [
    (dict(count=0), EINVAL, "count=0"),
    (dict(count=-3), EINVAL, "count=-3"),
    (dict(count=MANY, p=ptrs(*[FAKE] * MANY), g=ptrs(*[FAKE] * MANY), m=ptrs(*[FAKE] * MANY), n=counts(*[1] * MANY)), EUNSUPPORTED,
     "at most 64 tensors"),
    (dict(n=counts(-1)), EINVAL, "tensor 0 has n=-1"),
    (dict(p=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL p"),
    (dict(g=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL g"),
    (dict(m=ptrs(None)), EINVAL, "tensor 0 has 8 elements and a NULL m"),
    (dict(count=2, p=ptrs(FAKE, None), g=ptrs(FAKE, FAKE), m=ptrs(FAKE, FAKE), n=counts(0, 5)), EINVAL, "tensor 1 has 5 elements and a NULL p"),
    (dict(p=None), EINVAL, "arrays of pointers"),
    (dict(g=None), EINVAL, "arrays of pointers"),
    (dict(n=None), EINVAL, "arrays of pointers"),
    (dict(n=counts((1 << 31) * 4096)), EUNSUPPORTED, "2^31 chunks"),
    (dict(lr=float("nan")), EINVAL, "must be finite"),
    (dict(mu=float("-inf")), EINVAL, "must be finite"),
    (dict(wd=float("inf")), EINVAL, "must be finite"),
    (dict(inv_world=0.0), EINVAL, "inv_world"),
    (dict(inv_world=1.5), EINVAL, "inv_world"),
    (dict(inv_world=float("nan")), EINVAL, "inv_world"),
    (dict(counters=None), EINVAL, "counters must be non-NULL"),
]
REFUSAL_IDS = [f"{i}-{t[2][:24].replace(' ', '_')}" for i, t in enumerate(FINISH_REFUSALS)]
