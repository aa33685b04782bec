"""fuse._fold restated in numpy float32, one rounding per operation, in its order:

    s = gamma / sqrt(var + eps)        (eps as its fp32 rounding: torch adds a Python scalar to a float32 tensor in float32)
    w' = w * s[channel]                b' = (b - mean) * s + beta        (b = 0 for a convolution without bias)

IEEE add, subtract, multiply, divide and sqrt are correctly rounded in numpy as in torch's CPU kernels and in csrc/fold.hip (compiled without
contraction, sqrt and division through the correctly rounded intrinsics), so all three agree bit for bit; tests/test_validate_cpu.py holds this
file to torch, tests/test_gpu_fold.py holds the kernel to this file.  A NaN that enters passes through every operation with its payload, so the
bits agree there too as long as one operand of an operation is a NaN at most (two NaN operands: which payload wins is the processor's choice).
"""
import numpy as np


def scale(gamma, var, eps):
    assert gamma.dtype == var.dtype == np.float32
    with np.errstate(all="ignore"):
        return gamma / np.sqrt(var + np.float32(eps))


def fold_weight(w, gamma, var, eps):
    """w [O, ...] float32 -> w * s, s broadcast over everything but the first dimension."""
    assert w.dtype == np.float32
    s = scale(gamma, var, eps)
    with np.errstate(all="ignore"):
        return w * s.reshape((-1,) + (1,) * (w.ndim - 1))


def fold_bias(b, gamma, beta, mean, var, eps):
    """b [O] float32 or None (a convolution without bias) -> (b - mean) * s + beta."""
    s = scale(gamma, var, eps)
    old = np.zeros_like(mean) if b is None else b
    with np.errstate(all="ignore"):
        d = old - mean
        p = d * s
        return p + beta


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def seeded_bn(channels, seed, zero_var=True, negative_gamma=True, nonfinite=False):
    """(gamma, beta, mean, var) float32 [channels]: seeded values with, where there is room, a running_var of 0, a negative gamma and -- nonfinite
    -- a variance of +inf and one of NaN (single NaN operands: see the module docstring)."""
    g = np.random.default_rng(seed)
    gamma = g.normal(1.0, 0.5, channels).astype(np.float32)
    beta = g.normal(0.0, 0.3, channels).astype(np.float32)
    mean = g.normal(0.0, 1.0, channels).astype(np.float32)
    var = (g.random(channels) * 2 + 1e-3).astype(np.float32)
    if zero_var:
        var[0] = 0.0
    if negative_gamma:
        gamma[-1] = -abs(gamma[-1]) - 0.25
    if nonfinite and channels >= 3:
        var[1] = np.inf
        var[2] = np.nan
    return gamma, beta, mean, var
