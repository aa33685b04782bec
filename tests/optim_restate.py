"""The SGD step of csrc/optim.hip restated twice, and the bound that ties any fp32 evaluation of it to the exact one.

    g' = g + wd * p;   m' = mu * m + g';   p' = p - lr * m'

step_f32: numpy float32, one rounding per operation, in exactly this order -- the kernel (compiled without contraction) is bit-equal to it.
step_f64: float64, with lr, mu and wd taken as their fp32 roundings (the kernel's arguments are floats; with the Python doubles instead, the
          rounding of the hyper-parameters alone takes a share of the bound below that its derivation does not grant: 0.22 of err_m at unit
          scale, tests/test_optim_cpu.py prints it).
bound:    with u = 2^-24, for ANY fp32 evaluation, fused or not (a fused multiply-add rounds once where the unfused form rounds twice, so its error is
          covered by the same terms):
              err_g = u (|wd p| + |g'|)
              err_m = err_g + u (|mu m| + |m'|)
              err_p = lr err_m + u (|lr m'| + |p'|)
          each times 1 + 1e-6 for the second-order terms; no other margin.  The magnitudes are those of the float64 evaluation.
"""
import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 1e-6


def f32(x):
    return np.float32(x)


def step_f32(p, g, m, lr, mu, wd):
    """-> (p', m') as float32 arrays; p, g, m float32 arrays of one shape."""
    assert p.dtype == g.dtype == m.dtype == np.float32
    lr, mu, wd = f32(lr), f32(mu), f32(wd)
    with np.errstate(all="ignore"):
        g1 = g + wd * p
        m1 = mu * m + g1
        p1 = p - lr * m1
    assert p1.dtype == m1.dtype == np.float32
    return p1, m1


def step_f64(p, g, m, lr, mu, wd):
    """-> (p', m', err_p, err_m) in float64: the exact step of the fp32 inputs and fp32-rounded hyper-parameters, and the one-step bounds."""
    lr, mu, wd = float(f32(lr)), float(f32(mu)), float(f32(wd))
    p, g, m = p.astype(np.float64), g.astype(np.float64), m.astype(np.float64)
    g1 = g + wd * p
    m1 = mu * m + g1
    p1 = p - lr * m1
    err_g = U * (np.abs(wd * p) + np.abs(g1))
    err_m = err_g + U * (np.abs(mu * m) + np.abs(m1))
    err_p = lr * err_m + U * (np.abs(lr * m1) + np.abs(p1))
    return p1, m1, err_p * SECOND_ORDER, err_m * SECOND_ORDER


def worst_fraction(got, exact, err):
    """max |got - exact| / err over the elements with err > 0; an element with err == 0 must be exact."""
    diff = np.abs(got.astype(np.float64) - exact)
    zero = err == 0
    assert not np.any(diff[zero] != 0)
    return float(np.max(diff[~zero] / err[~zero])) if np.any(~zero) else 0.0


def seeded_values(n, seed, scales=(1.0, 1e-3, 1e3)):
    """n float32 normals, the scales cycling over thirds of the array, every 7th element (from index seed % 7 on) an exact zero."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    s = np.asarray(scales, dtype=np.float32)[(np.arange(n) * len(scales)) // max(n, 1)]
    v = v * s
    v[seed % 7::7] = 0.0
    return v
