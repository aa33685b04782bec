"""numpy restatement of TemporalNet's pooled tail: the 32.32 fixed-point pool words stm_conv2d_planar_windows_pool_f32 accumulates (csrc/conv_bf16x.hip,
pooled_epilogue), the mean and the stacked linear layers of stm_temporal_pool_fc_f32 (csrc/temporal.hip), the bound the fp32 tail is held to, and the
seeded cases tests/test_temporal_tail_cpu.py and tests/test_gpu_temporal_tail.py share."""
import functools
import math

import numpy as np

EPS = 2.0 ** -24
TWO32 = 4294967296.0
SENTINEL = 0x5A5AA5A5C3C33C3C          # the rows past n of every pool buffer hold SENTINEL + element index: they must come back unchanged
BIG = 3200000000 << 32                  # a sum of 3.2e9: >= 2^63 as a word, so negative when the int64 tensor is read as signed


def fixed_sum(values_f32):
    """The pool word of ONE piece (the pixels of one image that one wave meets in a row): values [k, ...] are added along axis 0 in fp32, in order, and
    the sum s becomes hi = uint32(trunc(s)), lo = uint32((s - hi) * 2^32) (fp32 arithmetic: both steps are exact, the conversion of lo truncates what lies
    below 2^-32), word = hi << 32 | lo.  Returns uint64 [...].  (Defined for 0 <= s < 2^32, the range the kernel's guard admits.)"""
    v = np.asarray(values_f32, dtype=np.float32)
    s = np.zeros(v.shape[1:], dtype=np.float32)
    for row in v:
        s = (s + row).astype(np.float32)
    hi = np.trunc(s).astype(np.float32)
    lo = ((s - hi).astype(np.float32) * np.float32(TWO32)).astype(np.float32)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def range_flagged(values_f32):
    """The guard of pooled_epilogue on one piece, !(s < 4e9f): True for a sum at or beyond 4e9 and for NaN."""
    v = np.asarray(values_f32, dtype=np.float32)
    s = np.zeros(v.shape[1:], dtype=np.float32)
    for row in v:
        s = (s + row).astype(np.float32)
    return ~(s < np.float32(4.0e9))


def fixed_to_float64(pool_u64):
    """The value of a pool word, hi + lo / 2^32, in fp64 (exact for words of at most 53 significant bits)."""
    u = np.asarray(pool_u64, dtype=np.uint64)
    return (u >> np.uint64(32)).astype(np.float64) + (u & np.uint64(0xFFFFFFFF)).astype(np.float64) / TWO32


def mean_of(pool_u64, npix):
    """float32(float64(u) * (1 / (2^32 npix))): the tail kernel's mean.  uint64 -> double rounds to nearest on the host as on the device, the product and
    the conversion to fp32 are IEEE operations: the device's pooled_out must equal this bit for bit."""
    u = np.asarray(pool_u64, dtype=np.uint64)
    return (u.astype(np.float64) * (1.0 / (TWO32 * float(npix)))).astype(np.float32)


def tail_fp64(mean_f32, w, bias):
    """(y, S): y = mean w^T + bias in fp64 and S = sum_k |mean_k w_ok| + |bias_o|, both [n, n_out]."""
    m, w64 = np.asarray(mean_f32, dtype=np.float64), np.asarray(w, dtype=np.float64)
    y, S = m @ w64.T, np.abs(m) @ np.abs(w64).T
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        y, S = y + b, S + np.abs(b)
    return y, S


def tail_bound(S, C):
    """|fp32 tail - fp64| <= (ceil(C / 64) + 8) 2^-24 S (1 + 2^-20).  From stm_wave_sum (csrc/stm_common.h) and temporal_pool_fc_kernel: a lane's fmaf chain
    over k = lane, lane + 64, ... has ceil(C / 64) roundings, the 16-lane row sum four DPP levels, the four row totals three additions, the bias one: every
    term passes through at most ceil(C / 64) + 8 roundings of partial sums that are bounded by S; (1 + 2^-20) covers the second-order terms
    ((1 + 2^-24)^40 - 1 < 40 * 2^-24 * (1 + 2^-20))."""
    return (math.ceil(C / 64) + 8) * EPS * S * (1.0 + 2.0 ** -20)


# ---- stm_temporal_pool_fc_f32 on synthetic pools: (n, C, n_out, n_first, npix, bias, clear)
TAIL_CASES = {
    "smallest_one_block": (1, 64, 1, None, 1, True, True),
    "model_test_shape": (8, 256, 36, 4, 49, True, True),
    "network_c_second_group_of_one": (9, 1024, 36, 4, 49, True, True),          # the sweep runs four times, the weight loop twice; last workgroup nr = 1
    "ragged_c_and_outputs": (13, 200, 7, 3, 45, True, True),                    # C no multiple of 64, n_out no multiple of 4
    "one_lane_two_terms_no_bias": (5, 65, 6, 2, 49, False, True),
    "second_round_one_element_no_clear": (4, 513, 5, None, 49, True, False),    # k0 = 512 has one live element
    "lds_limit": (5, 2048, 6, 2, 49, True, True),                               # 8 * 2048 * 4 B = 64 KB of dynamic LDS
}
SPARE_ROWS = 3


@functools.lru_cache(maxsize=None)
def draw_tail_case(name):
    """pool uint64 [n + 3, C]: sums below 2^12 with full 32-bit fractions; row 1 all zero and row n - 1 holding BIG (even columns exactly, odd columns with a
    random fraction) where n allows -- for n = 1 columns 0 / 1 of the only row; the three spare rows hold SENTINEL + index.  w [n_out, C], bias [n_out] or
    None, fp32."""
    n, C, n_out, n_first, npix, with_bias, clear = TAIL_CASES[name]
    g = np.random.default_rng(81000 + 131 * list(TAIL_CASES).index(name))
    hi = g.integers(0, 1 << 12, size=(n + SPARE_ROWS, C), dtype=np.uint64)
    lo = g.integers(0, 1 << 32, size=(n + SPARE_ROWS, C), dtype=np.uint64)
    pool = (hi << np.uint64(32)) | lo
    big = np.full(C, BIG, dtype=np.uint64)
    big[1::2] |= lo[0, 1::2]
    if n >= 3:
        pool[1] = 0
    if n >= 2:
        pool[n - 1] = big
    else:
        pool[0, 0], pool[0, 1] = 0, BIG
    pool[n:] = (np.uint64(SENTINEL) + np.arange(SPARE_ROWS * C, dtype=np.uint64)).reshape(SPARE_ROWS, C)
    w = (g.standard_normal((n_out, C)) * C ** -0.5).astype(np.float32)
    bias = g.standard_normal(n_out).astype(np.float32) if with_bias else None
    for a in (pool, w) + ((bias,) if with_bias else ()):
        a.setflags(write=False)
    return dict(pool=pool, w=w, bias=bias, n=n, C=C, n_out=n_out, n_first=n_first, npix=npix, clear=clear)


# ---- stm_conv2d_planar_windows_pool_f32 on maps other than the model's: (h, w, n, Cout), C = 64
POOL_C = 64
POOL_GEOMS = {
    "7x7_n37_o128": (7, 7, 37, 128),
    "5x9_n37_o384": (5, 9, 37, 384),            # three 128-column tiles
    "3x3_n101_o128": (3, 3, 101, 128),          # a 1-pixel interior class
    "7x7_n3_o384": (7, 7, 3, 384),              # fewer rows than one tile
}


@functools.lru_cache(maxsize=None)
def draw_pool_case(name):
    """x [n, h, w, 64] NHWC, weight [Cout, 64, 3, 3] scaled to unit output variance, bias [Cout]; fp32."""
    h, w, n, O = POOL_GEOMS[name]
    g = np.random.default_rng(82000 + 173 * list(POOL_GEOMS).index(name))
    x = g.standard_normal((n, h, w, POOL_C)).astype(np.float32)
    wt = (g.standard_normal((O, POOL_C, 3, 3)) * (POOL_C * 9) ** -0.5).astype(np.float32)
    b = g.standard_normal(O).astype(np.float32)
    for a in (x, wt, b):
        a.setflags(write=False)
    return dict(x=x, w=wt, b=b, h=h, wd=w, n=n, O=O)


def pool_bound(mag_sum, abs_sum, npix):
    """|pool word / 2^32 - fp64 sum over the image| per (image, channel): 2e-6 * mag_sum -- the per-pixel bound of the planar convolution
    (test_conv_window_launches_equal_the_padded_convolution), mag the convolution of |x|, |w|, |b|, summed over the image -- plus npix 2^-24 sum |v| for any
    fp32 order of adding the pixels inside the pieces, plus npix 2^-32: one truncation per piece, at most npix pieces."""
    return 2e-6 * mag_sum + npix * EPS * abs_sum + npix * 2.0 ** -32


# ---- the top of the fixed-point range: 7x7 map, x = 32768 in 128 channels, one centre tap -> every pixel is 128 * 32768 * tap
RANGE_HW, RANGE_N, RANGE_C, RANGE_O, RANGE_X = 7, 2, 128, 128, 32768.0
RANGE_PIECES = (1, 5, 1, 5, 25, 5, 1, 5, 1)          # pixels of the nine border classes of a 7x7 map: an image reaches the pool in (at least) these pieces


def range_pixel(tap):
    return np.float32(RANGE_C * RANGE_X * tap)


# With uniform pixels no single piece of a 7x7 image passes 2^31 before the total passes 2^32 (the largest piece is 25 / 49 of it), so the conversion of
# ONE piece above 2^31 gets a case of its own: x = 32768 on the 25 interior pixels only, 0 on the border, centre tap 24 -> one piece of 25 * 24 * 2^22.
RANGE_INTERIOR_TAP = 24.0
