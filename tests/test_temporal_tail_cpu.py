"""tests/temporal_tail_restate.py, the yardstick of tests/test_gpu_temporal_tail.py, on the CPU: the 32.32 encoding round-trips and is additive, the bound of
the fp32 tail already holds a plain fp32 matmul, and the values the range-flag test expects on the device, worked out here first."""
import math

import numpy as np
import pytest

import temporal_tail_restate as T


def word(hi, lo=0):
    return (int(hi) << 32) | int(lo)


def test_case_tables():
    assert [v for v in T.TAIL_CASES.values()] == [(1, 64, 1, None, 1, True, True), (8, 256, 36, 4, 49, True, True), (9, 1024, 36, 4, 49, True, True),
                                                  (13, 200, 7, 3, 45, True, True), (5, 65, 6, 2, 49, False, True), (4, 513, 5, None, 49, True, False),
                                                  (5, 2048, 6, 2, 49, True, True)]
    assert list(T.POOL_GEOMS.values()) == [(7, 7, 37, 128), (5, 9, 37, 384), (3, 3, 101, 128), (7, 7, 3, 384)]
    for name, (n, C, n_out, n_first, npix, with_bias, clear) in T.TAIL_CASES.items():
        c = T.draw_tail_case(name)
        pool = c["pool"]
        assert pool.shape == (n + 3, C) and pool.dtype == np.uint64 and c["w"].shape == (n_out, C) and (c["bias"] is None) == (not with_bias)
        assert (pool.view(np.int64) < 0).any() and (pool == T.BIG).any() and (pool == 0).any()          # the word that is negative as int64; a zero
        assert int(pool[n, 0]) == T.SENTINEL and int(pool[-1, -1]) == T.SENTINEL + 3 * C - 1
        if n >= 3:
            assert not pool[1].any() and ((pool[n - 1] >> np.uint64(32)) == 3200000000).all() and (pool[n - 1] & np.uint64(0xFFFFFFFF)).any()
        rnd = pool[0] if n >= 2 else pool[0, 2:]
        assert int((rnd >> np.uint64(32)).max()) < 1 << 12 and len(set((rnd & np.uint64(0xFFFFFFFF)).tolist())) > len(rnd) // 2
        assert T.draw_tail_case(name)["pool"] is pool                                                    # drawn once, shared, read-only
        with pytest.raises(ValueError):
            pool[0, 0] = 1


def test_encoding_round_trips():
    g = np.random.default_rng(1)
    # one value per piece: integers, fractions on the 2^-32 grid, the top of the range
    v = np.concatenate([g.integers(0, 1 << 24, 200).astype(np.float32), g.random(200, dtype=np.float32) * np.float32(4096.0),
                        np.float32([0.0, 1.0, 2.0 ** -32, 1.0 - 2.0 ** -24, 2.0 ** 31, 49 * 2.0 ** 26, 4.0e9 - 256, 2.0 ** 32 - 256])])
    w = T.fixed_sum(v[None])
    assert w.dtype == np.uint64 and w.shape == v.shape
    assert np.array_equal(T.fixed_to_float64(w), v.astype(np.float64))               # every one of them lies on the 2^-32 grid: nothing is lost
    assert int(T.fixed_sum(np.float32([[2.0 ** 31]]))[0]) == word(1 << 31)           # (unsigned) conversion: no sign to trip over
    assert int(T.fixed_sum(np.float32([[49 * 2.0 ** 26]]))[0]) == word(49 << 26)
    assert int(T.fixed_sum(np.float32([[1.5]]))[0]) == word(1, 1 << 31)
    # below the grid the conversion truncates, by less than 2^-32
    tiny = np.float32([2.0 ** -33, 3 * 2.0 ** -34, 2.0 ** -32 + 2.0 ** -40])
    assert T.fixed_sum(tiny[None]).tolist() == [0, 0, 1]
    assert np.array_equal(T.mean_of(w, 1), v)                                        # npix = 1: the mean of a one-piece pool is the value itself
    assert float(T.mean_of(np.uint64([word(49 << 26)]), 49)[0]) == 2.0 ** 26
    assert float(T.mean_of(np.uint64([T.BIG]), 1)[0]) == 3.2e9 and float(T.mean_of(np.uint64([0]), 49)[0]) == 0.0


def test_encoding_is_additive_and_exact():
    """Values with at most 24 significant bits above 2^-32 -- every fp32 at or above 2^-8 -- are encoded exactly, so the integer sum of the words of any
    split into pieces is the exact sum of the values, whatever the split; the fp32 sum of the same values is not."""
    g = np.random.default_rng(2)
    vals = (g.random((49, 64), dtype=np.float32) * np.float32(100.0) + np.float32(2.0 ** -8)).astype(np.float32)
    exact = vals.astype(np.float64).sum(0)
    singles = T.fixed_sum(vals[None])                                       # 49 pieces of one value each
    assert np.array_equal(T.fixed_to_float64(singles), vals.astype(np.float64))
    total = singles.sum(0, dtype=np.uint64)
    assert np.array_equal(T.fixed_to_float64(total), exact)
    assert (np.abs(vals.sum(0, dtype=np.float32).astype(np.float64) - exact) > 0).any()
    # pieces of several values: each piece is an fp32 sum (rounded), the pieces then add exactly
    cuts = np.cumsum((0,) + T.RANGE_PIECES)
    pieces = [T.fixed_sum(vals[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    tot = np.sum(pieces, axis=0, dtype=np.uint64)
    piece_sums = [T.fixed_to_float64(p) for p in pieces]
    assert np.array_equal(T.fixed_to_float64(tot), np.sum(piece_sums, axis=0))
    assert (np.abs(T.fixed_to_float64(tot) - exact) <= 49 * T.EPS * exact + 49 * 2.0 ** -32).all()      # the pool bound's last two terms
    # a different cut of the same values gives other words, inside the same bound
    other = T.fixed_sum(vals[:30]) + T.fixed_sum(vals[30:])
    assert (other != tot).any() and (np.abs(T.fixed_to_float64(other) - exact) <= 49 * T.EPS * exact + 49 * 2.0 ** -32).all()


@pytest.mark.parametrize("name", list(T.TAIL_CASES))
def test_reference_alone_is_inside_the_tail_bound(name):
    """fp32 numpy.matmul (its own summation order) against the fp64 product: the bound is derived for the kernel's order of ceil(C / 64) + 8 roundings per
    term, and numpy's pairwise sums are shorter than that -- a bound the plain fp32 product missed would be one no kernel could be held to."""
    c = T.draw_tail_case(name)
    n, C = c["n"], c["C"]
    mean = T.mean_of(c["pool"][:n], c["npix"])
    y64, S = T.tail_fp64(mean, c["w"], c["bias"])
    y32 = np.matmul(mean, c["w"].T)
    if c["bias"] is not None:
        y32 = y32 + c["bias"]
    assert y32.dtype == np.float32 and (S > 0).any()
    ratio = np.abs(y32.astype(np.float64) - y64) / np.maximum(T.tail_bound(S, C), 1e-300)
    print(f"\n{name}: fp32 matmul worst |d| / tail_bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) < 1.0
    assert T.tail_bound(1.0, C) == (math.ceil(C / 64) + 8) * 2.0 ** -24 * (1 + 2.0 ** -20)


def test_top_of_the_range_expected_on_the_device():
    """The values tests/test_gpu_temporal_tail.py::test_top_of_the_fixed_point_range_and_the_range_flag expects.  Centre tap 16: every pixel is 2^26, every
    piece and the total are exact, the image's word is 49 * 2^26 << 32 (above 2^31, below 4e9), no piece trips the guard.  Centre tap 32: the total, 49 *
    2^27, does not fit the word -- and NO piece reaches 4e9 (the largest, the 25 interior pixels, is 3.36e9): the per-piece guard alone would let the word
    wrap unseen, which is what the total check of pooled_epilogue is for."""
    cuts = np.cumsum((0,) + T.RANGE_PIECES)
    assert cuts[-1] == T.RANGE_HW * T.RANGE_HW == 49
    p16 = np.full((49, 1), T.range_pixel(16.0), dtype=np.float32)
    assert float(p16[0, 0]) == 2.0 ** 26
    assert int(T.fixed_sum(p16)[0]) == word(49 << 26) and 2 ** 31 < (49 << 26) < 4.0e9
    words = [int(T.fixed_sum(p16[a:b])[0]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert sum(words) == word(49 << 26) < 1 << 64                                     # any cut: the pieces are exact
    assert not any(bool(T.range_flagged(p16[a:b])[0]) for a, b in zip(cuts[:-1], cuts[1:]))
    assert (49 << 26) < (1 << 32) - 49 * (1 << 16)                                    # ... and below the margin the total check keeps (stmask_hip.h)
    assert float(T.mean_of(np.uint64([word(49 << 26)]), 49)[0]) == 2.0 ** 26
    p32 = np.full((49, 1), T.range_pixel(32.0), dtype=np.float32)
    words = [int(T.fixed_sum(p32[a:b])[0]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert sum(words) == word(49 << 27) >= 1 << 64                                    # the 64-bit word cannot hold it
    assert not any(bool(T.range_flagged(p32[a:b])[0]) for a, b in zip(cuts[:-1], cuts[1:]))
    assert bool(T.range_flagged(p32)[0])                                              # (in one piece it would have been caught)
    # one piece above 2^31 (interior pixels only, tap 24): exact, unflagged, and out of reach of a conversion through a signed int
    p24 = np.full((25, 1), T.range_pixel(T.RANGE_INTERIOR_TAP), dtype=np.float32)
    assert int(T.fixed_sum(p24)[0]) == word(600 << 22) and 2 ** 31 < (600 << 22) < 4.0e9 and not bool(T.range_flagged(p24)[0])
    assert float(T.mean_of(np.uint64([word(600 << 22)]), 49)[0]) == float(np.float32((600 << 22) / 49.0))
    nan = p16.copy()
    nan[3] = np.nan
    assert bool(T.range_flagged(nan)[0]) and bool(T.range_flagged(np.float32([[4.0e9]]))[0]) and not bool(T.range_flagged(np.float32([[3.9e9]]))[0])
