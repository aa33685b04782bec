"""TemporalNet's pooled tail on the MI355X, off the model's own shapes: stm_temporal_pool_fc_f32 (csrc/temporal.hip) on synthetic pools, and the pooled
epilogue of stm_conv2d_planar_windows_pool_f32 (csrc/conv_bf16x.hip) on other maps and at the top of its fixed-point range, against the restatement
of tests/temporal_tail_restate.py (which tests/test_temporal_tail_cpu.py checks on the CPU) and the fp64 oracle convolution."""
import functools

import numpy as np
import pytest
import torch

import oracle
import temporal_tail_restate as T
from stmask_amd import ops, planar
from stmask_amd._lib import StmError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def to_dev_i64(u64):
    """uint64 bit patterns -> the int64 tensor the binding takes (a word of 2^63 or more reads as negative)."""
    return torch.from_numpy(np.ascontiguousarray(u64).view(np.int64).copy()).to(DEV)


def as_u64(t):
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ a. stm_temporal_pool_fc_f32 on synthetic pools
@pytest.mark.parametrize("name", list(T.TAIL_CASES))
def test_pool_fc_on_synthetic_pools(name):
    c = T.draw_tail_case(name)
    n, C, n_out, n_first, npix = (c[k] for k in ("n", "C", "n_out", "n_first", "npix"))
    pool0 = to_dev_i64(c["pool"])
    assert pool0.shape == (n + T.SPARE_ROWS, C) and bool((pool0 < 0).any())
    w = torch.from_numpy(c["w"]).to(DEV)
    bias = torch.from_numpy(c["bias"]).to(DEV) if c["bias"] is not None else None

    def run():
        pool = pool0.clone()
        res = ops.temporal_pool_fc(pool, n, npix, w, bias, n_first=n_first, clear=c["clear"], want_pooled=True)
        torch.cuda.synchronize()
        return pool, res[:-1], res[-1]

    pool, blocks, pooled = run()
    # the means: one rounding, bit for bit
    mean = T.mean_of(c["pool"][:n], npix)
    assert pooled.shape == (n, C) and pooled.dtype == torch.float32
    assert np.array_equal(bits(pooled.cpu().numpy()), bits(mean))
    # the output blocks
    widths = [n_out] if n_first is None else [n_first, n_out - n_first]
    assert len(blocks) == len(widths)
    for blk, wd in zip(blocks, widths):
        assert tuple(blk.shape) == (n, wd) and blk.is_contiguous() and blk.dtype == torch.float32
    y = np.concatenate([b.cpu().numpy() for b in blocks], 1)
    y64, S = T.tail_fp64(mean, c["w"], c["bias"])
    assert np.isfinite(y).all()
    ratio = np.abs(y.astype(np.float64) - y64) / np.maximum(T.tail_bound(S, C), 1e-300)
    print(f"\n{name}: tail worst |d| / tail_bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0
    # what the launch leaves in the pool
    if c["clear"]:
        assert not bool(pool[:n].any()) and torch.equal(pool[n:], pool0[n:])
    else:
        assert torch.equal(pool, pool0)
    # once more on a restored pool: the same bits
    pool_b, blocks_b, pooled_b = run()
    assert torch.equal(pooled_b, pooled) and all(torch.equal(a, b) for a, b in zip(blocks, blocks_b)) and torch.equal(pool_b, pool)


def test_pool_fc_refusals():
    """Each is refused before anything is launched: the pool and the outputs of a good call made afterwards are untouched by them."""
    w = torch.zeros(3, 2049, device=DEV)
    with pytest.raises(StmError):
        ops.temporal_pool_fc(torch.zeros(2, 2049, device=DEV, dtype=torch.int64), 2, 49, w, None)              # C above the kernel's 2048
    with pytest.raises(StmError):
        ops.temporal_pool_fc(torch.zeros(2, 64, device=DEV, dtype=torch.int32), 2, 49, w[:, :64].contiguous(), None)
    with pytest.raises(StmError):
        ops.temporal_pool_fc(torch.zeros(2, 64, device=DEV, dtype=torch.float64), 2, 49, w[:, :64].contiguous(), None)
    pool = torch.full((2, 64), 7 << 32, device=DEV, dtype=torch.int64)
    with pytest.raises(StmError):
        ops.temporal_pool_fc(pool, 2, 49, w[:, :65].contiguous(), None)                                        # weight rows of another length
    with pytest.raises(StmError):
        ops.temporal_pool_fc(pool, 3, 49, w[:, :64].contiguous(), None)                                        # more rows asked for than the pool has
    torch.cuda.synchronize()
    assert bool((pool == 7 << 32).all())


# ------------------------------------------------------------------------------------------------ b. the pooled epilogue on other maps
def window_set(weight, h, w):
    """The border classes of a 3x3 / pad-1 layer on an h x w map, packed under one weight scale as PlanarTemporalNet._border_layer packs them."""
    wsc = ops._pow2_wscale(weight)
    wins, packed = [], []
    for ci, win in planar.border_windows(h, w):
        _, _, k0y, k1y, k0x, k1x = planar._BORDER_CLASSES[ci]
        wins.append(win)
        packed.append(ops.conv_pack_weights(weight[:, :, k0y:k1y, k0x:k1x].contiguous().to(DEV), tile_n=128, fmt=1, wscale=wsc)[0])
    return wins, packed, 1.0 / wsc


@functools.lru_cache(maxsize=None)
def pooled_reference(name, with_bias):
    """(fp64 sum over each image of the oracle's relu(conv + bias), the same of the magnitude convolution): [n, Cout] each, computed once."""
    c = T.draw_pool_case(name)
    x, w = torch.from_numpy(c["x"]), torch.from_numpy(c["w"])
    b = torch.from_numpy(c["b"]) if with_bias else None
    ref = oracle.conv2d_nhwc(x, w, b, None, padding=1, relu=True).double().sum((1, 2))
    mag = oracle.conv2d_nhwc(x.abs(), w.abs(), b.abs() if with_bias else None, None, padding=1).double().sum((1, 2))
    return ref.numpy(), mag.numpy()


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("name", list(T.POOL_GEOMS))
def test_pooled_epilogue_on_other_maps(name, with_bias):
    c = T.draw_pool_case(name)
    h, w, n, O, C = c["h"], c["wd"], c["n"], c["O"], T.POOL_C
    npix = h * w
    wins, packed, out_scale = window_set(torch.from_numpy(c["w"]), h, w)
    assert len(wins) == 9 and sum(win[4] * win[5] for win in wins) == npix
    xp = ops.split_planes(torch.from_numpy(c["x"]).to(DEV), 1)
    bias = torch.from_numpy(c["b"]).to(DEV) if with_bias else None
    flag = ops.planar_range_flag()
    flag.zero_()
    sentinel = to_dev_i64((np.uint64(T.SENTINEL) + np.arange(2 * O, dtype=np.uint64)).reshape(2, O))

    def run(prefill=None):
        pool = torch.zeros(n + 2, O, device=DEV, dtype=torch.int64)
        if prefill is not None:
            pool[:n] = prefill
        pool[n:] = sentinel
        assert ops.conv2d_planar_windows_pool(xp, packed, wins, bias, n, h, w, C, O, h, w, out_scale, pool) is pool
        torch.cuda.synchronize()
        return pool

    a, b = run(), run()
    assert torch.equal(a, b)                                                           # integer accumulation: arrival order cannot matter
    assert torch.equal(a[n:], sentinel)                                                # rows past B are not touched
    g = torch.Generator().manual_seed(5)
    prefill = torch.randint(0, 1 << 44, (n, O), generator=g, dtype=torch.int64).to(DEV)
    p = run(prefill)
    assert torch.equal(p[:n], prefill + a[:n]) and torch.equal(p[n:], sentinel)        # the launch ADDS into what the buffer holds
    # against the fp64 oracle
    ref, mag = pooled_reference(name, with_bias)
    words = as_u64(a[:n])
    got = T.fixed_to_float64(words)
    ratio = np.abs(got - ref) / T.pool_bound(mag, np.abs(ref), npix)
    print(f"\n{name} {'bias' if with_bias else 'no bias'}: pooled sums worst |d| / bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0 and (ref > 0).any()
    # ... and through the tail: the means of exactly these words
    out, pooled = ops.temporal_pool_fc(a, n, npix, torch.ones(3, O, device=DEV), None, want_pooled=True)
    assert np.array_equal(bits(pooled.cpu().numpy()), bits(T.mean_of(words, npix))) and out.shape == (n, 3)
    assert not bool(a[:n].any()) and torch.equal(a[n:], sentinel)
    assert int(flag.item()) == 0                                                       # in range: the flag was left alone


# ------------------------------------------------------------------------------------------------ c. the top of the range and the range flag
def test_top_of_the_fixed_point_range_and_the_range_flag():
    """Expected values: tests/test_temporal_tail_cpu.py::test_top_of_the_range_expected_on_the_device.  x = 32768 in 128 channels (exact in the fp16 planes),
    a 3x3 weight with only its centre tap, which every border class keeps: each pixel is 2^22 * tap."""
    hw, n, C, O = T.RANGE_HW, T.RANGE_N, T.RANGE_C, T.RANGE_O
    xp = ops.split_planes(torch.full((n, hw, hw, C), T.RANGE_X).to(DEV), 1)
    flag = ops.planar_range_flag()
    flag.zero_()
    pool = torch.zeros(n, O, device=DEV, dtype=torch.int64)

    def run(tap, bias=None, planes=xp):
        weight = torch.zeros(O, C, 3, 3)
        weight[:, :, 1, 1] = tap
        wins, packed, out_scale = window_set(weight, hw, hw)
        ops.conv2d_planar_windows_pool(planes, packed, wins, bias, n, hw, hw, C, O, hw, hw, out_scale, pool)
        torch.cuda.synchronize()
        return int(flag.item())

    try:
        assert run(16.0) == 0
        expect = (49 << 26) << 32
        assert expect >= 1 << 63 and float(T.range_pixel(16.0)) == 2.0 ** 26
        words = as_u64(pool)
        assert words.dtype == np.uint64 and bool((words == np.uint64(expect)).all())
        eye = torch.eye(O, device=DEV)
        out, pooled = ops.temporal_pool_fc(pool, n, 49, eye, None, want_pooled=True)
        assert bool((pooled == 2.0 ** 26).all()) and bool((out == 2.0 ** 26).all()) and not bool(pool.any())
        assert int(flag.item()) == 0
        # ONE piece above 2^31: only the 25 interior pixels are non-zero
        x_in = torch.zeros(n, hw, hw, C)
        x_in[:, 1:-1, 1:-1] = T.RANGE_X
        assert run(T.RANGE_INTERIOR_TAP, planes=ops.split_planes(x_in.to(DEV), 1)) == 0
        assert bool((as_u64(pool) == np.uint64((600 << 22) << 32)).all())
        pooled = ops.temporal_pool_fc(pool, n, 49, eye, None, want_pooled=True)[1]
        assert np.array_equal(bits(pooled.cpu().numpy()), bits(T.mean_of(np.full((n, O), (600 << 22) << 32, dtype=np.uint64), 49)))
        # 49 pixels of 2^27: the total leaves the word although no piece reaches the per-piece guard
        assert run(32.0) == 1
        flag.zero_()
        pool.zero_()
        # NaN in one channel's bias: !(sum < 4e9) is true for it
        bias = torch.zeros(O)
        bias[5] = float("nan")
        assert run(16.0, bias.to(DEV)) == 1
        words = as_u64(pool)
        assert bool((np.delete(words, 5, axis=1) == np.uint64(expect)).all())          # the other channels are what they were
    finally:
        flag.zero_()
        pool.zero_()
        torch.cuda.synchronize()
