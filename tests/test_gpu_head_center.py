"""The sparse head's output layers at the centre pixel of its 5 x 5 patch maps (planar.PlanarGraph._sparse_head with STM_HEAD_CENTER on):
the kx-reuse kernel's centre-window launch (csrc/conv_kxr.hip, CTR) and the planar kernel's one-pixel window launch against the centre row of
the "same"-padding launch over the whole maps, which is what the head ran before and what the dense head's sums are held to.

Equality is bit equality (torch.equal): the window forms stage other pixels, they do not form other sums.  Split-K is off on both sides, as in
the head (its launches are gated, and gated launches never split K).  The pixels of a map that the centre pixel's taps do not touch are NaN:
an addressing slip shows up as NaN, not as a small difference."""
import pytest
import torch

from stmask_amd import ops
from stmask_amd.planar import PlanarConv

pytestmark = pytest.mark.gpu

S, C2 = 5, 2                      # side of a patch map, its centre
SHAPES = [(3, 3), (3, 5), (5, 3)]  # kernel shapes of the head's output layers
CW, P = 256, 64                   # channels per tower group, output row stride of a group
GROUP_COUT = [5, 32]              # centerness + bbox, mask coefficients: one and two 16-channel tiles
WRITTEN = [c for g, real in enumerate(GROUP_COUT) for c in range(g * P, g * P + -(-real // 16) * 16)]      # every 16-channel tile is written whole
_cache = {}


def tile_positions(kw, fmt):
    """Positions (images) per workgroup tile of the centre-window launch, per group of GROUP_COUT."""
    return [ops.conv_kxr_tile_pixels(kw, fmt, -(-real // 16)) // kw for real in GROUP_COUT]


def n_max(fmt):
    return max(2 * max(tile_positions(kw, fmt)) + 3 for _, kw in SHAPES) + 8


def maps(fmt, kh, kw, groups_in, n):
    """n random 5 x 5 maps of groups_in * 256 channels as planes of `fmt`; the pixels outside the kh x kw window of the centre are NaN."""
    key = ("x", fmt, kh, kw, groups_in, n)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(1234 + 10 * kh + kw)
        x = torch.randn(n, S, S, groups_in * CW, device="cuda", generator=g)
        xp = ops.split_planes(x, fmt)
        keep = torch.zeros(S, S, dtype=torch.bool, device="cuda")
        keep[C2 - kh // 2:C2 + kh // 2 + 1, C2 - kw // 2:C2 + kw // 2 + 1] = True
        ring = (~keep).flatten().repeat(n)
        xp[:, :, ring, :] = float("nan")
        _cache[key] = xp
    return _cache[key]


def small_layer(fmt, kh, kw):
    key = ("small", fmt, kh, kw)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(77 + 10 * kh + kw)
        w = torch.randn(2 * P, CW, kh, kw, device="cuda", generator=g) * 0.03
        b = torch.randn(2 * P, device="cuda", generator=g)
        for i, real in enumerate(GROUP_COUT):      # rows past a group's real channels are padding
            w[i * P + real:(i + 1) * P] = 0
            b[i * P + real:(i + 1) * P] = 0
        _cache[key] = PlanarConv(w, b, 1, (kh // 2, kw // 2), relu=False, groups=2, tile_n=64, group_cout=GROUP_COUT, fmt=fmt)
        assert _cache[key].kxr
    return _cache[key]


def window(layer):
    return (0, 0, 1, 1, layer.ph - C2, layer.pw - C2, 1, 1)


def centre_launch(layer, xp, n, gate=None, **kw):
    out = torch.full((n, layer.O), float("nan"), device="cuda")
    layer(xp, ("img", n, S, S), out="f32", out_f32=out, window=window(layer), gate=gate, splitk=False, **kw)
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def counts(kw, fmt):
    tps = sorted(set(tile_positions(kw, fmt)))
    assert all(tp > 0 for tp in tps)
    many = 2 * max(tps) + 3           # three or more tiles of every group
    if many % 8 == 0:
        many += 1
    return sorted({1, many} | {tp + d for tp in tps for d in (-1, 0, 1)})


@pytest.mark.parametrize("fmt", [1, 2], ids=["fp16x2", "fp16x1"])
@pytest.mark.parametrize("kh,kw", SHAPES)
def test_centre_mode_is_the_centre_row_of_the_same_padding_launch(kh, kw, fmt):
    layer = small_layer(fmt, kh, kw)
    xp = maps(fmt, kh, kw, 2, n_max(fmt))
    for n in counts(kw, fmt):
        dense = layer(xp, ("img", n, S, S), out="f32", kxr=True, splitk=False).view(n, S * S, layer.O)[:, (S * S) // 2]
        got = centre_launch(layer, xp, n, kxr=True)
        torch.cuda.synchronize()
        assert torch.isfinite(dense[:, WRITTEN]).all(), (n, "the reference reads the NaN ring")
        assert torch.equal(got[:, WRITTEN], dense[:, WRITTEN]), (kh, kw, fmt, n)


@pytest.mark.parametrize("kh,kw", SHAPES)
def test_centre_mode_gate_counts_positions(kh, kw):
    fmt = 1
    layer = small_layer(fmt, kh, kw)
    tp = max(tile_positions(kw, fmt))
    n = 2 * tp + 3
    xp = maps(fmt, kh, kw, 2, n_max(fmt))
    full = centre_launch(layer, xp, n, kxr=True)
    ctl = torch.tensor([0, tp + 2, n, n + 100000], dtype=torch.int32, device="cuda")
    for i, gate in enumerate(ctl.tolist()):
        a = centre_launch(layer, xp, n, gate=(ctl, i), kxr=True)
        b = centre_launch(layer, xp, n, gate=(ctl, i), kxr=True)
        torch.cuda.synchronize()
        k = min(gate, n)
        assert torch.equal(a[:k, WRITTEN], full[:k, WRITTEN]), (kh, kw, gate)
        assert torch.isnan(a[k:]).all(), (kh, kw, gate, "rows at or past the gate were written")
        assert torch.equal(bits(a), bits(b)), (kh, kw, gate, "two runs differ")


@pytest.mark.parametrize("kh,kw", SHAPES)
def test_planar_one_pixel_window_is_the_centre_row_of_the_padded_launch(kh, kw):
    """The track layers (128 channels, the third 256-channel group of the patch planes: x_ch_off) on the tile the pipeline's launch gets, and the
    grouped small layer as the head runs it below the kx-reuse threshold."""
    fmt, n = 1, 300                  # three 128-pixel tiles, the last one partial
    xp = maps(fmt, kh, kw, 3, n)
    g = torch.Generator(device="cuda").manual_seed(5 + 10 * kh + kw)
    wt, bt = torch.randn(128, CW, kh, kw, device="cuda", generator=g) * 0.03, torch.randn(128, device="cuda", generator=g)
    trk = PlanarConv(wt, bt, 1, (kh // 2, kw // 2), relu=False, fmt=fmt)
    assert trk.pick_tile(n) == trk.pick_tile(2304) == 64      # (2 304: the positions the 32-clip step's launches are sized for)
    # the dense head, and the 25-pixel form before, run the track layers of a 32-clip batch on the wide tiles: the window launch on 128 x 64 tiles
    # must give their sums (the tile changes which workgroup forms a sum, not the sum)
    assert trk.pick_tile(2304 * S * S) == trk.pick_tile(32 * 5115) == 128
    wide = PlanarConv(wt, bt, 1, (kh // 2, kw // 2), relu=False, fmt=fmt, tile_n=128)
    padded_wide = wide(xp, ("img", n, S, S), out="f32", splitk=False, x_ch_off=2 * CW).view(n, S * S, 128)[:, (S * S) // 2]
    got_narrow = centre_launch(trk, xp, n, x_ch_off=2 * CW)
    torch.cuda.synchronize()
    assert torch.isfinite(padded_wide).all()
    assert torch.equal(got_narrow, padded_wide), (kh, kw, "128 x 64 window tiles against the padded launch on the wide tiles")
    ctl = torch.tensor([n, 130], dtype=torch.int32, device="cuda")
    for layer, kw_args, cols in ((trk, dict(x_ch_off=2 * CW), list(range(128))), (small_layer(fmt, kh, kw), dict(kxr=False), WRITTEN)):
        padded = layer(xp, ("img", n, S, S), out="f32", splitk=False, **kw_args).view(n, S * S, layer.O)[:, (S * S) // 2]
        got = centre_launch(layer, xp, n, **kw_args)
        gated = centre_launch(layer, xp, n, gate=(ctl, 0), **kw_args)
        part = centre_launch(layer, xp, n, gate=(ctl, 1), **kw_args)
        torch.cuda.synchronize()
        assert torch.isfinite(padded[:, cols]).all()
        assert torch.equal(got[:, cols], padded[:, cols]), (kh, kw, layer.O)
        assert torch.equal(gated[:, cols], padded[:, cols])
        # the planar kernel's gate cuts whole 128-pixel tiles: the rows of the tiles that start below it are written, the others are not
        assert torch.equal(part[:256, cols], padded[:256, cols]) and torch.isnan(part[256:]).all()
