"""fp64 restatement of layers.t2s_concat_feat (reference STMask.py:291-296 over track_to_segment_head.py:40-62) on top of autograd_restate.correlation,
with the magnitude sums the error bounds of tests/test_gpu_t2s_feat.py are made of, and the seeded cases those tests and
tests/golden/gen_t2s_feat_golden.py share."""
import functools

import torch

import autograd_restate as AR

EPS = 2.0 ** -24

# name -> bs, C, Cu, h, w, P, seed; ref: stored by tests/golden/gen_t2s_feat_golden.py from the reference's own correlate + relu(cat).
# The seed of a case is the first of 0, 1, 2, ... at which the margin condition holds (margin_ok below; test_t2s_feat_cpu.py asserts it).
CASES = {
    "smallest": dict(bs=1, C=8, Cu=4, h=3, w=4, P=3, seed=0, ref=True),
    "odd_clips": dict(bs=3, C=20, Cu=8, h=5, w=8, P=11, seed=0, ref=True),           # map smaller than the patch radius, odd clip count
    "ragged": dict(bs=2, C=18, Cu=6, h=6, w=37, P=11, seed=0, ref=False),            # w no multiple of 4, channel-chunk tail
    "p4_384x640": dict(bs=2, C=32, Cu=16, h=24, w=40, P=11, seed=0, ref=False),
    "row_736x1280": dict(bs=1, C=16, Cu=8, h=4, w=80, P=11, seed=0, ref=False),
    "tile_cross": dict(bs=1, C=12, Cu=4, h=3, w=70, P=5, seed=0, ref=False),         # a row crossing a 64-column tile of the adjoint
    # the adjoint's patch staging leaves LDS above 48 KB: P = 13 for the next-frame launch only (51 376 B; 43 264 B for the reference frame's),
    # P = 15 for both (57 600 B), there with a row that crosses a 64-column tile.  Appended: draw_case seeds by position.
    "mode1_global_p13": dict(bs=2, C=6, Cu=2, h=5, w=9, P=13, seed=0, ref=False),
    "both_global_p15": dict(bs=1, C=5, Cu=2, h=4, w=70, P=15, seed=0, ref=False),
}


@functools.lru_cache(maxsize=None)
def draw_case(name, seed=None):
    """fp32 CPU inputs: fpn [2 bs, C, h, w] with distinct values in every image, the next frame of the last clip exact zeros when there is more than
    one clip; t2s [2 bs, Cu, h, w] with negatives and exact zeros; grad_out [bs, P*P + 2 Cu, h, w]."""
    s = CASES[name]
    g = torch.Generator().manual_seed(52000 + 977 * list(CASES).index(name) + (s["seed"] if seed is None else seed))
    bs, C, Cu, h, w, P = (s[k] for k in ("bs", "C", "Cu", "h", "w", "P"))
    fpn = torch.randn(2 * bs, C, h, w, generator=g)
    if bs > 1:
        fpn[2 * bs - 1] = 0.0
    t2s = torch.randn(2 * bs, Cu, h, w, generator=g)
    t2s[torch.rand(t2s.shape, generator=g) < 0.1] = 0.0
    grad_out = torch.randn(bs, P * P + 2 * Cu, h, w, generator=g)
    return dict(fpn=fpn, t2s=t2s, grad_out=grad_out, P=P)


def feature(fpn, t2s, P):
    """(out, corr, S): out the fp64 feature [bs, P*P + 2 Cu, h, w]; corr the correlation channels before the clamp, sum_c a b / C; S = sum_c |a b|."""
    fpn, t2s = fpn.double(), t2s.double()
    n, C, h, w = fpn.shape
    ref, nxt = fpn[::2], fpn[1::2]
    corr = AR.correlation(ref, nxt, P).reshape(n // 2, P * P, h, w) / C
    S = AR.correlation(ref.abs(), nxt.abs(), P).reshape(n // 2, P * P, h, w)
    lrelu = torch.where(corr > 0, corr, 0.1 * corr)                                   # leaky_relu(0.1), then the relu over the cat
    out = torch.relu(torch.cat([lrelu, t2s[::2], t2s[1::2]], 1))
    return out, corr, S


def forward_bound(S, C):
    """|fp32 - fp64| of a correlation channel for ANY fp32 order of the sum of C products, the scaling by 1/C (rounded) and its rounding:
    (C + 2) 2^-24 S / C."""
    return (C + 2) * EPS * S / C


def margin_ok(name, seed=None):
    """Every correlation value is exactly 0 in fp64 or farther from 0 than the forward bound: fp32 and fp64 then agree on the gate."""
    c = draw_case(name, seed)
    _, corr, S = feature(c["fpn"], c["t2s"], c["P"])
    b = forward_bound(S, c["fpn"].shape[1])
    return bool(((corr == 0) | (corr.abs() > b)).all())


def gradients(fpn, t2s, grad_out, P):
    """(grad_fpn, grad_t2s, mag): autograd of the fp64 restatement, and mag = sum |g~ src| per element of grad_fpn (before the division by C)."""
    f64, t64 = fpn.double().requires_grad_(), t2s.double().requires_grad_()
    out, corr, _ = feature(f64, t64, P)
    g_fpn, g_t2s = torch.autograd.grad(out, (f64, t64), grad_out.double())
    n, C, h, w = fpn.shape
    a64 = fpn.double().abs().requires_grad_()
    mag_corr = AR.correlation(a64[::2], a64[1::2], P).reshape(n // 2, P * P, h, w)
    gate = (corr.detach() > 0).double()
    (mag,) = torch.autograd.grad(mag_corr, a64, grad_out[:, :P * P].double().abs() * gate)
    return g_fpn, g_t2s, mag


def backward_bound(mag, C, P):
    """(P^2 + 3) 2^-24 sum |g~ src| / C: the gate-and-scale product, the P^2 fmaf steps in any order, the products."""
    return (P * P + 3) * EPS * mag / C
