"""fp64 restatement of the mask loss tail -- the end of the reference's lincomb_mask_loss (layers/modules/multibox_loss.py:575, :598-603, the sum of
:613): gather one target per instance, bilinear upsampling (align_corners=False), clamp to [0, 1], binary cross entropy per pixel, sum per instance --
and of its gradient, written from the expressions.  It shares no code with csrc/mask_loss.hip or stmask_amd; test_mask_loss_cpu.py holds it to torch's
own F.interpolate + clamp + F.binary_cross_entropy + autograd, test_gpu_mask_loss.py holds the kernels to it.

The index / weight tables are formed in fp32 by the stated formula, every operation rounded on its own,
    scale = (float)in / (float)out,  src = max(scale * (dst + 0.5f) - 0.5f, 0),  i0 = (int)src,  i1 = i0 + (i0 < in - 1),  l1 = src - i0,  l0 = 1 - l1
and then applied as constants: they are inputs to the arithmetic under test, not part of it (the rule layer_grad_restate.crop_rect and
autograd_restate.py use for positions).  Everything else is fp64.

restate() returns the loss, grad_pred and their magnitude forms -- sum |terms| and sum weight * |dterm| * |grad_loss| -- the `sum|terms|` of the
tolerance |x - x64| <= 1e-5 * sum|terms| + 1e-7 (layer_grad_restate.worst_ratio).
"""
import torch
import torch.nn.functional as F

EPS = float(torch.tensor(1e-12, dtype=torch.float32))     # the floor of pc (1 - pc): torch holds its 1e-12 as an fp32 constant (9.99999996e-13), in fp64 too


def axis_table(n_in, n_out):
    """(i0, i1, l0, l1) of one axis: int64 taps and the fp32 weights as float64."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    dst = torch.arange(n_out, dtype=torch.float32)
    src = torch.clamp(scale * (dst + 0.5) - 0.5, min=0)
    assert src.dtype == torch.float32
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    l0 = 1 - l1
    return i0, i1, l0.double(), l1.double()


def axis_matrix(n_in, n_out):
    """[n_out, n_in] float64: row o holds l0 at i0 and l1 at i1 (added where the two coincide)."""
    i0, i1, l0, l1 = axis_table(n_in, n_out)
    a = torch.zeros(n_out, n_in, dtype=torch.float64)
    rows = torch.arange(n_out)
    a.index_put_((rows, i0), l0, accumulate=True)
    a.index_put_((rows, i1), l1, accumulate=True)
    return a


def upsample(pred, H, W):
    """pred [n,h,w] -> [n,H,W] float64: l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11) with the fp32 tables."""
    p = pred.detach().cpu().double()
    y0, y1, ly0, ly1 = axis_table(p.shape[1], H)
    x0, x1, lx0, lx1 = axis_table(p.shape[2], W)
    top, bot = p[:, y0], p[:, y1]
    return ly0.view(1, H, 1) * (lx0 * top[:, :, x0] + lx1 * top[:, :, x1]) + ly1.view(1, H, 1) * (lx0 * bot[:, :, x0] + lx1 * bot[:, :, x1])


def restate(pred, target, idx=None, grad_loss=None):
    """pred [n,h,w] fp32, target [G,H,W] (uint8 / bool / float), idx [n] int64 or None, grad_loss [n] or None (ones)
    -> (loss [n], grad_pred [n,h,w], mag_loss [n], mag_grad [n,h,w]), float64."""
    n, h, w = pred.shape
    H, W = target.shape[1:]
    t = target.detach().cpu()
    t = (t if idx is None else t[idx.cpu()]).double()
    g = torch.ones(n, dtype=torch.float64) if grad_loss is None else grad_loss.detach().cpu().double()
    up = upsample(pred, H, W)
    pc = up.clamp(0, 1)
    term = -(t * torch.log(pc).clamp(min=-100) + (1 - t) * torch.log(1 - pc).clamp(min=-100))
    dterm = torch.where((up >= 0) & (up <= 1), (pc - t) / (pc * (1 - pc)).clamp(min=EPS), torch.zeros_like(up))
    ay, ax = axis_matrix(h, H), axis_matrix(w, W)
    grad = torch.einsum("Yy,nYX,Xx->nyx", ay, dterm, ax) * g.view(n, 1, 1)
    mag_grad = torch.einsum("Yy,nYX,Xx->nyx", ay, dterm.abs(), ax) * g.abs().view(n, 1, 1)
    return term.sum((1, 2)), grad, term.abs().sum((1, 2)), mag_grad


def torch_chain(pred, target, idx=None, grad_loss=None, dtype=torch.float32):
    """The reference's op chain in torch on the CPU with autograd: (loss [n], grad_pred [n,h,w]) in `dtype`."""
    p = pred.detach().cpu().to(dtype).clone().requires_grad_()
    t = target.detach().cpu()
    t = (t if idx is None else t[idx.cpu()]).to(dtype)
    up = F.interpolate(p.unsqueeze(0), tuple(t.shape[1:]), mode="bilinear", align_corners=False).squeeze(0)
    loss = F.binary_cross_entropy(torch.clamp(up, 0, 1), t, reduction="none").sum(dim=(1, 2))
    g = torch.ones_like(loss) if grad_loss is None else grad_loss.detach().cpu().to(dtype)
    loss.backward(g)
    return loss.detach(), p.grad


def torch_chain_upsample32(pred, H, W):
    """F.interpolate alone, in fp32 on the CPU: [n,H,W]"""
    return F.interpolate(pred.detach().cpu().float().unsqueeze(0), (H, W), mode="bilinear", align_corners=False).squeeze(0)


def worst_ratio(x, x64, mag, rel=1e-5):
    """max |x - x64| / (rel * mag + 1e-7), as layer_grad_restate.worst_ratio; NaN anywhere gives inf."""
    d = (x.detach().cpu().double() - x64).abs()
    r = d / (rel * mag + 1e-7)
    return float("inf") if torch.isnan(r).any() else (r.max().item() if r.numel() else 0.0)


# ---- seeded inputs shared by test_mask_loss_cpu.py and test_gpu_mask_loss.py ----------------------------------------------------------------------
SHAPES = [(12, 20, 48, 80), (12, 20, 24, 40), (12, 20, 31, 47), (12, 20, 45, 77), (12, 20, 12, 20), (5, 7, 33, 29), (9, 13, 36, 52), (24, 40, 96, 160)]


def zero_outside_rectangles(pred, g, every=2):
    """rows 1, 1 + every, ... keep their values inside a random rectangle and are exactly 0 outside it, as generate_mask leaves them"""
    n, h, w = pred.shape
    for i in range(1, n, every):
        ya, xa = int(torch.randint(0, max(h - 2, 1), (1,), generator=g)), int(torch.randint(0, max(w - 2, 1), (1,), generator=g))
        yb, xb = int(torch.randint(ya + 1, h + 1, (1,), generator=g)), int(torch.randint(xa + 1, w + 1, (1,), generator=g))
        keep = torch.zeros(h, w)
        keep[ya:yb, xa:xb] = 1
        pred[i] *= keep
    return pred


def random_case(h, w, H, W, n, seed, G=None, kind="byte", with_idx=True):
    """pred uniform in [0.05, 0.95] with every other row zero outside a rectangle; targets random 0/1 bytes ("byte"), bools ("bool") or uniform fp32
    in [0, 1] ("soft"); idx with repeats over G = n // 2 + 2 targets (with_idx) or None with G = n; grad_loss of mixed signs with zeros."""
    g = torch.Generator().manual_seed(seed)
    pred = zero_outside_rectangles(torch.rand(n, h, w, generator=g) * 0.9 + 0.05, g)
    G = (n // 2 + 2 if with_idx else n) if G is None else G
    if kind == "soft":
        target = torch.rand(G, H, W, generator=g)
    else:
        target = torch.randint(0, 2, (G, H, W), generator=g, dtype=torch.uint8)
        if kind == "bool":
            target = target.bool()
    idx = torch.randint(0, G, (n,), generator=g) if with_idx else None
    grad_loss = torch.randn(n, generator=g)
    if n:
        grad_loss[::3] = 0
    return pred.float(), target, idx, grad_loss.float()


def input_condition(pred):
    """every nonzero prediction lies in [0.05, 0.95]: nearer to 0 or 1 the reference's own fp32 chain leaves the tolerance (near 1, rounding decides
    between log(1 - p) = -16.6 and the clamp at -100)"""
    p = pred.detach().cpu()
    nz = p[p != 0]
    return bool(((nz >= 0.05) & (nz <= 0.95)).all())
