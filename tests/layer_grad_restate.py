"""fp64 torch restatements of the three layer functions the reference's loss differentiates through -- generate_mask (layers/mask_utils.py:111-128
with box_utils.crop :341-364), decode (box_utils.py:274-280) and jaccard (box_utils.py:37-88) -- written from the reference's expressions.  They
share no code with the kernels or with stmask_amd/layers; tests/test_layer_grads_cpu.py holds them to the reference's own fp64 outputs and
autograd gradients (tests/golden/layer_grads.npz) and test_gpu_layer_grads.py holds the GPU gradients to them.

The crop rectangle is formed from the fp32 boxes in the kernel's operation order (sanitize_coordinates, cast=False, padding 1) and then applied
as a constant 0/1 mask: it is an input to the arithmetic under test, not part of it (the rule autograd_restate.py uses for sample positions).

Every gradient also has a magnitude form -- the same sum on absolute values, with s (1 - s) and 1 - t^2 kept as they are -- which is the
`sum|terms|` of the tests' tolerance |g - g64| <= rel * sum|terms| + 1e-7.
"""
import torch
import torch.nn.functional as F


# ---- generate_mask ------------------------------------------------------------------------------------------------------------------------
def crop_rect(boxes, h, w, padding=1):
    """[n,4] fp32 relative boxes -> the 0/1 crop mask [n,h,w] (float64), bounds computed in fp32 as box_utils.sanitize_coordinates(cast=False)."""
    b = boxes.detach().float().cpu()

    def bounds(c1, c2, size):
        c1, c2 = c1 * size, c2 * size
        lo, hi = torch.min(c1, c2) - padding, torch.max(c1, c2) + padding
        return torch.clamp(lo, min=0), torch.clamp(hi, max=size)

    x1, x2 = bounds(b[:, 0], b[:, 2], w)
    y1, y2 = bounds(b[:, 1], b[:, 3], h)
    cols = torch.arange(w, dtype=torch.float32).view(1, 1, w)
    rows = torch.arange(h, dtype=torch.float32).view(1, h, 1)
    inside = (cols >= x1.view(-1, 1, 1)) & (cols < x2.view(-1, 1, 1)) & (rows >= y1.view(-1, 1, 1)) & (rows < y2.view(-1, 1, 1))
    return inside.double()


def generate_mask(proto, coeff, rect=None, drop_crop=False):
    """proto [h,w,M], coeff [n,M] (fp64), rect = crop_rect(...) or None -> [n,h,w]: sigmoid(proto @ tanh(coeff)^T) * rect, permuted."""
    m = torch.sigmoid(proto @ torch.tanh(coeff).t())                 # [h,w,n]
    if rect is not None and not drop_crop:
        m = m * rect.permute(1, 2, 0)
    return m.permute(2, 0, 1).contiguous()


def generate_mask_grads(proto, coeff, rect, grad_out, absolute=False, drop_tanh_factor=False):
    """Closed-form (grad_proto, grad_coeff) of generate_mask; absolute=True: the magnitude form (|grad_out|, |t|, |proto| in the sums,
    s (1 - s) and 1 - t^2 as they are).  drop_tanh_factor: the bug of leaving 1 - t^2 out (test_layer_grads_cpu.py)."""
    t = torch.tanh(coeff)
    s = torch.sigmoid(proto @ t.t()).permute(2, 0, 1)                # [n,h,w]
    z = grad_out * s * (1 - s)
    if rect is not None:
        z = z * rect
    pp, tt = proto, t
    if absolute:
        z, pp, tt = z.abs(), proto.abs(), t.abs()
    gp = torch.einsum("nhw,nk->hwk", z, tt)
    gc = torch.einsum("nhw,hwk->nk", z, pp)
    if not drop_tanh_factor:
        gc = gc * (1 - t * t)
    return gp, gc


def generate_mask_chain_fp32(proto, coeff, boxes, grad_out):
    """The reference's own op chain (tanh, matmul, sigmoid, crop as a product with the 0/1 mask, permute) in fp32 torch with autograd: the yardstick
    of the GPU test's tolerance.  Returns (grad_proto, grad_coeff) in fp32."""
    p, c = proto.detach().float().clone().requires_grad_(), coeff.detach().float().clone().requires_grad_()
    m = torch.sigmoid(p @ torch.tanh(c).t())
    if boxes is not None:
        m = m * crop_rect(boxes, p.shape[0], p.shape[1]).float().permute(1, 2, 0)
    m.permute(2, 0, 1).contiguous().backward(grad_out.detach().float())
    return p.grad, c.grad


# ---- decode -------------------------------------------------------------------------------------------------------------------------------
def decode(loc, priors, x2_form="inplace"):
    """boxes = cat(priors_xy + loc_xy * 0.1 * priors_wh, priors_wh * exp(loc_wh * 0.2)); boxes_xy -= boxes_wh / 2; boxes_wh += boxes_xy.
    x2_form="detached_x1": the in-place step's second line differentiated as if the updated x1 were a constant (a wrong backward)."""
    cxy = priors[:, :2] + loc[:, :2] * 0.1 * priors[:, 2:]
    wh = priors[:, 2:] * torch.exp(loc[:, 2:] * 0.2)
    x1 = cxy - wh / 2
    if x2_form == "inplace":
        x2 = wh + x1
    elif x2_form == "centre":                                        # the same function written from the centre: the same derivative
        x2 = cxy + wh / 2
    else:
        assert x2_form == "detached_x1"
        x2 = wh + x1.detach()
    return torch.cat((x1, x2), 1)


def decode_grad_magnitude(loc, priors, grad_boxes):
    """sum|terms| of (grad_loc, grad_priors)."""
    g = grad_boxes.abs()
    gc = g[:, :2] + g[:, 2:]                                         # |d/dcx|: both corners
    gw = gc / 2                                                      # |d/dw|
    e = torch.exp(loc[:, 2:] * 0.2)
    mag_loc = torch.cat((gc * 0.1 * priors[:, 2:].abs(), gw * (priors[:, 2:].abs() * e) * 0.2), 1)
    mag_pri = torch.cat((gc, gc * (loc[:, :2].abs() * 0.1) + gw * e), 1)
    return mag_loc, mag_pri


# ---- jaccard ------------------------------------------------------------------------------------------------------------------------------
def jaccard(a, b):
    """[A,4] x [B,4] point-form boxes -> IoU [A,B]: clamp(min(a_hi, b_hi) - max(a_lo, b_lo), min=0) product over (area_a + area_b - inter)."""
    hi = torch.min(a[:, None, 2:], b[None, :, 2:])
    lo = torch.max(a[:, None, :2], b[None, :, :2])
    ext = torch.clamp(hi - lo, min=0)
    inter = ext[..., 0] * ext[..., 1]
    area_a = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    area_b = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    return inter / (area_a + area_b - inter)


def jaccard_ties(a, b):
    """Number of (pair, coordinate) positions where a min / max compares equal or an overlap extent is exactly zero (the kernel's documented tie
    conventions differ from autograd's there; the tests assert there are none)."""
    hi = torch.min(a[:, None, 2:], b[None, :, 2:])
    lo = torch.max(a[:, None, :2], b[None, :, :2])
    return int((a[:, None, :] == b[None, :, :]).sum() + ((hi - lo) == 0).sum())


def jaccard_grad_magnitude(a, b, grad_out):
    """sum|terms| of (grad_a, grad_b): the overlap path |g| (U + I) / U^2 * other extent, plus the area path |g| I / U^2 * |side|."""
    hi = torch.min(a[:, None, 2:], b[None, :, 2:])
    lo = torch.max(a[:, None, :2], b[None, :, :2])
    raw = hi - lo
    ext = torch.clamp(raw, min=0)
    inter = ext[..., 0] * ext[..., 1]
    wa, ha = (a[:, 2] - a[:, 0]).abs()[:, None], (a[:, 3] - a[:, 1]).abs()[:, None]
    wb, hb = (b[:, 2] - b[:, 0]).abs()[None, :], (b[:, 3] - b[:, 1]).abs()[None, :]
    uni = wa * ha + wb * hb - inter
    g = grad_out.abs()
    gi = g * (uni.abs() + inter) / (uni * uni)
    ga = g * inter / (uni * uni)
    gx, gy = gi * ext[..., 1] * (raw[..., 0] > 0), gi * ext[..., 0] * (raw[..., 1] > 0)
    a_lo_x, a_lo_y = a[:, None, 0] >= b[None, :, 0], a[:, None, 1] >= b[None, :, 1]
    a_hi_x, a_hi_y = a[:, None, 2] <= b[None, :, 2], a[:, None, 3] <= b[None, :, 3]
    mag_a = torch.stack((gx * a_lo_x + ga * ha, gy * a_lo_y + ga * wa, gx * a_hi_x + ga * ha, gy * a_hi_y + ga * wa), -1).sum(1)
    mag_b = torch.stack((gx * ~a_lo_x + ga * hb, gy * ~a_lo_y + ga * wb, gx * ~a_hi_x + ga * hb, gy * ~a_hi_y + ga * wb), -1).sum(0)
    return mag_a, mag_b


# ---- the tail of lincomb_mask_loss (multibox_loss.py:594-614) -----------------------------------------------------------------------------
def mask_loss_tail(masks, boxes, mask_t, weights):
    """masks [n,h,w] from generate_mask, boxes [n,4] point form, mask_t [n,2h,2w] 0/1, weights [n]: bilinear x2 upsampling, clamp to [0, 1], BCE per
    pixel, summed per instance and divided by the box's width and height in target pixels (each at least 1), weighted sum."""
    H, W = mask_t.shape[1:]
    up = F.interpolate(masks.unsqueeze(0), (H, W), mode="bilinear", align_corners=False).squeeze(0)
    pre = F.binary_cross_entropy(torch.clamp(up, 0, 1), mask_t, reduction="none")
    bw = torch.clamp((boxes[:, 2] - boxes[:, 0]) * W, min=1)
    bh = torch.clamp((boxes[:, 3] - boxes[:, 1]) * H, min=1)
    return torch.sum(weights * (pre.sum(dim=(1, 2)) / bw / bh))


class TinyMaskHead(torch.nn.Module):
    """The composite case: a 1x1 convolution (+ relu) makes the prototypes, a linear layer the coefficients; generate_mask and the loss tail follow."""

    def __init__(self, c_in, f_in, m):
        super().__init__()
        self.proto = torch.nn.Conv2d(c_in, m, 1)
        self.coef = torch.nn.Linear(f_in, m)

    def forward(self, x, feats, boxes, mask_t, weights, gen_mask):
        proto = torch.relu(self.proto(x[None]))[0].permute(1, 2, 0).contiguous()        # [h,w,M]
        return mask_loss_tail(gen_mask(proto, self.coef(feats), boxes), boxes, mask_t, weights)


# ---- seeded inputs shared by test_layer_grads_cpu.py and test_gpu_layer_grads.py ----------------------------------------------------------
def mask_boxes(n, h, w, g):
    """Row i is of kind i % 6: random; tiny (2 to 3 pixels, most pixel blocks miss it); whole frame; x1 > x2; partly outside [0, 1]; x1 == x2."""
    c = torch.rand(n, 2, generator=g) * 0.7 + 0.15
    wh = torch.rand(n, 2, generator=g) * 0.5 + 0.1
    b = torch.cat((c - wh / 2, c + wh / 2), 1)
    for i in range(n):
        kind = i % 6
        if kind == 1:
            px = torch.tensor([(2 + (i // 6) % 2) / w, (2 + (i // 12) % 2) / h]) * 0.98
            b[i] = torch.cat((c[i] - px / 2, c[i] + px / 2))
        elif kind == 2:
            b[i] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        elif kind == 3:
            b[i] = b[i, [2, 1, 0, 3]]
        elif kind == 4:
            b[i] = b[i] + torch.tensor([-0.4, -0.3, 0.3, 0.45])
        elif kind == 5:
            b[i, 2] = b[i, 0]
    return b.float()


def mask_case(h, w, n, seed, M=32, with_boxes=True, proto_scale=1.0):
    """relu(randn) prototypes and randn coefficients (the scale the reference's proto-net and head produce), boxes of every kind, randn grad_out."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.relu(torch.randn(h, w, M, generator=g)) * proto_scale
    coeff = torch.randn(n, M, generator=g)
    boxes = mask_boxes(n, h, w, g) if with_boxes else None
    return proto, coeff, boxes, torch.randn(n, h, w, generator=g)


def mask_reference(proto, coeff, boxes, grad_out):
    """(grads fp64, magnitudes) of generate_mask on fp32 inputs: ((gp, gc), (mag_p, mag_c))."""
    rect = None if boxes is None else crop_rect(boxes, proto.shape[0], proto.shape[1])
    args = (proto.double(), coeff.double(), rect, grad_out.double())
    return generate_mask_grads(*args), generate_mask_grads(*args, absolute=True)


def worst_ratio(g, g64, mag, rel=1e-5):
    """max |g - g64| / (rel * mag + 1e-7): the tests' tolerance is this <= 1 (or the stated multiple)."""
    d = (g.detach().cpu().double() - g64.detach().double()).abs()
    return (d / (rel * mag.detach().double() + 1e-7)).max().item()


def jaccard_boxes(A, B, seed):
    """Distinct seeded draws: overlapping pairs (b row i % A near a row) and far-away ones."""
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
        wh = torch.rand(n, 2, generator=g) * 0.3 + 0.05
        return torch.cat((c - wh / 2, c + wh / 2), 1)

    a = draw(A)
    b = draw(B)
    near = a[torch.arange(B) % A] + torch.randn(B, 4, generator=g) * 0.03
    pick = (torch.arange(B) % 3 != 2).view(-1, 1)
    return a.float(), torch.where(pick, near, b).float()
