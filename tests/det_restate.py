"""The deterministic backward (csrc/det_backward.hip, csrc/det_accum.h) restated in numpy, shared by test_deterministic_cpu.py and
test_gpu_deterministic.py.

  * exponent(): the rule that picks the fixed-point exponent p, in Python integers (exact).
  * col2im_terms() / roi_terms(): the fp32 terms the scatter kernels add and the flat index each goes to, every operation in np.float32 in the
    kernels' operand order (numpy rounds each once, nothing is contracted), beside the same terms in float64 from the same fp32 positions.
  * fixed_point(): rint(t * 2^p) to int64, the exact integer sum, one conversion -- what the kernels must reproduce bit for bit, in any order.
  * scatter_oracle(): the float64 sum and the tolerance of an element against it,
        4 eps sum|t_i| + L 2^-(p+1),       eps = 2^-23, L the number of terms of the element:
    a term carries at most five fp32 roundings (1 - l twice, the weight product, times the mask, times the gradient: 5/2 eps in all) and the result
    is rounded once more (eps / 2), which 4 eps covers; each term moves by at most half a fixed-point unit, 2^-(p+1).  The in-kernel sigmoid of a
    logit mask adds expf, an addition and a division, which in the worst case would use up the remaining eps and one more; on the MI355X that
    case sits at 0.43 of the bound or less.
  * upsample_adjoint(): the adjoint of bilinear upsampling in float64 with torch's rule and exact source indices, with its tolerance:
        (L + 3) u sum|terms|  +  6 u max(h_in, w_in) sum_near |g|,     u = 2^-24,
    L = the outputs that read the element.  First part: any order of adding L fp32 products errs by at most (L - 1) u of the sum of their
    magnitudes, each product carries two multiplications and the rounding of h = 1 - l (3 u), one more for the final value.  Second part: the fp32
    source index scale * (o + 0.5) - 0.5 is off by at most 3 u in (scale, the product and the difference round once each, on values up to `in`), which
    moves a weight by as much on each axis -- and may move an output across a floor, where its weight is below that error -- so every output
    whose exact index lies within the element's two-pixel reach (widened by the error) counts with |g|.  At a power-of-two ratio every step of
    the index is exact and the second part is zero.
"""
import math

import numpy as np

F = np.float32
EPS = 2.0 ** -23
U = 2.0 ** -24
MIN_BITS = 36
FINITE, ZERO, NONFINITE = 0, 1, 2
ONE_BITS = 0x3F800000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def absmax_bits(a):
    """The integer maximum over the bit patterns of |a| (0 for an empty array)."""
    a = np.abs(np.asarray(a, dtype=np.float32)).view(np.uint32)
    return int(a.max()) if a.size else 0


def value_of_bits(b):
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])


def ceil_log2(b):
    """ceil(log2 v) of the positive finite fp32 value with bit pattern b, exactly."""
    m, e = math.frexp(value_of_bits(b))          # v = m * 2^e, 0.5 <= m < 1
    return e - 1 if m == 0.5 else e


def shape_bits(terms_bound, mass_bound):
    """The largest q with mass_bound * 2^q + terms_bound / 2 < 2^62, or -1."""
    if mass_bound < 1 or terms_bound < 0:
        return -1
    q = -1
    while 2 * mass_bound * 2 ** (q + 1) + terms_bound < 2 ** 63:
        q += 1
    return q


def exponent(bits_a, bits_b, terms_bound, mass_bound):
    """-> (state, p, q).  p is q - E with 2^E the power-of-two bound of a term: E = ceil(log2 a) + ceil(log2 b)."""
    q = shape_bits(terms_bound, mass_bound)
    if bits_a >= 0x7F800000 or bits_b >= 0x7F800000:
        return NONFINITE, 0, q
    if bits_a == 0 or bits_b == 0:
        return ZERO, 0, q
    with np.errstate(over="ignore"):
        if not np.isfinite(F(value_of_bits(bits_a)) * F(value_of_bits(bits_b))):     # the largest product a term can be overflows fp32
            return NONFINITE, 0, q
    return FINITE, q - (ceil_log2(bits_a) + ceil_log2(bits_b)), q


def fixed_point(dest, t32, numel, p):
    """fp32( (sum_i rint(t_i 2^p)) / 2^p ) per destination; the scaling by a power of two is exact in float64."""
    acc = np.zeros(numel, np.int64)
    np.add.at(acc, dest, np.rint(t32.astype(np.float64) * 2.0 ** p).astype(np.int64))
    return (acc.astype(np.float64) * 2.0 ** -p).astype(np.float32)


def scatter_oracle(dest, t64, numel, p):
    """-> (float64 sums, tolerance per element)."""
    ref, mag, cnt = np.zeros(numel), np.zeros(numel), np.zeros(numel)
    np.add.at(ref, dest, t64)
    np.add.at(mag, dest, np.abs(t64))
    np.add.at(cnt, dest, 1.0)
    return ref, 4 * EPS * mag + cnt * 2.0 ** -(p + 1)


def det_result(dest, t32, numel, bits_a, bits_b, terms_bound, mass_bound):
    """What the three passes leave in the output for these terms: zeros, NaN, or the fixed-point sum.  -> (array, state, p)"""
    state, p, q = exponent(bits_a, bits_b, terms_bound, mass_bound)
    assert q >= MIN_BITS
    if state == ZERO:
        return np.zeros(numel, np.float32), state, p
    if state == NONFINITE:
        return np.full(numel, np.nan, np.float32), state, p
    return fixed_point(dest, t32, numel, p), state, p


# ---- deformable col2im ----------------------------------------------------------------------------------------------------------------------
def col2im_terms(gcols, off, mask, B, C, H, W, k, st, pad, dl, dg, mask_logit=False):
    """gcols [B, C*K, Ho*Wo], off [B, dg*2K, Ho, Wo], mask [B, dg*K, Ho, Wo] or None (logits with mask_logit) -> (dest, t32, t64): the terms of
    deform_col2im_kernel with a non-zero gradient value, flat indices into [B, C, H, W]."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = k, st, pad, dl
    K, Cg = kh * kw, C // dg
    Ho, Wo = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    HWo = Ho * Wo
    gcols = np.asarray(gcols, F).reshape(B, dg, Cg, K, HWo)
    off = np.asarray(off, F).reshape(B, dg, K, 2, HWo)
    ho, wo = np.divmod(np.arange(HWo), Wo)
    i, j = np.divmod(np.arange(K), kw)
    base_y = (ho[None, :] * sh - ph + i[:, None] * dh).astype(F)             # [K, HWo]
    base_x = (wo[None, :] * sw - pw + j[:, None] * dw).astype(F)
    fy, fx = base_y + off[:, :, :, 0], base_x + off[:, :, :, 1]              # [B, dg, K, HWo], one fp32 addition
    m32 = np.ones_like(fy)
    m64 = np.ones(fy.shape)
    if mask is not None:
        mk = np.asarray(mask, F).reshape(B, dg, K, HWo)
        if mask_logit:
            m32 = F(1) / (F(1) + np.exp(-mk))                                # the kernel's expression; expf itself may differ in the last bit
            m64 = 1.0 / (1.0 + np.exp(-mk.astype(np.float64)))
        else:
            m32, m64 = mk, mk.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = (fy > F(-1)) & (fx > F(-1)) & (fy < F(H)) & (fx < F(W))
    fl_y, fl_x = np.floor(fy), np.floor(fx)
    lh, lw = fy - fl_y, fx - fl_x
    hh, hw = F(1) - lh, F(1) - lw
    h_low, w_low = np.where(valid, fl_y, 0).astype(np.int64), np.where(valid, fl_x, 0).astype(np.int64)
    lh64, lw64 = lh.astype(np.float64), lw.astype(np.float64)
    corners = [(h_low, w_low, hh * hw * m32, (1 - lh64) * (1 - lw64) * m64), (h_low, w_low + 1, hh * lw * m32, (1 - lh64) * lw64 * m64),
               (h_low + 1, w_low, lh * hw * m32, lh64 * (1 - lw64) * m64), (h_low + 1, w_low + 1, lh * lw * m32, lh64 * lw64 * m64)]
    b_i, g_i, c_i = np.arange(B)[:, None, None, None, None], np.arange(dg)[None, :, None, None, None], np.arange(Cg)[None, None, :, None, None]
    dests, t32s, t64s = [], [], []
    for y, x, w32, w64 in corners:
        ok = valid & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
        take = ok[:, :, None] & (gcols != 0)                                   # [B, dg, Cg, K, HWo]
        d = ((b_i * C + g_i * Cg + c_i) * H + np.clip(y, 0, H - 1)[:, :, None]) * W + np.clip(x, 0, W - 1)[:, :, None]
        t32 = w32[:, :, None] * gcols
        t64 = w64[:, :, None] * gcols.astype(np.float64)
        dests.append(d[take]); t32s.append(t32[take]); t64s.append(t64[take])
    return np.concatenate(dests), np.concatenate(t32s).astype(F), np.concatenate(t64s)


def col2im_bounds(k, Ho, Wo):
    n = k[0] * k[1] * Ho * Wo
    return n, n


# ---- RoIAlign backward ----------------------------------------------------------------------------------------------------------------------
def roi_terms(gout, rois, B, C, H, W, PH, PW, scale, sampling_ratio, aligned):
    """gout [n, C, PH, PW], rois [n, 5] -> (dest, t32, t64): the terms of roi_align_backward_kernel (all four corners of every sample, zero weights
    included, for the non-zero gradient values), flat indices into [B, C, H, W].  Equal RoI rows share their sample positions: one pass each."""
    gout, rois = np.asarray(gout, F), np.asarray(rois, F)
    scale = F(scale)
    chan = np.arange(C)
    dests, t32s, t64s = [], [], []
    uniq, member = np.unique(rois, axis=0, return_inverse=True)
    member = member.reshape(-1)
    for u in range(uniq.shape[0]):
        roi, rows = uniq[u], np.nonzero(member == u)[0]
        bf = roi[0]
        if not (bf >= 0 and bf < B):
            continue
        b = int(bf)
        o = F(0.5) if aligned else F(0)
        sw_, sh_ = roi[1] * scale - o, roi[2] * scale - o
        ew_, eh_ = roi[3] * scale - o, roi[4] * scale - o
        rw, rh = ew_ - sw_, eh_ - sh_
        if not aligned:
            rw, rh = max(rw, F(1)), max(rh, F(1))
        bh, bw = rh / F(PH), rw / F(PW)
        gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / F(PH)))
        gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / F(PW)))
        count = F(max(gh * gw, 1))
        for py in range(PH):
            for px in range(PW):
                gv = gout[rows, :, py, px]                                   # [copies, C]
                nz = gv != 0
                g32 = gv / count
                g64 = gv.astype(np.float64) / float(count)
                for iy in range(gh):
                    y = sh_ + F(py) * bh + (F(iy) + F(0.5)) * bh / F(gh)
                    for ix in range(gw):
                        x = sw_ + F(px) * bw + (F(ix) + F(0.5)) * bw / F(gw)
                        if y < -1 or y > H or x < -1 or x > W:
                            continue
                        yy, xx = (F(0) if y <= 0 else y), (F(0) if x <= 0 else x)
                        yl, xl = int(yy), int(xx)
                        if yl >= H - 1:
                            yh = yl = H - 1
                            yy = F(yl)
                        else:
                            yh = yl + 1
                        if xl >= W - 1:
                            xh = xl = W - 1
                            xx = F(xl)
                        else:
                            xh = xl + 1
                        ly, lx = yy - F(yl), xx - F(xl)
                        hy, hx = F(1) - ly, F(1) - lx
                        ly64, lx64 = float(ly), float(lx)
                        for ya, xa, w32, w64 in ((yl, xl, hy * hx, (1 - ly64) * (1 - lx64)), (yl, xh, hy * lx, (1 - ly64) * lx64),
                                                 (yh, xl, ly * hx, ly64 * (1 - lx64)), (yh, xh, ly * lx, ly64 * lx64)):
                            d = np.broadcast_to(((b * C + chan) * H + ya) * W + xa, gv.shape)
                            dests.append(d[nz])
                            t32s.append((g32 * w32)[nz])
                            t64s.append((g64 * w64)[nz])
    if not dests:
        return np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0)
    return np.concatenate(dests), np.concatenate(t32s).astype(F), np.concatenate(t64s)


def roi_bounds(n, PH, PW, sampling_ratio):
    """(terms_bound, mass_bound) of csrc/det_backward.hip for n RoIs."""
    bins = n * PH * PW
    per_axis = sampling_ratio if sampling_ratio > 0 else 5
    return 4 * per_axis * per_axis * bins, bins + (bins >> 24) + 1


# ---- bilinear upsampling, adjoint ------------------------------------------------------------------------------------------------------------
def upsample_scale(n_in, n_out, scale_factor):
    """torch's scale of one axis in exact arithmetic (a Fraction-free float64: in / out or 1 / scale_factor)."""
    return 1.0 / scale_factor if scale_factor else n_in / n_out


def _axis(n_in, n_out, scale, reach):
    """W [n_in, n_out] float64 weights of torch's rule with exact source indices; near [n_in, n_out]: outputs whose index is within (i - 1 - reach,
    i + 1 + reach) of input i."""
    o = np.arange(n_out)
    src = np.maximum(scale * (o + 0.5) - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    lam = src - i0
    Wm = np.zeros((n_in, n_out))
    inside = i0 <= n_in - 1
    np.add.at(Wm, (np.minimum(i0, n_in - 1), o), np.where(inside, 1.0 - lam, 0.0))
    np.add.at(Wm, (np.minimum(i1, n_in - 1), o), np.where(inside, lam, 0.0))
    i = np.arange(n_in)[:, None]
    near = (src[None, :] > i - 1 - reach) & (src[None, :] < i + 1 + reach)
    return Wm, near.astype(np.float64)


def _is_pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


def upsample_adjoint(g, h_in, w_in, scale_factor=None):
    """g [..., h_out, w_out] -> (grad_in [..., h_in, w_in] float64, tolerance of the same shape)."""
    g = np.asarray(g, np.float64)
    h_out, w_out = g.shape[-2:]
    sf_h, sf_w = (scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor))
    sh, sw = upsample_scale(h_in, h_out, sf_h), upsample_scale(w_in, w_out, sf_w)
    dy = 0.0 if _is_pow2(sh) else 3 * U * h_in
    dx = 0.0 if _is_pow2(sw) else 3 * U * w_in
    Wy, near_y = _axis(h_in, h_out, sh, dy)
    Wx, near_x = _axis(w_in, w_out, sw, dx)
    ref = Wy @ g @ Wx.T
    mag = Wy @ np.abs(g) @ Wx.T
    L = near_y.sum(1)[:, None] * near_x.sum(1)[None, :]
    tol = (L + 3) * U * mag
    if dy or dx:
        tol = tol + 6 * U * max(h_in, w_in) * (near_y @ np.abs(g) @ near_x.T)
    return ref, tol
