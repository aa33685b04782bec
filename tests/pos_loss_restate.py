"""fp64 restatements of the positive-prior loss terms (include/stmask_hip.h) for the tests of layers.box_center_loss
and layers.track_loss, their derived error bounds, the seeded input draws and the constructed cases.

pos_i = conf_t_i > 0, npos_b the positives of image b, w_i = 1 / max(npos_b, 1).

Box / centerness (restate_box), per positive, from the fp32 inputs in double:
    pred   = decode(loc, prior):  cx = p.x + (l.x * 0.1) * p.z,  w = p.z * exp(l.z * 0.2),  x1 = cx - w / 2,  x2 = w + x1   (0.1, 0.2 as fp32 numbers)
    IoU    = I / U,  I = mx * my,  mx = max(0, min(gt.x2, pred.x2) - max(gt.x1, pred.x1)),  U = area_gt + area_pred - I
    c2     = max(ex^2 + ey^2, 1e-10),  ex = max - min over [pred.x1, pred.x2, gt.x1, gt.x2]
    d2     = dx^2 + dy^2,  dx = (pred.x1 / 2 + pred.x2 / 2) - (gt.x1 / 2 + gt.x2 / 2)
    DIoU   = IoU - d2 / c2
    biou   = alpha_b sum w_i (1 - DIoU_i),   center = alpha_c sum w_i smooth_l1(c_i - DIoU_i)
  Gradient conventions: the DIoU inside `center` is NOT detached (the reference's own behaviour; detach_target=True restates the other reading);
  c2's clamp passes nothing where it cut; min / max of the intersection give a tie to the ground truth's coordinate (jaccard's box_a) and an
  extent that is not strictly positive passes nothing; max / min of the enclosing box go to the FIRST maximal / minimal element in the order
  [pred.x1, pred.x2, gt.x1, gt.x2].

Track loss (restate_track), over the n positives of the whole batch in flattened order:
    s_ij = (x_i . x_j + 1) / 2,  L_ij = -log(max(s_ij, 1e-10)) where ids_i == ids_j else -log(max(1 - s_ij, 1e-10))
    T = alpha sum_{i<j} w_i w_j L_ij / W,  W = sum_{i<j} w_i w_j;   n < 2: T = 0 and a zero gradient (the reference: NaN)
    dL/ds = -1 / s where s > 1e-10 (equal ids), +1 / (1 - s) where 1 - s > 1e-10 (different ids), exactly 0 where the clamp cut; ds/dx_i = x_j / 2.

Bounds.  Every bound is MARGIN times a first-order forward error analysis with eps = 2^-24 per fp32 operation, summed with the weights:
  DIoU:  the decoded coordinates carry dlt_x = eps (|cx| + (4 + |l.z| / 5) w + |x1| + |x2|); through I, the areas and U this gives
         err(IoU) = dI (U + I) / U^2 + dA I / U^2 + 3 eps IoU  (the factor 1 / union), through dx, ex
         err(d2 / c2) = d(d2) / c2 + d(c2) d2 / c2^2 + eps d2 / c2  (the factor 1 / c2).
  track: the fp32 dot of D products carries D eps sum_k |x_ik x_jk|; the pair term is conditioned by 1 / max(s, 1e-10) resp.
         1 / max(1 - s, 1e-10): err(L_ij) = err(s_ij) / max(v_ij, 1e-10) + eps (|L_ij| + 1); a row's gradient is a sum of n fp32 terms added one
         after the other: n eps sum_j |coef_ij x_jd| besides the terms' own errors.
MARGIN is the constant that keeps the reference's own fp32 CPU result inside on every golden case (tests/golden/gen_pos_loss_golden.py asserts it and
stores the observed fraction per case): the derived bounds need no widening, MARGIN = 1, and the reference's largest fraction of them is 0.43
(grad_centerness; 0.18 for the track loss).

The list cases (LIST_CASES, list_targets).  The ordered list of the positives that the track loss, the temporal-fusion loss and the mask term
share is built over tiles of TILE = 256 priors of one image (tpi = ceil(P / 256) tiles per image) and ends in one workgroup of 256 threads: thread
t owns the tiles [t * chunk, (t + 1) * chunk), chunk = ceil(B * tpi / 256), carries the count across them, and takes the images t, t + 256, ...
The reference's generators stay below 256 tiles and 4 images, where neither the carry nor the second trip over the images runs.  The list cases
reach chunk = 2 with images that begin in the middle of a thread's chunk (tpi odd), chunk = 4 with B > 256, and B > 256 with one tile per image,
with positives in an image's first and last row and on both sides of both kinds of tile border (inside a chunk, between two chunks).
"""
import numpy as np
import torch

EPS = 2.0 ** -24
MARGIN = 1.0
V0, V1 = float(np.float32(0.1)), float(np.float32(0.2))
CLAMP = float(np.float32(1e-10))        # the fp32 number nearest 1e-10: what clamp(min=1e-10) compares an fp32 tensor with
TCLAMP = 1e-10                          # the track loss compares in double


def _weights(conf_t):
    """(pos [N] bool, w [n] double per positive in flattened order, npos [B])."""
    B = conf_t.shape[0]
    pos = conf_t > 0
    npos = pos.view(B, -1).sum(1)
    w_img = 1.0 / npos.clamp(min=1).double()
    img = torch.arange(B)[:, None].expand_as(pos)
    return pos.reshape(-1), w_img[img[pos]], npos


def _first_arg(vals, largest):
    """Index of the first maximal / minimal element along dim 1 (strict comparison while scanning in order)."""
    best = torch.zeros(vals.shape[0], dtype=torch.int64)
    cur = vals[:, 0].clone()
    for k in range(1, vals.shape[1]):
        better = vals[:, k] > cur if largest else vals[:, k] < cur
        best[better] = k
        cur = torch.where(better, vals[:, k], cur)
    return best


def _diou_and_jacobian(pred, gt):
    """DIoU [n], its parts, and J [n,4] = d DIoU / d pred under the conventions above."""
    px1, py1, px2, py2 = pred.unbind(1)
    gx1, gy1, gx2, gy2 = gt.unbind(1)
    rx = torch.minimum(gx2, px2) - torch.maximum(gx1, px1)
    ry = torch.minimum(gy2, py2) - torch.maximum(gy1, py1)
    mx, my = rx.clamp(min=0), ry.clamp(min=0)
    inter = mx * my
    wa, ha, wb, hb = gx2 - gx1, gy2 - gy1, px2 - px1, py2 - py1
    uni = wa * ha + wb * hb - inter
    iou = inter / uni
    xs = torch.stack([px1, px2, gx1, gx2], 1)
    ys = torch.stack([py1, py2, gy1, gy2], 1)
    ex = xs.max(1).values - xs.min(1).values
    ey = ys.max(1).values - ys.min(1).values
    c2raw = ex * ex + ey * ey
    cut = c2raw < CLAMP
    c2 = torch.where(cut, torch.full_like(c2raw, CLAMP), c2raw)
    dx = (px1 / 2 + px2 / 2) - (gx1 / 2 + gx2 / 2)
    dy = (py1 / 2 + py2 / 2) - (gy1 / 2 + gy2 / 2)
    d2 = dx * dx + dy * dy
    q = d2 / c2
    diou = iou - q
    # d IoU / d pred (pred is jaccard's box_b: it owns max(x1) only where strictly larger, min(x2) only where strictly smaller)
    gi = (uni + inter) / (uni * uni)
    ga = -inter / (uni * uni)
    gmx = torch.where(rx > 0, gi * my, torch.zeros_like(rx))
    gmy = torch.where(ry > 0, gi * mx, torch.zeros_like(ry))
    zero = torch.zeros_like(rx)
    J = torch.stack([torch.where(gx1 >= px1, zero, -gmx) - ga * hb, torch.where(gy1 >= py1, zero, -gmy) - ga * wb,
                     torch.where(gx2 <= px2, zero, gmx) + ga * hb, torch.where(gy2 <= py2, zero, gmy) + ga * wb], 1)
    # -d2 / c2: the centres ...
    J[:, 0] -= dx / c2
    J[:, 2] -= dx / c2
    J[:, 1] -= dy / c2
    J[:, 3] -= dy / c2
    # ... and the enclosing box: + d2 / c2^2 * d c2, to the first maximal / minimal element
    gc2 = torch.where(cut, zero, q / c2)
    for vals, ext, (lo, hi) in ((xs, ex, (0, 2)), (ys, ey, (1, 3))):
        gext = gc2 * 2 * ext
        imax, imin = _first_arg(vals, True), _first_arg(vals, False)
        J[:, lo] += torch.where(imax == 0, gext, zero) - torch.where(imin == 0, gext, zero)
        J[:, hi] += torch.where(imax == 1, gext, zero) - torch.where(imin == 1, gext, zero)
    parts = dict(mx=mx, my=my, inter=inter, wa=wa, ha=ha, wb=wb, hb=hb, uni=uni, iou=iou, ex=ex, ey=ey, c2=c2, cut=cut, dx=dx, dy=dy, d2=d2, q=q,
                 gi=gi, ga=ga)
    return diou, J, parts


def restate_box(loc_data, priors, gt_boxes_t, conf_t, centerness_data=None, alpha_b=1.0, alpha_c=1.0, g_b=1.0, g_c=1.0, detach_target=False):
    """-> dict: biou, center (None without centerness), grad_loc [B*P,4], grad_cent [B*P] (or None), their bounds, pos, npos, diou."""
    B, P = loc_data.shape[:2]
    N = B * P
    pos, w, npos = _weights(conf_t)
    n = int(pos.sum())
    l = loc_data.detach().double().reshape(N, 4)[pos]
    p = (priors if priors.dim() == 3 else priors[None].expand(B, P, 4)).double().reshape(N, 4)[pos]
    gt = gt_boxes_t.double().reshape(N, 4)[pos]
    has_c = centerness_data is not None
    c = centerness_data.detach().double().reshape(N)[pos] if has_c else None

    tx, ty = l[:, 0] * V0 * p[:, 2], l[:, 1] * V0 * p[:, 3]
    cx, cy = p[:, 0] + tx, p[:, 1] + ty
    ax, ay = l[:, 2] * V1, l[:, 3] * V1
    bw, bh = p[:, 2] * torch.exp(ax), p[:, 3] * torch.exp(ay)
    x1, y1 = cx - bw / 2, cy - bh / 2
    pred = torch.stack([x1, y1, bw + x1, bh + y1], 1)
    diou, J, q = _diou_and_jacobian(pred, gt)

    tb = 1 - diou
    biou = alpha_b * (w * tb).sum()
    sB = g_b * alpha_b * w
    gD = -sB
    center = gc = None
    if has_c:
        dlt = c - diou
        ad = dlt.abs()
        tc = torch.where(ad < 1, 0.5 * dlt * dlt, ad - 0.5)
        center = alpha_c * (w * tc).sum()
        sC = g_c * alpha_c * w
        sl = torch.where(ad < 1, dlt, torch.sign(dlt))
        gc = sC * sl
        if not detach_target:
            gD = gD - gc
    gp = gD[:, None] * J
    gcx, gcy = gp[:, 0] + gp[:, 2], gp[:, 1] + gp[:, 3]
    gw, gh = (gp[:, 2] - gp[:, 0]) / 2, (gp[:, 3] - gp[:, 1]) / 2
    gl = torch.stack([gcx * V0 * p[:, 2], gcy * V0 * p[:, 3], gw * bw * V1, gh * bh * V1], 1)

    # ---- bounds (first order, see the module docstring)
    e = EPS
    dlx = e * (cx.abs() + (4 + ax.abs()) * bw + pred[:, 0].abs() + pred[:, 2].abs())
    dly = e * (cy.abs() + (4 + ay.abs()) * bh + pred[:, 1].abs() + pred[:, 3].abs())
    inter, uni = q["inter"], q["uni"]
    dI = dlx * q["my"] + dly * q["mx"] + 2 * e * inter
    dA = 2 * dlx * q["hb"] + 2 * dly * q["wb"] + 3 * e * (q["wa"] * q["ha"] + q["wb"] * q["hb"])
    dU = dA + dI + e * (q["wa"] * q["ha"] + q["wb"] * q["hb"] + uni.abs())
    e_iou = dI * (uni + inter) / uni ** 2 + dA * inter / uni ** 2 + 3 * e * q["iou"]
    ddx = dlx + 2 * e * (pred[:, 0].abs() + pred[:, 2].abs() + gt[:, 0].abs() + gt[:, 2].abs())
    ddy = dly + 2 * e * (pred[:, 1].abs() + pred[:, 3].abs() + gt[:, 1].abs() + gt[:, 3].abs())
    dd2 = 2 * q["dx"].abs() * ddx + 2 * q["dy"].abs() * ddy + 3 * e * q["d2"]
    dex, dey = dlx + e * q["ex"], dly + e * q["ey"]
    dc2 = torch.where(q["cut"], torch.zeros_like(dex), 2 * q["ex"] * dex + 2 * q["ey"] * dey + 3 * e * q["c2"])
    c2 = q["c2"]
    e_q = dd2 / c2 + dc2 * q["d2"] / c2 ** 2 + e * q["q"]
    e_d = e_iou + e_q + e * diou.abs()
    biou_bound = MARGIN * abs(alpha_b) * (w * (e_d + 3 * e * tb.abs())).sum()
    # the Jacobian's error per coordinate: every part that can reach it
    relU = dU / uni
    t1x, t1y = q["gi"] * q["my"], q["gi"] * q["mx"]                     # through the overlap extents
    t2x, t2y = q["ga"].abs() * q["hb"], q["ga"].abs() * q["wb"]         # through the predicted box's area
    e_t1x = t1x * ((dU + dI) / (uni + inter) + 2 * relU + 4 * e) + dly * q["gi"]
    e_t1y = t1y * ((dU + dI) / (uni + inter) + 2 * relU + 4 * e) + dlx * q["gi"]
    e_t2x = t2x * (2 * relU + 4 * e) + (dI * q["hb"] + inter * 2 * dly) / uni ** 2
    e_t2y = t2y * (2 * relU + 4 * e) + (dI * q["wb"] + inter * 2 * dlx) / uni ** 2
    jdx, jdy = q["dx"].abs() / c2, q["dy"].abs() / c2
    e_jdx = ddx / c2 + jdx * (dc2 / c2 + 3 * e)
    e_jdy = ddy / c2 + jdy * (dc2 / c2 + 3 * e)
    jcx, jcy = 2 * q["ex"] * q["q"] / c2, 2 * q["ey"] * q["q"] / c2
    e_jcx = 2 * (dex * q["d2"] + q["ex"] * dd2) / c2 ** 2 + jcx * (2 * dc2 / c2 + 4 * e)
    e_jcy = 2 * (dey * q["d2"] + q["ey"] * dd2) / c2 ** 2 + jcy * (2 * dc2 / c2 + 4 * e)
    e_jx = e_t1x + e_t2x + e_jdx + e_jcx + 4 * e * (t1x + t2x + jdx + jcx)
    e_jy = e_t1y + e_t2y + e_jdy + e_jcy + 4 * e * (t1y + t2y + jdy + jcy)
    e_gD = e * 3 * sB.abs()
    gc_bound = None
    if has_c:
        lin = (ad < 1).double()
        e_sl = lin * (e_d + e * (c.abs() + ad))
        e_gc = sC.abs() * e_sl + 3 * e * gc.abs()
        gc_bound = MARGIN * e_gc
        if not detach_target:
            e_gD = e_gD + e_gc
        tc_err = torch.minimum(ad, torch.ones_like(ad)) * (e_d + e * (c.abs() + ad)) + 3 * e * tc
        center_bound = MARGIN * abs(alpha_c) * (w * tc_err).sum()
    e_gpx = gD.abs() * e_jx          # for either x coordinate
    e_gpy = gD.abs() * e_jy
    e_gp = torch.stack([e_gpx, e_gpy, e_gpx, e_gpy], 1) + e_gD[:, None] * J.abs() + 2 * e * gp.abs()
    sx, sy = e_gp[:, 0] + e_gp[:, 2] + e * (gp[:, 0].abs() + gp[:, 2].abs()), e_gp[:, 1] + e_gp[:, 3] + e * (gp[:, 1].abs() + gp[:, 3].abs())
    gl_bound = MARGIN * torch.stack([sx * V0 * p[:, 2] + 3 * e * gl[:, 0].abs(), sy * V0 * p[:, 3] + 3 * e * gl[:, 1].abs(),
                                     sx / 2 * bw * V1 + (6 + ax.abs()) * e * gl[:, 2].abs(), sy / 2 * bh * V1 + (6 + ay.abs()) * e * gl[:, 3].abs()], 1)

    def scatter(v, width=None):
        out = torch.zeros((N,) if width is None else (N, width), dtype=torch.float64)
        out[pos] = v
        return out
    return dict(B=B, P=P, N=N, n=n, pos=pos, npos=npos, w=w, diou=diou, pred=pred, biou=biou, center=center, biou_bound=biou_bound,
                center_bound=center_bound if has_c else None, grad_loc=scatter(gl, 4), grad_loc_bound=scatter(gl_bound, 4),
                grad_cent=scatter(gc) if has_c else None, grad_cent_bound=scatter(gc_bound) if has_c else None)


def restate_track(track_data, conf_t, ids_t, alpha=1.0, g=1.0):
    """-> dict: loss, grad [B*P,D], loss_bound, grad_bound [B*P,D], pos, n, min_v (the smallest clamp argument that was not cut)."""
    B, P, D = track_data.shape
    N = B * P
    pos, w, npos = _weights(conf_t)
    n = int(pos.sum())
    grad = torch.zeros(N, D, dtype=torch.float64)
    grad_bound = torch.zeros(N, D, dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    if n < 2:
        return dict(B=B, P=P, D=D, N=N, n=n, pos=pos, loss=zero, loss_bound=zero, grad=grad, grad_bound=grad_bound, min_v=float("inf"))
    X = track_data.detach().double().reshape(N, D)[pos]
    ids = ids_t.reshape(N)[pos]
    dot = X @ X.t()
    adot = X.abs() @ X.abs().t()
    s = (dot + 1) / 2
    eq = ids[:, None] == ids[None, :]
    v = torch.where(eq, s, 1 - s)
    vc = v.clamp(min=TCLAMP)
    L = -torch.log(vc)
    ww = w[:, None] * w[None, :]
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    W = ww[upper].sum()
    loss = alpha * (ww * L)[upper].sum() / W
    live = v > TCLAMP
    dl = torch.where(live, torch.where(eq, -1 / vc, 1 / vc), torch.zeros_like(v))
    coef = g * alpha / W * ww * dl / 2
    coef.fill_diagonal_(0.0)
    gpos = coef @ X
    e = EPS
    e_s = D * e * adot / 2 + e * (dot.abs() + 1 + s.abs())
    e_L = torch.where(live, e_s / vc, torch.zeros_like(v)) + e * (L.abs() + 1)
    loss_bound = MARGIN * (abs(alpha) / W * (ww * e_L)[upper].sum() + 2 * e * loss.abs())
    e_coef = coef.abs() * (e_s / vc + 4 * e)
    gb = MARGIN * (e_coef @ X.abs() + n * e * (coef.abs() @ X.abs()))
    grad[pos] = gpos
    grad_bound[pos] = gb
    off = ~torch.eye(n, dtype=torch.bool)
    return dict(B=B, P=P, D=D, N=N, n=n, pos=pos, loss=loss, loss_bound=loss_bound, grad=grad, grad_bound=grad_bound, W=W,
                min_v=float(v[off & live].min()) if bool((off & live).any()) else float("inf"))


# ------------------------------------------------------------------------------------------ input draws
def draw_conf_t(B, P, npos, gen, nneutral=0):
    """conf_t int64 [B,P]: npos[b] positives (labels 1..40) at random priors of image b, nneutral neutrals (-1), background elsewhere."""
    t = torch.zeros(B, P, dtype=torch.int64)
    for b in range(B):
        perm = torch.randperm(P, generator=gen)
        t[b, perm[:npos[b]]] = torch.randint(1, 41, (npos[b],), generator=gen)
        t[b, perm[npos[b]:npos[b] + nneutral]] = -1
    return t


def draw_boxes(B, P, seed, per_image_priors=False):
    """(loc_data [B,P,4], priors [P,4] or [B,P,4] centre form, gt_boxes_t [B,P,4] point form, centerness [B,P,1]): every prior gets a ground truth
    near its own box (IoU with the decoded prediction mostly 0.2 .. 0.8), the centerness spreads over both branches of smooth-L1."""
    gen = torch.Generator().manual_seed(int(seed))
    shape = (B, P) if per_image_priors else (P,)
    pri = torch.cat([0.1 + 0.8 * torch.rand(*shape, 2, generator=gen), 0.05 + 0.35 * torch.rand(*shape, 2, generator=gen)], -1)
    loc = torch.randn(B, P, 4, generator=gen) * torch.tensor([1.0, 1.0, 0.8, 0.8])
    pb = pri if per_image_priors else pri[None].expand(B, P, 4)
    gc = pb[..., :2] + 0.25 * pb[..., 2:] * torch.randn(B, P, 2, generator=gen)
    gs = pb[..., 2:] * torch.exp(0.25 * torch.randn(B, P, 2, generator=gen))
    gt = torch.cat([gc - gs / 2, gc + gs / 2], -1)
    cent = 1.2 * torch.randn(B, P, 1, generator=gen)
    return loc, pri, gt, cent


def draw_track(B, P, D, seed, n_ids=5):
    """(track_data [B,P,D] unit rows, ids_t int64 [B,P] in 1..n_ids)."""
    gen = torch.Generator().manual_seed(int(seed))
    x = torch.nn.functional.normalize(torch.randn(B, P, D, generator=gen), dim=-1)
    return x, torch.randint(1, n_ids + 1, (B, P), generator=gen)


def targets_at(B, P, rows):
    """conf_t int64 [B,P] with label 1 at the flattened rows given."""
    t = torch.zeros(B * P, dtype=torch.int64)
    t[torch.as_tensor(rows, dtype=torch.int64)] = 1
    return t.view(B, P)


def scalar(a):
    return float(np.asarray(a).reshape(-1)[0])


TILE = 256                              # priors per tile of the positive list, threads of its scanning workgroup

# name -> (B, P, period, {image index modulo the period: its positive priors}); the images not named have none
LIST_CASES = {
    # tpi = 37, 259 tiles, chunk = 2: the images 1, 3 and 5 begin at an odd tile, inside a thread's chunk; the last thread owns one tile
    "tiles_259": (7, 9400, 7, {0: [0, 255, 256, 511, 512, 9399], 1: [0, 1279, 1280, 9399], 3: [0, 2660, 9399], 5: [9399],
                               6: [0, 255, 256, 9215, 9216, 9399]}),
    # tpi = 3 (256 + 256 + 88 priors), 900 tiles, chunk = 4, 300 images
    "tiles_900": (300, 600, 10, {1: [0, 599], 3: [255, 256], 5: [300, 511, 512], 8: [0, 255, 256, 511, 512, 599]}),
    # tpi = 1, 300 tiles, chunk = 2, 300 images: every tile border is an image border
    "images_300": (300, 37, 7, {1: [0, 36], 2: [0], 4: [36], 5: [0, 1, 17, 20, 35, 36]}),
}


def list_positives(name):
    """(B, P, [the positive priors of image b, ascending] for every b) of a list case."""
    B, P, period, table = LIST_CASES[name]
    return B, P, [table.get(b % period, []) for b in range(B)]


def list_targets(name):
    """conf_t int64 [B,P] of a list case: labels 1 .. 40 at its positives, neutrals (-1) at every 11th prior besides, background elsewhere."""
    B, P, per_image = list_positives(name)
    t = torch.zeros(B, P, dtype=torch.int64)
    t[:, 7::11] = -1
    for b, priors in enumerate(per_image):
        for p in priors:
            t[b, p] = 1 + (b * P + p) % 40
    return t


# name -> (B, P, positives per image, neutrals per image, priors per image?)
BOX_GOLDEN = [
    ("p37", 1, 37, [5], 2, False),
    ("ragged", 3, 300, [7, 0, 3], 3, False),
    ("per_image", 2, 300, [6, 4], 2, True),
    ("full_b2", 2, 15345, [80, 70], 12, False),
]
# name -> (B, P, D, positives per image, number of ids)
TRACK_GOLDEN = [
    ("n2", 1, 37, 8, [2], 1),
    ("n63", 1, 300, 8, [63], 4),
    ("n64", 1, 300, 5, [64], 4),
    ("n65", 2, 300, 8, [40, 25], 4),
    ("n130_d128", 3, 300, 128, [70, 0, 60], 5),
    ("d512", 2, 300, 512, [20, 30], 5),
    ("many_pairs", 2, 1000, 8, [800, 700], 12),
    ("full_b2", 2, 15345, 128, [80, 70], 6),
]


def golden_box_case(z, name):
    B, P = (int(v) for v in z[f"box_{name}__shape"])
    per = bool(scalar(z[f"box_{name}__per_image"]))
    loc, pri, gt, cent = draw_boxes(B, P, int(scalar(z[f"box_{name}__seed"])), per)
    return loc, pri, gt, torch.from_numpy(z[f"box_{name}__conf_t"].astype(np.int64)).view(B, P), cent


def golden_track_case(z, name):
    B, P, D = (int(v) for v in z[f"track_{name}__shape"])
    x, ids = draw_track(B, P, D, int(scalar(z[f"track_{name}__seed"])), int(scalar(z[f"track_{name}__n_ids"])))
    return x, torch.from_numpy(z[f"track_{name}__conf_t"].astype(np.int64)).view(B, P), ids


def constructed_box_cases():
    """name -> (loc, priors, gt, conf_t, centerness)"""
    cases = {}
    # P = 257: positives in rows 255, 256 (a tile border inside the image) and in the image's last row of both images
    loc, pri, gt, cent = draw_boxes(2, 257, 5201)
    cases["tile_edges"] = (loc, pri, gt, targets_at(2, 257, [255, 256, 257 + 255, 257 + 256, 3]), cent)
    # the predicted box equals the ground truth (dyadic numbers: the same in fp32 and in double): IoU 1, d2 = 0, 1 - DIoU = 0; every min / max ties
    loc, pri, gt, cent = draw_boxes(1, 37, 5202)
    loc[0, 5] = 0.0
    pri[5] = torch.tensor([0.5, 0.375, 0.25, 0.125])
    gt[0, 5] = torch.tensor([0.375, 0.3125, 0.625, 0.4375])
    cases["degenerate"] = (loc, pri, gt, targets_at(1, 37, [5, 11]), cent)
    # enclosing-box ties: pred.x1 == gt.x1 (the minimum: pred's coordinate comes first and takes the gradient), pred.y2 == gt.y2 (the maximum)
    loc, pri, gt, cent = draw_boxes(1, 37, 5203)
    loc[0, 7] = 0.0
    pri[7] = torch.tensor([0.5, 0.5, 0.25, 0.25])                       # pred = [0.375, 0.375, 0.625, 0.625]
    gt[0, 7] = torch.tensor([0.375, 0.25, 0.75, 0.625])
    cases["enclosing_ties"] = (loc, pri, gt, targets_at(1, 37, [7]), cent)
    return cases


def clamp_case():
    """Rows e1, -e1, e1, e2 with ids 1, 1, 2, 3: pair (0,1) has s = 0 with equal ids, pair (0,2) has 1 - s = 0 with different ids; both terms are
    -log(1e-10) and pass exactly zero gradient.  Basis vectors: every summation order gives the same bits."""
    x = torch.zeros(1, 4, 4)
    x[0, 0, 0], x[0, 1, 0], x[0, 2, 0], x[0, 3, 1] = 1.0, -1.0, 1.0, 1.0
    return x, torch.ones(1, 4, dtype=torch.int64), torch.tensor([[1, 1, 2, 3]])


def constructed_track_cases():
    """name -> (track_data, conf_t, ids_t)"""
    cases = {"clamp": clamp_case()}
    gen = torch.Generator().manual_seed(5300)
    x, ids = draw_track(1, 37, 8, 5301)
    cases["n0"] = (x, draw_conf_t(1, 37, [0], gen, 3), ids)
    cases["n1"] = (x, draw_conf_t(1, 37, [1], gen, 3), ids)
    # three images, the middle one empty, the same ids in the first and the last (cross-image equal-id pairs); ids negative, zero and huge
    x, ids = draw_track(3, 300, 8, 5302, 3)
    ids = torch.tensor([0, -7, 0, 1 << 40])[ids]                        # (draw_track's ids are 1..3)
    cases["cross_image"] = (x, draw_conf_t(3, 300, [9, 0, 5], gen, 2), ids)
    # the list cases (module docstring), D = 8: W = (s1^2 - s2) / 2 passes through the scan's loop over more than 256 images
    for i, name in enumerate(LIST_CASES):
        B, P, _ = list_positives(name)
        x, ids = draw_track(B, P, 8, 5310 + i, 6)
        cases[name] = (x, list_targets(name), ids)
    return cases
