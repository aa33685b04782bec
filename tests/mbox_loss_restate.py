"""fp64 restatement of the batched mask term of the training criterion (the reference's lincomb_mask_loss, multibox_loss.py:544-616, :636;
include/stmask_hip_train.h and INTEGRATION.md section 14) for the tests of layers.lincomb_mask_loss and layers.MultiBoxLoss: the loss, its
gradients w.r.t. the coefficients and the prototypes, the derived bounds, and the seeded case draws.  It shares no code with
csrc/mbox_loss.hip or stmask_amd/layers; it strings together the restatements the project already has -- the crop rectangle and generate_mask
(layer_grad_restate), the upsampled BCE (mask_loss_restate), the target assignment (match_restate).

Semantics.  r runs over the positives (conf_t > 0) of the batch in flattened order, b(r) its image, n_b the image's positives, w_r = 1 / max(n_b, 1):
    box_r  = clamp(point_form(center_size(decode(loc_r, prior_r)) with width, height * 1.2), 1e-5, 1)         fp32, an INPUT of the arithmetic
             under test (crop_box_f32 below: the torch expression of :559-563; the rule layer_grad_restate.crop_rect uses for positions)
    bce_r  = sum over H x W of BCE(mask idx_t[r] of image b(r), clamp(upsample(generate_mask(proto_b, coeff_r, box_r)), 0, 1))
    term_r = bce_r / max(bw_r W, 1) / max(bh_r H, 1),   bw = box.x2 - box.x1,  bh = box.y2 - box.y1
    M      = mask_alpha * sum_r w_r term_r                                (before multibox_loss's own division by the batch size)
An idx_t outside its image's masks is clamped into range (the reference would raise).

Bounds, first order with eps = 2^-24 per fp32 operation, MARGIN = 1.
  M given the rows' BCE sums (restate_reduce; the M_shift form of t2s_loss_restate): the term carries 6 eps (two differences, two products,
      two quotients), w_r one, the weighted sum of a image's n_b rows n_b more, the scale 2:
          mask_alpha * sum_r w_r (8 + n_b) eps |term_r| + 2 eps |M|
      It holds for ANY fp32 evaluation order (the reference adds an image's rows in fp32, the kernel adds all rows in double).
  grad_bce_r = g * mask_alpha * scale_r (the reduction's adjoint, checked on its own): the fp32 scale carries the term's 6 eps and w_r's one, the
      product in double is rounded once: 8 eps |grad_bce_r|.
  bce_r itself, and M from the inputs (compose): the project's tolerance of the mask kernels, |x - x64| <= 1e-5 * sum|terms| + 1e-7
      (mask_loss_restate), so   |M - M64| <= reduce bound + mask_alpha * sum_r w_r (1e-5 * sum|terms|_r + 1e-7) / max(bw W, 1) / max(bh H, 1).
  grad mask_coeff, grad proto: the project's 1e-5 * sum|terms| + 1e-7 (tests/test_gpu_layer_grads.py), sum|terms| being the same sums on
      absolute values with the BCE adjoint's own magnitude form as the incoming gradient.
Input conditions of a golden case (asserted by the generator, which tries seeds in order): every nonzero mask value lies in [0.05, 0.95]
(mask_loss_restate.input_condition: nearer 1, fp32 rounding decides between log(1 - p) and the clamp at -100), and every crop edge stays at
least EDGE = 1e-4 prototype pixels away from where the crop rule (sanitize_coordinates, padding 1, cast=False) changes an integer, so that a
few ULP of exp cannot move a pixel in or out.

CONSTRUCTED holds a module-level case that no run of the reference backs: the loss kernels end in single-workgroup scans over 256-row tiles whose
threads own more than one tile only past 256 tiles (conf_loss_restate, pos_loss_restate), a size no golden case has; its seed meets the same input
conditions (INPUT_CONDITIONS, EDGE, t2s_loss_restate.KINK), which tests/test_mbox_loss_cpu.py asserts.
"""
import types

import numpy as np
import torch

import layer_grad_restate as LR
import mask_loss_restate as ML
import match_restate
import t2s_loss_restate as T2S

EPS = 2.0 ** -24
MARGIN = 1.0
EDGE = 1e-4
MASK_ALPHA = 6.125                     # mask_alpha of the STMask configs
ALPHAS = dict(bboxiou_alpha=5.0, center_alpha=20.0, conf_alpha=6.125, mask_alpha=6.125, track_alpha=5.0, boxshift_alpha=5.0, maskshift_alpha=6.125)
NUM_CLASSES, POS_T, NEG_T, RATIO = 41, 0.5, 0.4, 3
EMBED = 8


# ------------------------------------------------------------------------------------------ the crop box and the row list
def crop_box_f32(decoded):
    """multibox_loss.py:560-563 on decode's fp32 output [n,4], in torch ops on whatever device the boxes are."""
    b = decoded.detach().float()
    cs = torch.cat(((b[:, 2:] + b[:, :2]) / 2, b[:, 2:] - b[:, :2]), 1)                  # center_size
    cs[:, 2:] *= 1.2
    pf = torch.cat((cs[:, :2] - cs[:, 2:] / 2, cs[:, :2] + cs[:, 2:] / 2), 1)            # point_form
    return torch.clamp(pf, min=1e-5, max=1)


def positives(conf_t):
    """conf_t int64 [B,P] -> (rows: flattened indices of the positives in order, img [n], w [n] double = 1 / max(n_b, 1), n_b [B])."""
    B, P = conf_t.shape
    rows = torch.nonzero(conf_t.reshape(-1) > 0).reshape(-1)
    img = rows // P
    n_b = (conf_t > 0).sum(1)
    return rows, img, 1.0 / n_b.clamp(min=1)[img].double(), n_b


def mask_rows(conf_t, idx_t, counts):
    """Row of the concatenated masks of every positive: offs[b] + clamp(idx_t, 0, G_b - 1)."""
    rows, img, _, _ = positives(conf_t)
    c = torch.tensor(counts, dtype=torch.int64)
    offs = torch.cumsum(c, 0) - c
    k = torch.minimum(idx_t.reshape(-1)[rows].clamp(min=0), c[img] - 1)
    return offs[img] + k


def edge_distance(box, h, w):
    """Smallest distance (prototype pixels) of a crop bound from an integer at which the crop of a pixel row / column changes."""
    b = box.double()
    best = float("inf")
    for c1, c2, size in ((b[:, 0], b[:, 2], w), (b[:, 1], b[:, 3], h)):
        a1, a2 = c1.float().double() * size, c2.float().double() * size
        for v in (torch.minimum(a1, a2) - 1, torch.maximum(a1, a2) + 1):
            k = torch.round(v)
            live = (k >= 0) & (k <= size - 1)
            if bool(live.any()):
                best = min(best, float((v - k).abs()[live].min()))
    return best


# ------------------------------------------------------------------------------------------ the reduction given the rows
def restate_reduce(bce, box, w, n_of_row, H, W, alpha=1.0, g=1.0):
    """bce [n], box [n,4] (fp32 values, used in double), w [n], n_of_row [n] -> dict M, M_bound, term, scale, grad_bce, grad_bce_bound."""
    bce, b, w, nr = bce.double(), box.double(), w.double(), n_of_row.double()
    bw, bh = ((b[:, 2] - b[:, 0]) * W).clamp(min=1), ((b[:, 3] - b[:, 1]) * H).clamp(min=1)
    scale = w / bw / bh
    term = bce / bw / bh
    M = alpha * (w * term).sum()
    bound = MARGIN * (abs(alpha) * (w * (8 + nr) * EPS * term.abs()).sum() + 2 * EPS * M.abs())
    g_bce = g * alpha * scale
    return dict(M=M, M_bound=bound, term=term, scale=scale, grad_bce=g_bce, grad_bce_bound=MARGIN * 8 * EPS * g_bce.abs())


# ------------------------------------------------------------------------------------------ the whole term in double
def compose(loc, coeff, proto, priors, conf_t, idx_t, gt_masks, decode_f32, alpha=MASK_ALPHA, g=1.0):
    """All inputs on the CPU (fp32 values).  loc [B,P,4], coeff [B,P,M], proto [B,h,w,M], priors [P,4] or [B,P,4], conf_t / idx_t int64 [B,P],
    gt_masks: list of B [G_b,H,W]; decode_f32: an fp32 decode ([n,4], [n,4] -> [n,4]).  -> dict: n, rows, img, w, n_b, box (fp32), idx (global
    mask rows), bce, bce_mag, M, M_bound (from the inputs: see the module docstring), reduce (restate_reduce on the fp64 bce), grad_coeff
    [B,P,M], grad_proto [B,h,w,M] of g * M with their magnitudes, pred_ok, min_edge."""
    B, P = conf_t.shape
    Md = coeff.shape[2]
    h, wd = proto.shape[1:3]
    H, W = gt_masks[0].shape[1:]
    rows, img, w, n_b = positives(conf_t)
    n = rows.numel()
    gc, gc_mag = torch.zeros(B * P, Md, dtype=torch.float64), torch.zeros(B * P, Md, dtype=torch.float64)
    gp, gp_mag = torch.zeros(B, h, wd, Md, dtype=torch.float64), torch.zeros(B, h, wd, Md, dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    if n == 0:
        return dict(n=0, rows=rows, img=img, w=w, n_b=n_b, M=zero, M_bound=zero, grad_coeff=gc.view(B, P, Md), grad_proto=gp,
                    grad_coeff_mag=gc_mag.view(B, P, Md), grad_proto_mag=gp_mag, pred_ok=True, min_edge=float("inf"))
    pri = priors.reshape(-1, 4)[rows] if priors.dim() == 3 else priors[rows % P]
    box = crop_box_f32(decode_f32(loc.reshape(-1, 4)[rows].float().contiguous(), pri.float().contiguous()))
    idx = mask_rows(conf_t, idx_t, [int(m.shape[0]) for m in gt_masks])
    masks = torch.cat(list(gt_masks))
    red0 = restate_reduce(torch.zeros(n), box, w, n_b[img], H, W, alpha, g)
    bce, bce_mag = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pred_ok = True
    for b in sorted(set(img.tolist())):
        sel = torch.nonzero(img == b).reshape(-1)
        rect = LR.crop_rect(box[sel], h, wd)
        p64, c64 = proto[b].double(), coeff.reshape(-1, Md)[rows[sel]].double()
        m64 = LR.generate_mask(p64, c64, rect)
        pred_ok = pred_ok and ML.input_condition(m64)
        loss, gpred, mag_loss, mag_g = ML.restate(m64, masks, idx[sel], red0["grad_bce"][sel])
        bce[sel], bce_mag[sel] = loss, mag_loss
        gp[b], gcs = LR.generate_mask_grads(p64, c64, rect, gpred)
        gp_mag[b], gcs_mag = LR.generate_mask_grads(p64, c64, rect, mag_g, absolute=True)
        gc[rows[sel]], gc_mag[rows[sel]] = gcs, gcs_mag
    red = restate_reduce(bce, box, w, n_b[img], H, W, alpha, g)
    tol_bce = 1e-5 * bce_mag + 1e-7
    return dict(n=n, rows=rows, img=img, w=w, n_b=n_b, box=box, idx=idx, bce=bce, bce_mag=bce_mag, reduce=red, M=red["M"],
                M_bound=red["M_bound"] + abs(alpha) * (red["scale"] * tol_bce).sum(), grad_coeff=gc.view(B, P, Md), grad_proto=gp,
                grad_coeff_mag=gc_mag.view(B, P, Md), grad_proto_mag=gp_mag, pred_ok=pred_ok, min_edge=edge_distance(box, h, wd))


# ------------------------------------------------------------------------------------------ seeded draws
# name -> spec.  Priors: a grid of centres with len(scales) square-ish anchors each, P = gy * gx * len(scales).
#   tiny    P = 300: two 256-tiles per image, the second partial; 240 prototype pixels: less than one pixel block; G = (1, 3)
#   blocks  P = 700; 960 prototype pixels: 3.75 pixel blocks; one ground-truth box large enough for >= 17 positives (the 16-row chunk is crossed)
#   m64     P = 260, M = 64
GOLDEN = {
    "tiny": dict(grid=(10, 10), scales=[0.2, 0.35, 0.5], proto=(12, 20), M=8, HW=(48, 80), G=(1, 3), big=None),
    "blocks": dict(grid=(10, 10), scales=[0.15, 0.25, 0.35, 0.45, 0.55, 0.62, 0.7], proto=(24, 40), M=32, HW=(96, 160), G=(2, 5, 1, 4), big=(1, 0)),
    "m64": dict(grid=(13, 10), scales=[0.25, 0.45], proto=(12, 20), M=64, HW=(48, 80), G=(2, 2), big=None),
}
GOLDEN_SEED0 = {name: 51000 + 1000 * i for i, name in enumerate(GOLDEN)}
NET_SEED = T2S.NET_SEED
# Constructed, not captured from the reference: a batch above both lines of the loss kernels' single-workgroup scans (conf_loss_restate,
# pos_loss_restate).  P = 48 * 80 * 3 = 11 520 and 6 images (3 clips): 69 120 OHEM rows in 270 tiles, and 45 list tiles per image -- an odd
# number, so images begin inside a scan thread's chunk of 2 -- 270 in all.  "seed": the first from 54000 on that meets the input conditions the
# golden cases meet (INPUT_CONDITIONS; tests/test_mbox_loss_cpu.py asserts them).
CONSTRUCTED = {
    "rows_270": dict(grid=(48, 80), scales=[0.1, 0.16, 0.24], proto=(12, 20), M=8, HW=(48, 80), G=(2, 3, 1, 2, 2, 1), big=None, seed=54153),
}
# what the generator of the golden cases requires of a seed: the margins of the target assignment and of the OHEM cut, the smallest clamp
# argument of the track loss (the crop edges' EDGE and smooth-L1's t2s_loss_restate.KINK are defined with their restatements)
INPUT_CONDITIONS = dict(match_margin=1e-3, ohem_margin=1e-3, track_min_v=2e-3)


def spec_of(name):
    return GOLDEN[name] if name in GOLDEN else CONSTRUCTED[name]


def make_priors(grid, scales):
    gy, gx = grid
    data = []
    for j in range(gy):
        for i in range(gx):
            for k, s in enumerate(scales):
                ar = 1.0 + 0.1 * ((i + j + k) % 3 - 1)
                data += [(i + 0.5) / gx, (j + 0.5) / gy, s * ar, s / ar]
    return torch.tensor(data, dtype=torch.float64).float().view(-1, 4)


def draw_case(spec, seed):
    """The arguments of MultiBoxLoss.forward on the CPU plus the targets match_restate assigns (conf_t, idx_t, ids_t, gt_boxes_t).  Images 2 c
    and 2 c + 1 are the two frames of clip c; ids are shared between the frames of a clip (1 .. G, offset by 10 per clip)."""
    gen = torch.Generator().manual_seed(int(seed))
    pri = make_priors(spec["grid"], spec["scales"])
    P, M, (H, W), (h, w) = pri.shape[0], spec["M"], spec["HW"], spec["proto"]
    G = spec["G"]
    B = len(G)
    pf = match_restate.point_form(pri)
    inside = torch.nonzero(((pf >= 0.03) & (pf <= 0.97)).all(1)).reshape(-1)
    boxes, labels, ids, masks = [], [], [], []
    for b in range(B):
        pick = inside[torch.randperm(inside.numel(), generator=gen)[:G[b]]]
        bx = pf[pick] + 0.02 * (torch.rand(G[b], 4, generator=gen) - 0.5)
        if spec["big"] is not None and spec["big"][0] == b:
            bx[spec["big"][1]] = torch.tensor([0.19, 0.2, 0.81, 0.8]) + 0.01 * (torch.rand(4, generator=gen) - 0.5)
        boxes.append(bx.float())
        labels.append(torch.randint(1, NUM_CLASSES, (G[b],), generator=gen))
        ids.append(torch.arange(1, G[b] + 1, dtype=torch.int64) + 10 * (b // 2))
        ys, xs = (torch.arange(H).float().view(1, H, 1) + 0.5) / H, (torch.arange(W).float().view(1, 1, W) + 0.5) / W
        rect = (xs >= bx[:, 0].view(-1, 1, 1)) & (xs < bx[:, 2].view(-1, 1, 1)) & (ys >= bx[:, 1].view(-1, 1, 1)) & (ys < bx[:, 3].view(-1, 1, 1))
        masks.append((rect & (torch.rand(G[b], H, W, generator=gen) > 0.15)).to(torch.uint8))          # the box's rectangle with holes
    case = dict(loc=0.3 * torch.randn(B, P, 4, generator=gen), conf=2.0 * torch.randn(B, P, NUM_CLASSES, generator=gen),
                mask_coeff=torch.randn(B, P, M, generator=gen), centerness=torch.tanh(torch.randn(B, P, 1, generator=gen)),
                track=torch.nn.functional.normalize(torch.randn(B, P, EMBED, generator=gen), dim=-1), priors=pri,
                proto=torch.relu(torch.randn(B, h, w, M, generator=gen)) * (1.1 / M ** 0.5),
                T2S_concat_feat=torch.randn(B // 2, T2S.C_FEAT, *T2S.FEAT_HW, generator=gen))
    fold = lambda v: [[v[2 * c], v[2 * c + 1]] for c in range(B // 2)]          # noqa: E731
    case.update(gt_bboxes=fold(boxes), gt_labels=fold(labels), gt_masks=fold(masks), gt_ids=fold(ids))
    m = [match_restate.match(POS_T, NEG_T, boxes[b], labels[b], ids[b], pri, case["conf"][b]) for b in range(B)]
    for k in ("conf_t", "idx_t", "ids_t", "gt_boxes_t", "loc_t"):
        case[k] = torch.stack([r[k] for r in m])
    case["match_margin"] = min(match_restate.margin(r) for r in m)
    return case


def predictions(case, dev=None, grad=False):
    """The `predictions` dict of forward (priors [1,P,4] as the head returns them); grad: leaves that require grad."""
    out = {}
    for k in ("loc", "conf", "mask_coeff", "centerness", "track", "proto", "T2S_concat_feat"):
        t = case[k].clone() if dev is None else case[k].to(dev)
        out[k] = t.requires_grad_() if grad else t
    out["priors"] = (case["priors"] if dev is None else case["priors"].to(dev))[None]
    return out


def ground_truth(case, dev=None):
    mv = (lambda t: t) if dev is None else (lambda t: t.to(dev))
    return tuple([[mv(t) for t in pair] for pair in case[k]] for k in ("gt_bboxes", "gt_labels", "gt_masks", "gt_ids"))


def stand_in_net(M, dev=None, double=False):
    net = T2S.StandInNet(T2S.C_FEAT, M, NET_SEED)
    net = net.double() if double else net
    return types.SimpleNamespace(TemporalNet=net if dev is None else net.to(dev))


def t2s_case(case):
    """The arguments t2s_loss_restate.compose reads, from a case of this module (multibox_loss.py:103-109)."""
    return dict(concat_feat=case["T2S_concat_feat"], loc_ref=case["loc"][::2], ids_t=case["ids_t"][::2], mask_coeff_ref=case["mask_coeff"][::2],
                proto_next=case["proto"][1::2], priors=case["priors"], gt_bboxes=case["gt_bboxes"], gt_ids=case["gt_ids"], gt_masks=case["gt_masks"])


def scalar(a):
    return float(np.asarray(a).reshape(-1)[0])


# ------------------------------------------------------------------------------------------ functional cases with hand-made targets
def functional_case(name, seed=61000):
    """(loc, coeff, proto, priors, conf_t, idx_t, gt_masks) on the CPU with hand-made conf_t / idx_t.
      gap      three images, the middle one without positives; neutral (-1) priors; an idx_t below 0 and one past its image's masks
      none     a batch without any positive (neutrals and background only)"""
    gen = torch.Generator().manual_seed(seed + sorted(("gap", "none")).index(name))
    B, M, (h, w), (H, W) = 3, 8, (12, 20), (24, 40)
    pri = make_priors((10, 10), [0.2, 0.35, 0.5])
    P = pri.shape[0]
    G = (2, 1, 3)
    conf_t = torch.zeros(B, P, dtype=torch.int64)
    idx_t = torch.zeros(B, P, dtype=torch.int64)
    conf_t[:, ::7] = -1
    if name == "gap":
        for b, cnt in ((0, 5), (2, 19)):
            at = torch.randperm(P, generator=gen)[:cnt]
            conf_t[b, at] = torch.randint(1, NUM_CLASSES, (cnt,), generator=gen)
            idx_t[b, at] = torch.randint(0, G[b], (cnt,), generator=gen)
        conf_t[0, 255], conf_t[0, 256], conf_t[2, P - 1] = 3, 4, 5            # both sides of a tile border, the last prior
        idx_t[0, 255], idx_t[0, 256], idx_t[2, P - 1] = -3, 99, 2            # outside the image's masks: clamped
    masks = [(torch.rand(g, H, W, generator=gen) > 0.5).to(torch.uint8) for g in G]
    return dict(loc=0.3 * torch.randn(B, P, 4, generator=gen), mask_coeff=torch.randn(B, P, M, generator=gen),
                proto=torch.relu(torch.randn(B, h, w, M, generator=gen)) * (1.1 / M ** 0.5), priors=pri, conf_t=conf_t, idx_t=idx_t,
                gt_masks=masks)
