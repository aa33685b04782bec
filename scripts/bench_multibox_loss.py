#!/usr/bin/env python3
"""layers.MultiBoxLoss (the whole training criterion on the device, csrc/mbox_loss.hip and csrc/lincomb_backward.hip for its batched mask term) forward + backward with the
stand-in TemporalNet of tests/t2s_loss_restate.py, against two baselines on the same card in the same process:

  P = 15 345, 41 classes, B = 2 / 8 / 16 images (B / 2 clips of two frames), 5 wide boxes per frame with 20 planted priors each (about 100
  positives per image; the count the target assignment gives is printed), prototypes 96 x 160 x 32, masks 384 x 640, 48 x 80 feature map.

  module max_pos=None   layers.MultiBoxLoss: two host reads (the prefix of the mask term's and of the shift loss's row lists)
  module max_pos=K      the padded form, K = 160 B: no host synchronisation
  (a) per-image M       the same layers.* calls with losses['M'] formed as before this module existed: a Python loop over the images with a
                        boolean gather mask_data[idx, cur_pos] (a host round trip), layers.decode, and layers.lincomb_mask_loss_image per image
  (b) torch chain       the reference's chain restated in torch ops: match per image (tests/match_restate.py), the box / centerness, OHEM,
                        track and shift chains of bench_pos_losses.py, bench_conf_loss.py and bench_t2s_loss.py, and the per-image mask loop
                        of multibox_loss.py:555-616 with F.interpolate and F.binary_cross_entropy at target resolution
with, for each path: the time (HIP events around `--reps` back-to-back forward + backward calls after a warm-up, median of 5 groups),
torch.cuda.max_memory_allocated (a fresh peak counter per path; the inputs are included), the host synchronisations of one forward + backward
(torch.cuda.set_sync_debug_mode("warn"), counted warnings; the mode's own once-per-process notice that it is a prototype feature is not one) and, last, the device launches of one forward + backward (kernels and copies seen
by torch.profiler, the stand-in's included; "not measured" if the profiler cannot trace the device).
Usage: python scripts/bench_multibox_loss.py [--reps 3] [--bs 2 8 16] [--out FILE]
"""
import argparse
import os
import sys
import types
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_conf_loss  # noqa: E402
import bench_pos_losses  # noqa: E402
import bench_t2s_loss  # noqa: E402
import match_restate  # noqa: E402
import t2s_loss_restate as T2S  # noqa: E402
from bench_pos_losses import device_launches, peak_mb, timed  # noqa: E402
from stmask_amd import layers  # noqa: E402

P, NC, M, PH, PW, H, W, FH, FW, D = 15345, 41, 32, 96, 160, 384, 640, 48, 80, 128
G, PER_BOX = 5, 20
ALPHAS = dict(bboxiou_alpha=5.0, center_alpha=20.0, conf_alpha=6.125, mask_alpha=6.125, track_alpha=5.0, boxshift_alpha=5.0, maskshift_alpha=6.125)
bench_pos_losses.AB, bench_pos_losses.AC, bench_pos_losses.AT = 5.0, 20.0, 5.0             # the chains read their alphas at call time


def host_syncs(fn):
    """Synchronising operations of one call, as torch's sync debug mode warns of them.  The mode's own notice ("... is a prototype feature ..."),
    raised once per process when the mode is first set, also speaks of synchronising and is not counted."""
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    return sum(1 for w in seen if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message))


def crop_box(b):
    """multibox_loss.py:560-563 on a decoded box, in torch ops (nothing on the device formed it before lincomb_mask_loss)."""
    cs = bench_t2s_loss.t_center_size(b)
    cs[:, 2:] *= 1.2
    pf = torch.cat((cs[:, :2] - cs[:, 2:] / 2, cs[:, :2] + cs[:, 2:] / 2), 1)
    return torch.clamp(pf, min=1e-5, max=1)


def targets(pred, gt):
    boxes, labels, masks, ids = (sum(v, []) for v in gt)
    _, conf_t, idx_t, ids_t, gt_boxes_t = layers.match_batch(0.5, 0.4, boxes, labels, ids, pred["priors"], pred["conf"])
    return conf_t, idx_t, ids_t, gt_boxes_t, masks


def per_image_m(pred, gt, net):
    """(a): the composition a user of the parent commit writes."""
    B = pred["loc"].shape[0]
    conf_t, idx_t, ids_t, gt_boxes_t, masks = targets(pred, gt)
    pri = pred["priors"]
    biou, center = layers.box_center_loss(pred["loc"], pri, gt_boxes_t, conf_t, pred["centerness"], 5.0, 20.0)
    pos = conf_t > 0
    loss_m = 0
    for b in range(B):
        cur = pos[b]
        coeff = pred["mask_coeff"][b, cur]                                                 # the boolean gather: a host round trip
        if coeff.shape[0] == 0:
            continue
        box = crop_box(layers.decode(pred["loc"][b, cur].detach(), pri[cur]))
        w = torch.full((coeff.shape[0],), 1.0 / coeff.shape[0], device=coeff.device)
        loss_m = loss_m + layers.lincomb_mask_loss_image(pred["proto"][b], coeff, box, masks[b], idx_t[b, cur], w)
    c = layers.ohem_conf_loss(pred["conf"], conf_t, 3, 6.125, weights="reference")
    out = {"BIoU": biou / B, "M": loss_m * 6.125 / B, "C": c / B, "center": center / B}
    out.update(layers.track_to_segment_loss(net.TemporalNet, pred["T2S_concat_feat"], pred["loc"][::2], ids_t[::2], pred["mask_coeff"][::2],
                                            pred["proto"][1::2], pri, gt[0], gt[3], gt[2], boxshift_alpha=5.0, maskshift_alpha=6.125))
    out["T"] = layers.track_loss(pred["track"], conf_t, ids_t, 5.0)
    return out


def torch_chain(pred, gt, net):
    """(b): the reference's chain in torch ops."""
    B = pred["loc"].shape[0]
    boxes, labels, masks, ids = (sum(v, []) for v in gt)
    pri = pred["priors"]
    m = [match_restate.match(0.5, 0.4, boxes[b], labels[b], ids[b], pri, pred["conf"][b]) for b in range(B)]      # :138-142
    conf_t, idx_t, ids_t, gt_boxes_t = (torch.stack([r[k] for r in m]) for k in ("conf_t", "idx_t", "ids_t", "gt_boxes_t"))
    priors_b = pri[None].repeat(B, 1, 1)
    biou, center = bench_pos_losses.torch_box_chain(pred["loc"], priors_b, gt_boxes_t, conf_t, pred["centerness"])
    per_img, _ = bench_pos_losses.pos_weights_of(conf_t)
    pos = conf_t > 0
    loss_m = 0
    for b in range(B):                                                                         # :555-616
        cur = pos[b]
        pos_idx_t = idx_t[b, cur]
        box = crop_box(bench_pos_losses.t_decode(pred["loc"][b, cur], pri[cur]).detach())
        if pos_idx_t.size(0) == 0:
            continue
        mask_t = masks[b][pos_idx_t].float()
        soft = bench_t2s_loss.t_generate_mask(pred["proto"][b], pred["mask_coeff"][b, cur, :], box)
        up = F.interpolate(soft.unsqueeze(0), (H, W), mode="bilinear", align_corners=False).squeeze(0)
        pre = F.binary_cross_entropy(torch.clamp(up, 0, 1), mask_t, reduction="none")
        cs = bench_t2s_loss.t_center_size(box)
        bw, bh = torch.clamp(cs[:, 2] * W, min=1), torch.clamp(cs[:, 3] * H, min=1)
        loss_m = loss_m + torch.sum(per_img[b] * (pre.sum(dim=(1, 2)) / bw / bh))
    c = bench_conf_loss.torch_chain(pred["conf"], conf_t)
    out = {"BIoU": biou / B, "M": loss_m * 6.125 / B, "C": c / B, "center": center / B}
    b_shift, m_shift = bench_t2s_loss.torch_chain(net.TemporalNet, pred["T2S_concat_feat"], pred["loc"][::2].detach(), ids_t[::2],
                                                  pred["mask_coeff"][::2].detach(), pred["proto"][1::2].detach(), pri, gt[0], gt[3], gt[2])
    out["B_shift"], out["M_shift"] = b_shift, m_shift
    out["T"] = bench_pos_losses.torch_track_chain(pred["track"], conf_t, ids_t)
    return out


def make_case(B, seed):
    """Priors as bench_pos_losses.py draws them, except that PER_BOX priors per ground-truth box are that box itself, slightly jittered."""
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    pri = torch.cat([0.1 + 0.8 * torch.rand(P, 2, generator=g), 0.05 + 0.35 * torch.rand(P, 2, generator=g)], -1)
    gt = ([], [], [], [])
    slot = torch.randperm(P, generator=g)[:G * PER_BOX].view(G, PER_BOX)
    frames = []
    for b in range(B):
        # wide, thin, disjoint boxes: no randomly drawn prior (at most 0.4 wide) reaches an IoU of 0.5 with them, so the planted ones are the positives
        c = torch.stack([0.5 + 0.02 * torch.rand(G, generator=g), 0.15 * torch.arange(1, G + 1) + 0.01 * torch.rand(G, generator=g)], 1)
        wh = torch.stack([0.86 + 0.04 * torch.rand(G, generator=g), 0.09 + 0.02 * torch.rand(G, generator=g)], 1)
        if b == 0:                                                                             # every image sees the same planted priors
            for k in range(G):
                pri[slot[k]] = torch.cat([c[k], wh[k]])[None] * (1 + 0.04 * (torch.rand(PER_BOX, 4, generator=g) - 0.5))
            base = (c, wh)
        c, wh = base[0] + 0.01 * torch.randn(G, 2, generator=g), base[1] * (1 + 0.02 * torch.randn(G, 2, generator=g))
        frames.append((torch.cat([c - wh / 2, c + wh / 2], 1).to(dev), torch.randint(1, NC, (G,), generator=g).to(dev),
                       (torch.rand(G, H, W, generator=g) > 0.5).to(torch.uint8).to(dev), (torch.arange(1, G + 1) + 10 * (b // 2)).to(dev)))
    for c0 in range(0, B, 2):
        for k in range(4):
            gt[k].append([frames[c0][k], frames[c0 + 1][k]])
    pred = dict(loc=0.3 * torch.randn(B, P, 4, generator=g), conf=2.0 * torch.randn(B, P, NC, generator=g),
                mask_coeff=torch.randn(B, P, M, generator=g), centerness=torch.tanh(torch.randn(B, P, 1, generator=g)),
                track=F.normalize(torch.randn(B, P, D, generator=g), dim=-1), proto=torch.relu(torch.randn(B, PH, PW, M, generator=g)) * 0.2,
                T2S_concat_feat=torch.randn(B // 2, T2S.C_FEAT, FH, FW, generator=g))
    return {k: v.to(dev) for k, v in pred.items()}, pri.to(dev), gt


def case(B, reps, emit):
    pred0, pri, gt = make_case(B, 1400 + B)
    net = types.SimpleNamespace(TemporalNet=T2S.StandInNet(T2S.C_FEAT, M, T2S.NET_SEED).cuda())
    K = 160 * B
    crit = {None: layers.MultiBoxLoss(NC, 0.5, 0.4, 3), K: layers.MultiBoxLoss(NC, 0.5, 0.4, 3, max_pos=K)}

    def run(fn):
        for p in net.TemporalNet.parameters():
            p.grad = None
        pred = {k: v.detach().requires_grad_() for k, v in pred0.items()}
        pred["priors"] = pri
        losses = fn(pred)
        sum(losses.values()).backward()
        return {k: v.detach() for k, v in losses.items()}, pred["proto"].grad, pred["mask_coeff"].grad

    paths = [("module max_pos=None", lambda: run(lambda p: crit[None](net, p, *gt))), (f"module max_pos={K}", lambda: run(lambda p: crit[K](net, p, *gt))),
             ("(a) per-image M", lambda: run(lambda p: per_image_m(p, gt, net))), ("(b) torch chain", lambda: run(lambda p: torch_chain(p, gt, net)))]
    tag = f"B={B:<2d}"
    with torch.no_grad():
        conf_t = targets({**pred0, "priors": pri}, gt)[0]
    emit(f"  {tag}  positives per image: {(conf_t > 0).sum(1).tolist()}")
    ref = paths[3][1]()
    for what, fn in paths[:3]:
        got = fn()
        rel = "  ".join(f"{k} {float((got[0][k] - ref[0][k]).abs() / ref[0][k].abs()):.1e}" for k in ref[0])
        gr = "  ".join(f"{float((a - b).abs().max() / b.abs().max()):.1e}" for a, b in zip(got[1:], ref[1:]))
        emit(f"  {tag}  {what:<22s} |x - torch chain| / |torch chain|: {rel}; grad proto, grad mask_coeff (max norm): {gr}")
    t = {}
    for what, fn in paths:
        t[what] = timed(fn, reps)
        emit(f"  {tag}  {what:<22s} forward + backward {t[what] / 1000.0:9.2f} ms   max_memory_allocated {peak_mb(fn):9.1f} MB   "
             f"host synchronisations {host_syncs(fn):4d}")
    for what, _ in paths[:2]:
        for base in ("(a) per-image M", "(b) torch chain"):
            emit(f"  {tag}  {what:<22s} {base} / module = {t[base] / t[what]:.2f}x" + ("" if t[what] <= t[base] else "   MODULE SLOWER"))
    return tag, paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bs", type=int, nargs="*", default=[2, 8, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multibox_loss.py needs the GPU: no timing is taken on a CPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    try:
        clock = f"{torch.cuda.clock_rate()} MHz shader clock at start"
    except Exception as exc:                                # noqa: BLE001
        clock = f"clock not read ({type(exc).__name__})"
    emit(f"# layers.MultiBoxLoss, forward + backward of the sum of all seven terms, stand-in TemporalNet (C = {T2S.C_FEAT}), P = {P}, {NC} classes, "
         f"prototypes {PH} x {PW} x {M}, masks {H} x {W}, {FH} x {FW} features, {torch.cuda.get_device_name(0)}, {clock}, median of 5 x {a.reps} "
         "calls, fp32")
    kept = [case(B, a.reps, emit) for B in a.bs]
    for tag, paths in kept:                                 # last: the profiler slows the host, and nothing timed comes after it
        for what, fn in paths:
            try:
                emit(f"  {tag}  {what:<22s} device launches (kernels and copies, the stand-in's included) {device_launches(fn):6d}")
            except Exception as exc:                        # noqa: BLE001
                emit(f"  {tag}  {what:<22s} device launches: not measured ({type(exc).__name__}: {exc})")


if __name__ == "__main__":
    main()
