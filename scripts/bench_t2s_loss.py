#!/usr/bin/env python3
"""layers.track_to_segment_loss (csrc/t2s_loss.hip, csrc/lincomb_backward.hip) with the real TemporalNet against a torch-op restatement of the reference's per-clip loop
(multibox_loss.py:247-326), forward + backward, on the same card in the same process:

  C = 633, 48 x 80 feature map, P = 15 345, prototypes 96 x 160, M = 32, masks 384 x 640; bs = 2 / 8 / 16 clips; 20 and 100 shift-positives
  per clip out of 5 / 6 boxes per frame (one id of the reference frame is missing from the next frame).

  kernels      layers.track_to_segment_loss with max_pos=None (one host read), max_pos = n and max_pos = 2 n (none; padded rows cost
               TemporalNet work)
  torch chain  the reference's loop written with torch ops in this file: a Python loop over clips and ids with `id in ids_next` (a device-to-host
               read each), a boolean scatter and an encode per id, boolean gathers, list.index per positive, decode, the box -> RoI conversion,
               this project's RoIAlign (with its backward), one TemporalNet call per clip, tanh / matmul / sigmoid / crop, F.interpolate, clamp,
               F.binary_cross_entropy at target resolution
with, for each path: the time (HIP events around `--reps` back-to-back forward + backward calls after a warm-up of every shape, median of 5
groups), torch.cuda.max_memory_allocated (a fresh peak counter per path; the inputs are included), the host synchronisations of one forward +
backward (torch.cuda.set_sync_debug_mode("warn"), counted warnings) and, last, the device launches of one forward + backward (kernels and copies
seen by torch.profiler, TemporalNet's included; "not measured" if the profiler cannot trace the device).
Usage: python scripts/bench_t2s_loss.py [--reps 3] [--out FILE]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_pos_losses import device_launches, host_syncs, peak_mb, timed  # noqa: E402
from stmask_amd import layers  # noqa: E402
from stmask_amd.mmcv_ops import roi_align  # noqa: E402

C, FH, FW, P, PH, PW, M, H, W = 633, 48, 80, 15345, 96, 160, 32, 384, 640
AB, AM = 5.0, 6.125


def t_encode(matched, priors):
    g_cxcy = ((matched[:, :2] + matched[:, 2:]) / 2 - priors[:, :2]) / (0.1 * priors[:, 2:])
    g_wh = torch.log((matched[:, 2:] - matched[:, :2]) / priors[:, 2:]) / 0.2
    return torch.cat([g_cxcy, g_wh], 1)


def t_center_size(b):
    return torch.cat(((b[:, 2:] + b[:, :2]) / 2, b[:, 2:] - b[:, :2]), 1)


def t_decode(loc, priors):
    boxes = torch.cat((priors[:, :2] + loc[:, :2] * 0.1 * priors[:, 2:], priors[:, 2:] * torch.exp(loc[:, 2:] * 0.2)), 1)
    x1y1 = boxes[:, :2] - boxes[:, 2:] / 2
    return torch.cat((x1y1, boxes[:, 2:] + x1y1), 1)


def t_sanitize(a, b, size, padding=0):
    a, b = a * size, b * size
    lo, hi = torch.min(a, b), torch.max(a, b)
    return torch.clamp(lo - padding, min=0), torch.clamp(hi + padding, max=size)


def t_generate_mask(proto, coeff, bbox):
    m = torch.sigmoid(proto @ torch.tanh(coeff).t())
    h, w, n = m.shape
    x1, x2 = t_sanitize(bbox[:, 0], bbox[:, 2], w, 1)
    y1, y2 = t_sanitize(bbox[:, 1], bbox[:, 3], h, 1)
    rows = torch.arange(w, device=m.device, dtype=x1.dtype).view(1, -1, 1).expand(h, w, n)
    cols = torch.arange(h, device=m.device, dtype=x1.dtype).view(-1, 1, 1).expand(h, w, n)
    crop = (rows >= x1.view(1, 1, -1)) * (rows < x2.view(1, 1, -1)) * (cols >= y1.view(1, 1, -1)) * (cols < y2.view(1, 1, -1))
    return (m * crop.float()).permute(2, 0, 1).contiguous()


def torch_chain(net, concat_feat, loc_ref, ids_t_ref, mask_data_ref, proto_next, priors, gt_bboxes, gt_ids, gt_masks):
    feat_h, feat_w = concat_feat.size()[2:]
    loss_b = torch.zeros(1, device=loc_ref.device)
    loss_m = torch.zeros(1, device=loc_ref.device)
    bs = loc_ref.size(0)
    for i in range(bs):
        ids_cur = ids_t_ref[i].clone()
        ids_ref, ids_next = gt_ids[i][0], gt_ids[i][1]
        reg = torch.zeros_like(loc_ref[i])
        for j, idv in enumerate(ids_ref):
            if idv in ids_next:
                keep = ids_cur == idv
                cur = t_encode(gt_bboxes[i][1][ids_next == idv].view(1, 4), t_center_size(gt_bboxes[i][0][j].view(1, 4)))
                reg[keep] = cur.repeat(keep.sum(), 1)
            else:
                ids_cur[ids_t_ref[i] == idv] = 0
        pos = ids_cur > 0
        if pos.sum() == 0:
            continue
        bbox_p = t_decode(loc_ref[i][pos].view(-1, 4).detach(), priors[pos].view(-1, 4))
        x1, x2 = t_sanitize(bbox_p[:, 0], bbox_p[:, 2], feat_w)
        y1, y2 = t_sanitize(bbox_p[:, 1], bbox_p[:, 3], feat_h)
        rois = torch.stack([torch.zeros_like(x1), x1, y1, x2, y2], 1)
        bbox_reg, shift = net(roi_align(concat_feat[i].unsqueeze(0), rois, 7))
        loss_b += F.smooth_l1_loss(bbox_reg, reg[pos], reduction="none").sum(1).mean()
        pos_idx_t = [ids_next.tolist().index(idv) for idv in ids_cur[pos]]
        bbox_t, mask_t = gt_bboxes[i][1][pos_idx_t], gt_masks[i][1][pos_idx_t].float()
        pred = t_generate_mask(proto_next[i], mask_data_ref[i, pos] + shift, bbox_t)
        up = F.interpolate(pred.unsqueeze(0), (H, W), mode="bilinear", align_corners=False).squeeze(0)
        pre = F.binary_cross_entropy(torch.clamp(up, 0, 1), mask_t, reduction="none")
        cs = t_center_size(bbox_t)
        loss_m += torch.mean(pre.sum(dim=(1, 2)) / (cs[:, 2] * W) / (cs[:, 3] * H))
    return loss_b[0] / bs * AB, loss_m[0] / bs * AM


def make_case(bs, npos, seed):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    pri = torch.cat([0.1 + 0.8 * torch.rand(P, 2, generator=g), 0.05 + 0.35 * torch.rand(P, 2, generator=g)], -1)
    d = dict(concat_feat=torch.randn(bs, C, FH, FW, generator=g).to(dev), loc_ref=(0.5 * torch.randn(bs, P, 4, generator=g)).to(dev),
             mask_coeff_ref=torch.randn(bs, P, M, generator=g).to(dev), proto_next=torch.relu(torch.randn(bs, PH, PW, M, generator=g)).to(dev),
             priors=pri.to(dev), gt_bboxes=[], gt_ids=[], gt_masks=[])
    ids_t = torch.zeros(bs, P, dtype=torch.int64)

    def boxes(G):
        c, wh = 0.25 + 0.5 * torch.rand(G, 2, generator=g), 0.1 + 0.4 * torch.rand(G, 2, generator=g)
        return torch.cat([c - wh / 2, c + wh / 2], 1)

    for i in range(bs):
        ref, nxt = [1, 2, 3, 4, 5, 6], [6, 4, 3, 2, 1]                         # id 5 is missing from the next frame
        d["gt_bboxes"].append([boxes(6).to(dev), boxes(5).to(dev)])
        d["gt_ids"].append([torch.tensor(ref).to(dev), torch.tensor(nxt).to(dev)])
        d["gt_masks"].append([(torch.rand(6, H, W, generator=g) > 0.5).to(torch.uint8).to(dev),
                              (torch.rand(5, H, W, generator=g) > 0.5).to(torch.uint8).to(dev)])
        perm = torch.randperm(P, generator=g)
        ids_t[i, perm[:npos]] = torch.tensor(nxt)[torch.randint(0, 5, (npos,), generator=g)]
        ids_t[i, perm[npos:npos + 10]] = 5                                      # matched priors whose instance left the clip
    d["ids_t"] = ids_t.to(dev)
    return d


def case(bs, npos, reps, emit, net):
    d = make_case(bs, npos, 100 * bs + npos)
    n = bs * npos
    args = (d["concat_feat"], d["loc_ref"], d["ids_t"], d["mask_coeff_ref"], d["proto_next"], d["priors"], d["gt_bboxes"], d["gt_ids"], d["gt_masks"])

    def run(fn):
        for p in net.parameters():
            p.grad = None
        feat = d["concat_feat"].detach().requires_grad_()
        b, m = fn(feat)
        (b + m).backward()
        return b.detach(), m.detach(), net.fc.weight.grad, feat.grad

    def kern(max_pos):
        return lambda: run(lambda feat: tuple(layers.track_to_segment_loss(net, feat, *args[1:], boxshift_alpha=AB, maskshift_alpha=AM,
                                                                           max_pos=max_pos).values()))
    chain = lambda: run(lambda feat: torch_chain(net, feat, *args[1:]))      # noqa: E731
    paths = [("kernels max_pos=None", kern(None)), (f"kernels max_pos={n}", kern(n)), (f"kernels max_pos={2 * n}", kern(2 * n)), ("torch chain", chain)]
    tag = f"bs={bs:<2d} n={n:<4d}"
    rt = chain()
    for what, fn in paths[:3]:
        rk = fn()
        rel = "  ".join(f"{float((a - b).abs().max() / b.abs().max()):.2e}" for a, b in zip(rk, rt))
        emit(f"  {tag}  {what:<24s} max |kernels - torch chain| / max |torch chain| over (B_shift, M_shift, grad fc.weight, grad concat_feat): {rel}")
    t = {}
    for what, fn in paths:
        t[what] = timed(fn, reps)
        emit(f"  {tag}  {what:<24s} forward + backward {t[what] / 1000.0:9.2f} ms   max_memory_allocated {peak_mb(fn):9.1f} MB   "
             f"host synchronisations {host_syncs(fn):4d}")
    for what, _ in paths[:3]:
        emit(f"  {tag}  {what:<24s} torch chain / kernels = {t['torch chain'] / t[what]:.2f}x" + ("" if t[what] <= t["torch chain"] else "   KERNELS SLOWER"))
    return tag, paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bs", type=int, nargs="*", default=[2, 8, 16])
    ap.add_argument("--npos", type=int, nargs="*", default=[20, 100])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_t2s_loss.py needs the GPU: no timing is taken on a CPU")
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
    emit(f"# track_to_segment_loss, forward + backward, real TemporalNet (C = {C}), {FH} x {FW} features, P = {P}, prototypes {PH} x {PW} x {M}, "
         f"masks {H} x {W}, {torch.cuda.get_device_name(0)}, {clock}, median of 5 x {a.reps} calls, fp32")
    torch.manual_seed(0)
    net = layers.TemporalNet(C, M).cuda()
    kept = [case(bs, npos, a.reps, emit, net) for bs in a.bs for npos in a.npos]
    for tag, paths in kept:                                 # last: the profiler slows the host, and nothing timed comes after it
        for what, fn in paths:
            try:
                emit(f"  {tag}  {what:<24s} device launches (kernels and copies, TemporalNet's included) {device_launches(fn):6d}")
            except Exception as exc:                        # noqa: BLE001
                emit(f"  {tag}  {what:<24s} device launches: not measured ({type(exc).__name__}: {exc})")


if __name__ == "__main__":
    main()
