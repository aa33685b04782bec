"""The positive-prior loss terms -- losses['BIoU'] with losses['center'] (multibox_loss.py:164-172, :450-455) and losses['T'] (track_loss,
:328-351) -- forward + backward on one MI355X at the training shape, next to torch-op restatements of the reference's chains on the same card in
the same process.

Shape: P = 15 345 priors, D = 128 track channels, B = 2 / 8 / 32 images with 100 positives per image (and 12 neutrals), 6 instance ids.
Two whole paths per function are timed, each forward + backward with autograd from the leaves to .grad:
  kernels   layers.box_center_loss (csrc/pos_loss.hip: 2 launches forward, 1 backward) and layers.track_loss (5 forward, 5 backward); no host
            synchronisation
  torch     the reference's chains as torch ops on the device: the positives' weights, boolean gathers, decode and get_DIoU (the full n x n
            jaccard for its diagonal) once for BIoU and once more for center; cos_sim, inst_eq, loss_weights, the clamps, logs and triu_ of
            track_loss -- with the host round trips the reference has
with, for each path: the time (HIP events around `--reps` back-to-back calls after a warm-up, median of 5 groups), torch.cuda.max_memory_allocated
(a fresh peak counter per path; the inputs are allocated before it is reset and are included), the host synchronisations of one forward +
backward (torch.cuda.set_sync_debug_mode("warn"), counted warnings) and, last, the device launches of one forward + backward (kernels and
copies seen by torch.profiler; "not measured" if the profiler cannot trace the device).
Usage: python scripts/bench_pos_losses.py [--reps 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stmask_amd import layers  # noqa: E402

P, D, NPOS, NNEU, N_IDS = 15345, 128, 100, 12, 6
AB, AC, AT = 1.5, 1.0, 5.0


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1000.0 / reps)
    return statistics.median(per)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 1e6


def host_syncs(fn):
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
    return sum(1 for w in seen if "synchroniz" in str(w.message).lower())


def device_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    if n == 0:
        raise RuntimeError("the profiler saw no device activity")
    return n


def pos_weights_of(conf_t):
    pos = conf_t > 0
    num_pos_per_img = [pos[i].sum().long() for i in range(conf_t.size(0))]
    split = torch.ones(int(pos.sum().tolist()), device=conf_t.device).split(num_pos_per_img)
    per_img = [cur / torch.clamp(cur.sum(), min=1) for cur in split]
    return per_img, torch.cat(per_img, dim=0)


def t_decode(loc, priors):
    boxes = torch.cat((priors[:, :2] + loc[:, :2] * 0.1 * priors[:, 2:], priors[:, 2:] * torch.exp(loc[:, 2:] * 0.2)), 1)
    x1y1 = boxes[:, :2] - boxes[:, 2:] / 2
    return torch.cat((x1y1, boxes[:, 2:] + x1y1), 1)


def t_jaccard(a, b):
    A, Bn = a.size(0), b.size(0)
    max_xy = torch.min(a[:, 2:].unsqueeze(1).expand(A, Bn, 2), b[:, 2:].unsqueeze(0).expand(A, Bn, 2))
    min_xy = torch.max(a[:, :2].unsqueeze(1).expand(A, Bn, 2), b[:, :2].unsqueeze(0).expand(A, Bn, 2))
    inter = torch.clamp(max_xy - min_xy, min=0)
    inter = inter[:, :, 0] * inter[:, :, 1]
    area_a = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).unsqueeze(1).expand_as(inter)
    area_b = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).unsqueeze(0).expand_as(inter)
    return inter / (area_a + area_b - inter)


def t_diou(pred, gt):
    iou = t_jaccard(gt, pred).diag().view(-1)
    x_label = torch.cat([pred[:, ::2], gt[:, ::2]], dim=1)
    y_label = torch.cat([pred[:, 1::2], gt[:, 1::2]], dim=1)
    c2 = (x_label.max(dim=1)[0] - x_label.min(dim=1)[0]) ** 2 + (y_label.max(dim=1)[0] - y_label.min(dim=1)[0]) ** 2
    c2 = torch.clamp(c2, min=1e-10)
    d2 = ((pred[:, :2] / 2 + pred[:, 2:] / 2 - (gt[:, :2] / 2 + gt[:, 2:] / 2)) ** 2).sum(dim=1)
    return iou - d2 / c2


def torch_box_chain(loc_data, priors, gt_boxes_t, conf_t, centerness_data):
    pos = conf_t > 0
    _, pos_weights = pos_weights_of(conf_t)
    decoded = t_decode(loc_data[pos].view(-1, 4), priors[pos].view(-1, 4))                 # :165-172
    biou = (pos_weights * (1 - t_diou(decoded, gt_boxes_t[pos]))).sum() * AB
    pos = (conf_t.view(-1) > 0).float().gt(0)                                              # :450-455
    decoded = t_decode(loc_data.view(-1, 4)[pos], priors.view(-1, 4)[pos])
    diou = t_diou(decoded, gt_boxes_t.view(-1, 4)[pos])
    center = AC * (pos_weights * F.smooth_l1_loss(centerness_data.view(-1)[pos], diou, reduction="none")).sum()
    return biou, center


def torch_track_chain(track_data, conf_t, ids_t):
    per_img, _ = pos_weights_of(conf_t)
    pos = conf_t > 0
    pos_track_data = track_data[pos]
    pos_ids_t = ids_t[pos]
    cos_sim = pos_track_data @ pos_track_data.t()
    inst_eq = (pos_ids_t.view(-1, 1) == pos_ids_t.view(1, -1)).float()
    cur_weights = torch.cat(per_img)
    loss_weights = cur_weights.view(-1, 1) @ cur_weights.view(1, -1)
    loss_weights.triu_(diagonal=1)
    cos_sim = (cos_sim + 1) / 2
    cos_sim.triu_(diagonal=1)
    cos_sim_diff = torch.clamp(1 - cos_sim, min=1e-10)
    loss_m = -1 * (inst_eq * torch.clamp(cos_sim, min=1e-10).log() + (1 - inst_eq) * cos_sim_diff.log())
    loss_m.triu_(diagonal=1)
    return (loss_m * loss_weights).sum() * AT / loss_weights.sum()


def case(B, reps, emit):
    g = torch.Generator().manual_seed(B)
    pri = torch.cat([0.1 + 0.8 * torch.rand(P, 2, generator=g), 0.05 + 0.35 * torch.rand(P, 2, generator=g)], -1)
    loc = torch.randn(B, P, 4, generator=g) * torch.tensor([1.0, 1.0, 0.8, 0.8])
    gc = pri[None, :, :2] + 0.25 * pri[None, :, 2:] * torch.randn(B, P, 2, generator=g)
    gs = pri[None, :, 2:] * torch.exp(0.25 * torch.randn(B, P, 2, generator=g))
    gt = torch.cat([gc - gs / 2, gc + gs / 2], -1).cuda()
    cent = (1.2 * torch.randn(B, P, 1, generator=g)).cuda()
    track = F.normalize(torch.randn(B, P, D, generator=g), dim=-1).cuda()
    ids = torch.randint(1, N_IDS + 1, (B, P), generator=g).cuda()
    conf_t = torch.zeros(B, P, dtype=torch.int64)
    for b in range(B):
        perm = torch.randperm(P, generator=g)
        conf_t[b, perm[:NPOS]] = torch.randint(1, 41, (NPOS,), generator=g)
        conf_t[b, perm[NPOS:NPOS + NNEU]] = -1
    conf_t, loc = conf_t.cuda(), loc.cuda()
    priors_b = pri[None].repeat(B, 1, 1).cuda()            # the reference indexes priors [B,P,4] with pos
    pri = pri.cuda()

    def box(fn, priors):
        l, c = loc.detach().requires_grad_(), cent.detach().requires_grad_()
        biou, center = fn(l, priors, gt, conf_t, c)
        (biou + center).backward()
        return biou, center, l.grad, c.grad

    def trk(fn):
        x = track.detach().requires_grad_()
        loss = fn(x, conf_t, ids)
        loss.backward()
        return loss, x.grad

    paths = {
        "box / centerness": (lambda: box(lambda l, p, g_, t, c: layers.box_center_loss(l, p, g_, t, c, AB, AC), pri),
                             lambda: box(torch_box_chain, priors_b)),
        "track loss      ": (lambda: trk(lambda x, t, i: layers.track_loss(x, t, i, AT)), lambda: trk(torch_track_chain)),
    }
    tag = f"B={B:<2d}"
    rows = []
    for what, (kern, chain) in paths.items():
        rk, rt = kern(), chain()
        diffs = "  ".join(f"{float((a - b).abs().max()):.2e}" for a, b in zip(rk, rt))
        emit(f"  {tag}  {what}  n = {B * NPOS}  max |kernels - torch chain| over (losses, gradients): {diffs}")
        t_k, t_t = timed(kern, reps), timed(chain, reps)
        m_k, m_t = peak_mb(kern), peak_mb(chain)
        s_k, s_t = host_syncs(kern), host_syncs(chain)
        emit(f"  {tag}  {what}  forward + backward   kernels {t_k:9.1f} us   torch chain {t_t:9.1f} us   ({t_t / t_k:.2f}x)" +
             ("" if t_k <= t_t else "   KERNELS SLOWER"))
        emit(f"  {tag}  {what}  max_memory_allocated kernels {m_k:9.1f} MB   torch chain {m_t:9.1f} MB")
        emit(f"  {tag}  {what}  host synchronisations kernels {s_k:8d}      torch chain {s_t:9d}")
        rows.append((what, kern, chain))
    return tag, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pos_losses.py needs the GPU: no timing is taken on a CPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# positive-prior loss terms, forward + backward, P = {P}, D = {D}, {NPOS} positives and {NNEU} neutrals per image, "
         f"{torch.cuda.get_device_name(0)}, median of 5 x {a.reps} calls")
    kept = [case(B, a.reps, emit) for B in (2, 8, 32)]
    for tag, rows in kept:                                  # last: the profiler slows the host, and nothing timed comes after it
        for what, kern, chain in rows:
            try:
                emit(f"  {tag}  {what}  device launches (kernels and copies) kernels {device_launches(kern):5d}   torch chain {device_launches(chain):5d}")
            except Exception as exc:                        # noqa: BLE001
                emit(f"  {tag}  {what}  device launches: not measured ({type(exc).__name__}: {exc})")


if __name__ == "__main__":
    main()
