"""One image's mask loss (the reference's lincomb_mask_loss, multibox_loss.py:594-616) forward + backward on one MI355X at a training shape, next to
the reference's fp32 torch op chain on the same card.

Shape: 96x160 prototypes, M = 32, 384x640 targets (x4), G = 8 byte targets, n = 20 / 100 / 300 positives (boxes of 5-45 % of each frame side).
Two whole paths are timed, each forward + backward with autograd from leaves to .grad:
  kernels   layers.lincomb_mask_loss_image: generate_mask, mask_bce_sum (csrc/mask_loss.hip), box normalisation, weighted sum
  torch     generate_mask as torch ops (tanh, matmul, sigmoid, crop, permute), masks_gt[idx].float(), F.interpolate, clamp, F.binary_cross_entropy,
            sum, normalise -- the reference's chain, fp32
with torch.cuda.max_memory_allocated of each path (a fresh peak counter per path; the inputs are allocated before it is reset and are included),
and the two new launches alone (ops.*, no autograd), with algorithmic bytes:
  forward   4 n h w + n H W                 every prediction and every target byte of every instance read once
  adjoint   4 n h w + n H W + 4 n h w       the same, plus the gradient written
Each figure: HIP events around `--reps` back-to-back calls after a warm-up, median of 5 groups.
Usage: python scripts/bench_mask_loss.py [--reps 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stmask_amd import layers, ops  # noqa: E402
from stmask_amd.layers import box_utils  # noqa: E402

h, w, M, SCALE, G = 96, 160, 32, 4, 8
H, W = h * SCALE, w * SCALE


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


def torch_chain(proto, coeff, boxes, masks_gt, idx, weights):
    m = torch.sigmoid(proto @ torch.tanh(coeff).t())
    _, m = box_utils.crop(m, boxes)
    pred = m.permute(2, 0, 1).contiguous()
    mask_t = masks_gt[idx].float()
    up = F.interpolate(pred.unsqueeze(0), (H, W), mode="bilinear", align_corners=False).squeeze(0)
    pre = F.binary_cross_entropy(torch.clamp(up, 0, 1), mask_t, reduction="none")
    bw = torch.clamp((boxes[:, 2] - boxes[:, 0]) * W, min=1)
    bh = torch.clamp((boxes[:, 3] - boxes[:, 1]) * H, min=1)
    return torch.sum(weights * (pre.sum(dim=(1, 2)) / bw / bh))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 1e6


def case(n, reps, emit):
    dev = "cuda"
    g = torch.Generator().manual_seed(n)
    proto = (torch.relu(torch.randn(h, w, M, generator=g)) * 0.2).to(dev)
    coeff = torch.randn(n, M, generator=g).to(dev)
    c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(n, 2, generator=g) * 0.4 + 0.05
    boxes = torch.cat((c - wh / 2, c + wh / 2), 1).to(dev)
    masks_gt = torch.randint(0, 2, (G, H, W), generator=g, dtype=torch.uint8).to(dev)
    idx = torch.randint(0, G, (n,), generator=g).to(dev)
    weights = (torch.rand(n, generator=g) + 0.5).to(dev)

    def whole(fn):
        p, q = proto.detach().requires_grad_(), coeff.detach().requires_grad_()
        fn(p, q, boxes, masks_gt, idx, weights).backward()

    tag = f"n={n:<3d}"
    t_k = timed(lambda: whole(layers.lincomb_mask_loss_image), reps)
    t_t = timed(lambda: whole(torch_chain), reps)
    m_k, m_t = peak_mb(lambda: whole(layers.lincomb_mask_loss_image)), peak_mb(lambda: whole(torch_chain))
    emit(f"  {tag}  forward + backward   kernels {t_k:9.1f} us   torch chain {t_t:9.1f} us   ({t_t / t_k:.2f}x)" +
         ("" if t_k <= t_t else "   KERNELS SLOWER"))
    emit(f"  {tag}  max_memory_allocated kernels {m_k:9.1f} MB   torch chain {m_t:9.1f} MB")
    pred = ops.lincomb_sigmoid_crop(proto, coeff, boxes)
    gl = weights.clone()
    fb = 4 * n * h * w + n * H * W
    bb = fb + 4 * n * h * w
    t_f = timed(lambda: ops.mask_bce_upsampled(pred, masks_gt, idx), reps)
    t_b = timed(lambda: ops.mask_bce_upsampled_backward(gl, pred, masks_gt, idx), reps)
    emit(f"  {tag}  mask_bce forward     {t_f:9.1f} us  {fb / 1e6:7.2f} MB  {fb / t_f / 1e3:7.1f} GB/s   (2 launches: tiles, then the per-instance sum)")
    emit(f"  {tag}  mask_bce adjoint     {t_b:9.1f} us  {bb / 1e6:7.2f} MB  {bb / t_b / 1e3:7.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_loss.py needs the GPU: no timing is taken on a CPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# lincomb mask loss of one image, forward + backward, {h}x{w} prototypes -> {H}x{W} targets, M = {M}, G = {G}, "
         f"{torch.cuda.get_device_name(0)}, median of 5 x {a.reps} calls")
    for n in (20, 100, 300):
        case(n, a.reps, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
