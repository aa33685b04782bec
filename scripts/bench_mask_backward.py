"""generate_mask forward + backward on one MI355X at a training shape, next to the same fp32 torch op chain on the same card.

Shape: 96x160 prototypes, M = 32, n = 20 / 100 / 300 positives, with and without crop (boxes of 5-45 % of each frame side, as a training batch's
positives).  Two whole paths are timed, each forward + backward with autograd from leaves to .grad:
  kernels   layers.generate_mask (stm_lincomb_sigmoid_crop_f32, then stm_lincomb_backward_f32 through autograd.LincombMaskFunction)
  torch     tanh, matmul, sigmoid, layers.crop, permute + contiguous -- the reference's chain (layers/mask_utils.py:111-128), fp32
and the launches alone (ops.*, no autograd), with algorithmic bytes (fp32; A = pixels inside the crop rectangles, n*h*w without crop):
  forward   4*(h*w*M + n*M + n*h*w)                prototypes and coefficients read, every mask pixel written
  backward  4*(2*h*w*M + 2*n*M + A)                prototypes, coefficients and grad_out inside the rectangles read; both gradients written
  (the backward's partial sums -- [pixel block][n][M] and, when rows are split, [split][h*w][M] -- are not algorithmic bytes)
`--splits` also times the backward with the row split forced to 1 (STM_LCB_SPLITS): the measurement behind the split rule of
csrc/lincomb_backward.hip.  Each figure: HIP events around `--reps` back-to-back calls after a warm-up, median of 5 groups.
Usage: python scripts/bench_mask_backward.py [--reps 20] [--splits] [--out FILE] [--once]     (--once: one pass per shape, for a profiler run)
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stmask_amd import _lib, layers, ops  # noqa: E402
from stmask_amd.layers import box_utils  # noqa: E402

H, W, M = 96, 160, 32


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


def torch_chain(proto, coeff, boxes):
    m = torch.sigmoid(proto @ torch.tanh(coeff).t())
    if boxes is not None:
        _, m = box_utils.crop(m, boxes)
    return m.permute(2, 0, 1).contiguous()


def case(n, crop, reps, splits, emit):
    dev = "cuda"
    g = torch.Generator().manual_seed(n)
    proto = torch.relu(torch.randn(H, W, M, generator=g)).to(dev)
    coeff = torch.randn(n, M, generator=g).to(dev)
    c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(n, 2, generator=g) * 0.4 + 0.05
    boxes = torch.cat((c - wh / 2, c + wh / 2), 1).to(dev) if crop else None
    go = torch.randn(n, H, W, generator=g).to(dev)
    inside = int(box_utils.crop(torch.ones(H, W, n, device=dev), boxes)[0].sum().item()) if crop else n * H * W

    def whole(fn):
        p, q = proto.detach().requires_grad_(), coeff.detach().requires_grad_()
        fn(p, q, boxes).backward(go)

    tag = f"n={n:<3d} {'crop   ' if crop else 'no crop'}"
    t_k = timed(lambda: whole(layers.generate_mask), reps)
    t_t = timed(lambda: whole(torch_chain), reps)
    emit(f"  {tag}  forward + backward   kernels {t_k:8.1f} us   torch chain {t_t:8.1f} us   ({t_t / t_k:.2f}x)" +
         ("" if t_k <= t_t else "   KERNELS SLOWER"))
    fb, bb = 4 * (H * W * M + n * M + n * H * W), 4 * (2 * H * W * M + 2 * n * M + inside)
    t_f = timed(lambda: ops.lincomb_sigmoid_crop(proto, coeff, boxes), reps)
    t_b = timed(lambda: ops.lincomb_sigmoid_crop_backward(go, proto, coeff, boxes), reps)
    emit(f"  {tag}  lincomb forward      {t_f:8.1f} us  {fb / 1e6:7.2f} MB  {fb / t_f / 1e3:7.1f} GB/s")
    emit(f"  {tag}  lincomb backward     {t_b:8.1f} us  {bb / 1e6:7.2f} MB  {bb / t_b / 1e3:7.1f} GB/s   (both gradients; 3 launches when rows are split)")
    for np_, nc, what in ((True, False, "grad_proto only"), (False, True, "grad_coeff only")):
        t = timed(lambda: ops.lincomb_sigmoid_crop_backward(go, proto, coeff, boxes, need_proto=np_, need_coeff=nc), reps)
        emit(f"  {tag}  lincomb backward     {t:8.1f} us   {what}")
    if splits:
        os.environ["STM_LCB_SPLITS"] = "1"
        _lib.lib().stm_debug_reload_tunables()
        t1 = timed(lambda: ops.lincomb_sigmoid_crop_backward(go, proto, coeff, boxes), reps)
        del os.environ["STM_LCB_SPLITS"]
        _lib.lib().stm_debug_reload_tunables()
        emit(f"  {tag}  lincomb backward     {t1:8.1f} us   rows not split over workgroups (60 workgroups)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--splits", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_backward.py needs the GPU: no timing is taken on a CPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.once:
        for n in (20, 100, 300):
            for crop in (True, False):
                g = torch.Generator().manual_seed(n)
                proto = torch.relu(torch.randn(H, W, M, generator=g)).cuda().requires_grad_()
                coeff = torch.randn(n, M, generator=g).cuda().requires_grad_()
                c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
                wh = torch.rand(n, 2, generator=g) * 0.4 + 0.05
                boxes = torch.cat((c - wh / 2, c + wh / 2), 1).cuda() if crop else None
                for _ in range(5):
                    layers.generate_mask(proto, coeff, boxes).backward(torch.ones(n, H, W, device="cuda"))
        torch.cuda.synchronize()
        return
    emit(f"# generate_mask forward + backward, {H}x{W} prototypes, M = {M}, {torch.cuda.get_device_name(0)}, median of 5 x {a.reps} calls")
    for n in (20, 100, 300):
        for crop in (True, False):
            case(n, crop, a.reps, a.splits, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
