"""The OHEM class-confidence loss (the reference's ohem_conf_loss over select_neg_bboxes, multibox_loss.py:402-448) forward + backward on one
MI355X at the training shape, next to a torch-op restatement of the reference's chain on the same card in the same process.

Shape: P = 15 345 priors, C = 41 classes, B = 2 / 8 / 32 images with 75 positives and 12 neutrals per image (about 600 and 100 at B = 8), logits
2 * randn.  Two whole paths are timed, each forward + backward with autograd from the leaf to .grad:
  kernels   layers.ohem_conf_loss (csrc/conf_loss.hip): 8 launches forward, 1 backward, no host synchronisation
  torch     the reference's chain as torch ops on the device: positives' weights, log_sum_exp with the global maximum, four masked writes, the
            full descending sort of all B * P scores, scatter, boolean gather of the kept rows, F.cross_entropy, autograd -- with the host
            round trips the reference has (num_neg as a slice bound, the boolean gather, torch.ones(num_neg))
with torch.cuda.max_memory_allocated of each path (a fresh peak counter per path; the inputs are allocated before it is reset and are included).
Then the device form's parts alone (ops.*, no autograd) with their algorithmic bytes against the HBM peak (8 TB/s):
  forward   4 N C + 8 N                  the logits and the labels read once (the [N] vectors in between are 4 N each and stay in the caches)
  select    the same, 7 of the 8 launches
  adjoint   4 N C + 4 C * (kept rows)    the gradient written once, the logits read for the kept rows only
Each figure: HIP events around `--reps` back-to-back calls after a warm-up, median of 5 groups.
Usage: python scripts/bench_conf_loss.py [--reps 10] [--out FILE]
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

P, C, RATIO, ALPHA = 15345, 41, 3, 6.125
HBM_GBS = 8000.0


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


def torch_chain(conf_data, conf_t):
    B = conf_t.size(0)
    pos = conf_t > 0
    num_pos_per_img = [pos[i].sum().long() for i in range(B)]
    split = torch.ones(int(pos.sum().tolist()), device=conf_data.device).split(num_pos_per_img)
    pos_weights = torch.cat([cur / torch.clamp(cur.sum(), min=1) for cur in split], dim=0)
    conf_t = conf_t.view(-1)
    conf_data = conf_data.view(-1, C)
    pos = (conf_t > 0).float()
    x_max = conf_data.data.max()
    loss_c = torch.log(torch.sum(torch.exp(conf_data - x_max), 1)) + x_max - conf_data[:, 0]
    num_pos = (conf_t > 0).sum()
    num_neg = torch.clamp(RATIO * num_pos, max=conf_t.size()[0] - 1)
    loss_c[conf_t > 0] = 0
    loss_c[conf_t < 0] = 0
    _, loss_idx = loss_c.sort(descending=True)
    neg = torch.zeros(conf_t.size(), device=conf_t.device)
    neg[loss_idx[:num_neg]] = 1
    neg[conf_t > 0] = 0
    neg[conf_t < 0] = 0
    keep = (pos + neg).gt(0)
    use_conf_t = conf_t[keep]
    use_conf_data = conf_data[keep]
    num_neg = (neg > 0).sum()
    neg_weights = torch.ones(num_neg, device=pos_weights.device) / num_neg * RATIO * B
    loss_weights = torch.cat([pos_weights, neg_weights])
    loss = F.cross_entropy(use_conf_data, use_conf_t, reduction="none")
    return ALPHA * (loss_weights * loss).sum() / (RATIO + 1)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 1e6


def case(B, reps, emit):
    g = torch.Generator().manual_seed(B)
    conf = (2 * torch.randn(B, P, C, generator=g)).cuda()
    conf_t = torch.zeros(B, P, dtype=torch.int64)
    for b in range(B):
        perm = torch.randperm(P, generator=g)
        conf_t[b, perm[:75]] = torch.randint(1, C, (75,), generator=g)
        conf_t[b, perm[75:87]] = -1
    conf_t = conf_t.cuda()
    N = B * P

    def whole(fn):
        x = conf.detach().requires_grad_()
        loss = fn(x, conf_t)
        loss.backward()
        return loss, x.grad

    kernels = lambda x, t: layers.ohem_conf_loss(x, t, RATIO, ALPHA)      # noqa: E731
    lk, gk = whole(kernels)
    lt, gt = whole(torch_chain)
    tag = f"B={B:<2d}"
    emit(f"  {tag}  loss kernels {float(lk):.6f}  torch chain {float(lt):.6f}  max |grad difference| {float((gk - gt).abs().max()):.2e}")
    t_k = timed(lambda: whole(kernels), reps)
    t_t = timed(lambda: whole(torch_chain), reps)
    m_k, m_t = peak_mb(lambda: whole(kernels)), peak_mb(lambda: whole(torch_chain))
    emit(f"  {tag}  forward + backward   kernels {t_k:9.1f} us   torch chain {t_t:9.1f} us   ({t_t / t_k:.2f}x)" +
         ("" if t_k <= t_t else "   KERNELS SLOWER"))
    emit(f"  {tag}  max_memory_allocated kernels {m_k:9.1f} MB   torch chain {m_t:9.1f} MB")
    loss, lse, w = ops.ohem_conf_loss(conf, conf_t, RATIO, ALPHA)
    kept = int((w != 0).sum())
    one = torch.ones((), device="cuda")
    fb = 4 * N * C + 8 * N
    bb = 4 * N * C + 4 * C * kept
    t_f = timed(lambda: ops.ohem_conf_loss(conf, conf_t, RATIO, ALPHA), reps)
    t_s = timed(lambda: ops.ohem_select_neg(conf, conf_t, RATIO), reps)
    t_b = timed(lambda: ops.ohem_conf_loss_backward(one, conf, conf_t, lse, w, RATIO, ALPHA), reps)
    for what, t, nb, note in (("forward ", t_f, fb, "8 launches"), ("select  ", t_s, fb, "7 launches"), ("adjoint ", t_b, bb, f"1 launch, {kept} kept rows")):
        emit(f"  {tag}  {what}            {t:9.1f} us  {nb / 1e6:7.2f} MB  {nb / t / 1e3:7.1f} GB/s  {100 * nb / t / 1e3 / HBM_GBS:5.1f} % of HBM peak   ({note})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conf_loss.py needs the GPU: no timing is taken on a CPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# OHEM class-confidence loss, forward + backward, P = {P}, C = {C}, negpos_ratio = {RATIO}, 75 positives and 12 neutrals per image, "
         f"{torch.cuda.get_device_name(0)}, median of 5 x {a.reps} calls")
    for B in (2, 8, 32):
        case(B, a.reps, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
