"""Backward kernels of the drop-ins on one MI355X: us per launch and achieved GB/s (algorithmic bytes in the style of SURVEY.md section 8(d)).

Shapes: the 7 R50 DCN layers at batch 8 (384x640 frames, fused conv_offset_mask input as DCN feeds it), FCB's DeformConv2d 3x3 / 3x5 / 5x3 on the
256-channel 48x80 level at batch 8, RoIAlign of 100 RoIs x 7x7 on a 256-channel 48x80 map, correlation P = 11 on 48x80x256.  Each launch is timed
alone with HIP events around `--reps` back-to-back launches after a warm-up, median of 5 groups.  The accumulating scatters (col2im, RoIAlign) add
into the same buffer every launch, which changes no traffic.

Algorithmic bytes (fp32, per launch; K taps, P = 3K (DCN) or 2K (v1) offset + mask channels per group, HWo output positions):
  im2col (recompute)   4*B*(C*H*W + P*HWo + C*K*HWo)            -- SURVEY 8(d)
  col2im               4*B*(C*K*HWo + P*HWo + C*H*W)            grad_cols and offsets read, grad_x written once
  col2im_coord         4*B*(C*K*HWo + C*H*W + P*HWo + P*HWo)    grad_cols, x, offsets read; grad_offset + grad_mask written
  gemms                TFLOP/s: 2*O*C*K*B*HWo flops each (grad_cols = W^T grad_out; grad_weight incl. its two layout copies)
  roi_align_backward   4*(n*C*PH*PW + C*H*W)                    grad_out read, grad_feat written
  corr_backward        4*(P*P*H*W + 2*C*H*W) per input gradient
Usage: python scripts/bench_backward.py [--reps 20] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stmask_amd import ops  # noqa: E402
from stmask_amd._lib import c_p, call  # noqa: E402

R50 = [("L1.0", 128, 96, 160, 2), ("L1.2", 128, 48, 80, 1), ("L2.0", 256, 48, 80, 2), ("L2.2", 256, 24, 40, 1), ("L2.4", 256, 24, 40, 1),
       ("L3.0", 512, 24, 40, 2), ("L3.2", 512, 12, 20, 1)]


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


def deform_layer(name, B, C, H, W, kh, kw, stride, pad, fused, reps, out):
    dev = "cuda"
    g = ops._geom(torch.empty(B, C, H, W, device="meta"), (kh, kw), stride, pad, 1, 1)
    K, HWo = kh * kw, g.Ho * g.Wo
    CK = C * K
    x = torch.randn(B, C, H, W, device=dev)
    if fused:
        om = torch.randn(B, 3 * K, g.Ho, g.Wo, device=dev)
        off, mask, P = None, None, 3 * K
    else:
        om, off, mask, P = None, torch.randn(B, 2 * K, g.Ho, g.Wo, device=dev), None, 2 * K
    w = torch.randn(C, C, kh, kw, device=dev) * 0.02
    go = torch.randn(B, C, g.Ho, g.Wo, device=dev)
    cols = torch.empty(B, CK, HWo, device=dev)
    gcols = torch.randn(B, CK, HWo, device=dev)
    gx = torch.zeros_like(x)
    o_t, obs, _, mk_ptr, mbs = ops._offset_mask_views(off, mask, g, om)
    logit = 1 if fused else 0
    goff = torch.empty(B, P, g.Ho, g.Wo, device=dev)
    wT = w.view(C, CK).t().contiguous()
    gemm_flops = 2.0 * C * CK * B * HWo
    rows = []

    def im2col():
        ops.deform_im2col(x, off, mask, (kh, kw), stride, pad, 1, 1, fused_om=om, out=cols)

    def grad_weight():
        a = cols.permute(1, 0, 2).reshape(CK, B * HWo).contiguous()
        bm = go.view(B, C, HWo).permute(0, 2, 1).reshape(B * HWo, C).contiguous()
        ops.gemm_bias(a, bm)

    def grad_cols():
        ops.gemm_bias(wT, go.view(B, C, HWo))

    def col2im():
        call("stm_deform_col2im_f32", ops._p(gcols), ops._p(o_t), obs, c_p(mk_ptr), mbs, logit, ops._p(gx), ctypes.byref(g), ops._stream())

    def coord():
        gm_ptr = c_p(goff.data_ptr() + 4 * 2 * K * HWo) if P == 3 * K else c_p(0)
        call("stm_deform_col2im_coord_f32", ops._p(gcols), ops._p(x), ops._p(o_t), obs, c_p(mk_ptr), mbs, logit, ops._p(goff), P * HWo, gm_ptr,
             P * HWo, ctypes.byref(g), ops._stream())

    def whole():
        ops.deform_conv_backward(go, x, off, mask, w, stride, pad, 1, 1, fused_om=om)

    parts = [("im2col (recompute)", im2col, 4.0 * B * (C * H * W + P * HWo + CK * HWo), None),
             ("grad_weight gemm + copies", grad_weight, None, gemm_flops),
             ("grad_cols gemm", grad_cols, None, gemm_flops),
             ("col2im (atomic)", col2im, 4.0 * B * (CK * HWo + P * HWo + C * H * W), None),
             ("col2im_coord", coord, 4.0 * B * (CK * HWo + C * H * W + 2 * P * HWo), None)]
    total = 0.0
    for pname, fn, nbytes, flops in parts:
        us = timed(fn, reps)
        total += us
        rate = f"{nbytes / us / 1e3:8.1f} GB/s" if nbytes else f"{flops / us / 1e6:8.1f} TFLOP/s"
        rows.append((pname, us))
        out(f"  {name:<12} {pname:<26} {us:9.1f} us  {rate}")
    us = timed(whole, max(2, reps // 4))
    top = max(rows, key=lambda r: r[1])
    out(f"  {name:<12} {'whole backward (ops)':<26} {us:9.1f} us  (parts sum {total:.1f}; largest: {top[0]}, {100 * top[1] / total:.0f} %)")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    out(f"# backward kernels of the drop-ins, {torch.cuda.get_device_name(0)}, median of 5 x {args.reps} launches")
    out("## DCN (dcn_v2.DCN, fused conv_offset_mask input), R50 layers at batch 8")
    share = {}
    for name, C, H, W, s in R50:
        for pname, us in deform_layer(name, 8, C, H, W, 3, 3, s, 1, True, args.reps, out):
            share[pname] = share.get(pname, 0.0) + us
    tot = sum(share.values())
    out("  all 7 layers: " + ", ".join(f"{k} {v:.0f} us ({100 * v / tot:.0f} %)" for k, v in sorted(share.items(), key=lambda kv: -kv[1])))
    out("## FCB DeformConv2d (v1, no mask), C = 256, 48x80, batch 8")
    for kh, kw in ((3, 3), (3, 5), (5, 3)):
        deform_layer(f"{kh}x{kw}", 8, 256, 48, 80, kh, kw, 1, (kh // 2, kw // 2), False, args.reps, out)
    out("## RoIAlign backward: 100 RoIs x 7x7, 256 x 48 x 80, sampling_ratio 0")
    C, H, W, n = 256, 48, 80, 100
    g = torch.Generator().manual_seed(1)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([W * 0.7, H * 0.7])
    wh = torch.rand(n, 2, generator=g) * torch.tensor([W * 0.3, H * 0.3]) + 1
    rois = torch.cat([torch.zeros(n, 1), xy, xy + wh], 1).cuda()
    go = torch.randn(n, C, 7, 7, device="cuda")
    gfeat = torch.zeros(1, C, H, W, device="cuda")

    def roi():
        call("stm_roi_align_backward_f32", ops._p(go), ops._p(rois), ops._p(gfeat), 1, C, H, W, n, 7, 7, 1.0, 0, 1, ops._stream())
    us = timed(roi, args.reps)
    out(f"  roi_align_backward         {us:9.1f} us  {4.0 * (n * C * 49 + C * H * W) / us / 1e3:8.1f} GB/s")
    out("## correlation backward: P = 11, 256 x 48 x 80, batch 1")
    P = 11
    f1, f2 = torch.randn(1, C, H, W, device="cuda"), torch.randn(1, C, H, W, device="cuda")
    gc = torch.randn(1, P, P, H, W, device="cuda")
    g1, g2 = torch.empty_like(f1), torch.empty_like(f2)
    for label, a, b in (("grad_in1", g1, None), ("grad_in2", None, g2)):
        def corr(a=a, b=b):
            call("stm_corr_backward_f32", ops._p(gc), ops._p(f1), ops._p(f2), ops._p(a), ops._p(b), 1, C, H, W, P, 1, ops._stream())
        us = timed(corr, args.reps)
        out(f"  corr_backward {label:<12} {us:9.1f} us  {4.0 * (P * P * H * W + 2 * C * H * W) / us / 1e3:8.1f} GB/s")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
