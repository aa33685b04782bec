#!/usr/bin/env python3
"""The shared head's stages timed alone on the benchmark's tensors (32 clips, eager, HIP events, nothing beside them): the eager trunk with
the dense and the sparse head, then each launch group of PlanarGraph._sparse_head and of the dense head (best of four passes).
Wrote profiles/sparse_head_stages.txt and, run with STM_HEAD_CENTER / STM_HEAD_SPLIT / STM_HEAD_SHAPES = 0 and 1 by scripts/ab_head_switch.sh,
profiles/head_center_stages.txt / profiles/head_split_stages.txt / profiles/head_shapes_stages.txt.  Also prints the shape mix of the listed
(position, kernel shape) entries, which the shapes form's gain follows from.
usage: [STM_HEAD_CENTER=0] [STM_HEAD_SPLIT=0] [STM_HEAD_SHAPES=0] bench_sparse_head_stages.py > profiles/sparse_head_stages.txt"""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import bench
from benchlib.runner import build_net, Runner
from stmask_amd import ops, planar

args = bench.parse_args([])
B = 32
dev = torch.device("cuda:0")
net = build_net(args, dev)
r = Runner(args, dev, 0, 1, B, net=net)
x = r.frames_t[1]
pg = net._planar
sizes = [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]
ntot = sum(B * h * w for h, w in sizes)

# whole trunk, eager, dense vs sparse
def trunk(sparse, n=8):
    pg.sparse = sparse
    with torch.no_grad():
        for _ in range(3):
            net.forward_single(x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            net.forward_single(x)
        e1.record()
    torch.cuda.synchronize()
    pg.sparse = None
    return e0.elapsed_time(e1) / n
thr = net.cfg.eval_conf_thresh
print("trunk eager ms: dense", trunk(None), "sparse", trunk((thr, None)), "dense", trunk(None), "sparse", trunk((thr, None)), flush=True)

# stages of the sparse head on the `up` planes of this frame
cap = {}
orig_up = pg.up.__call__
ups = []
class Grab:
    pass
orig = planar.PlanarConv.__call__
def grab(self, *a, **kw):
    y = orig(self, *a, **kw)
    if self is pg.up:
        ups.append(y)
    return y
planar.PlanarConv.__call__ = grab
with torch.no_grad():
    net.forward_single(x)
planar.PlanarConv.__call__ = orig
up = ups[0][1] if isinstance(ups[0], tuple) else ups[0]
lv = ("levels", B, sizes)
t1c, t1r, t2c, t2r, cls_l, small_l = pg._build_sparse()
trk_l = [f.trk for f in pg.finals]
cw, P = 256, 64
NP, pdt = ops.plane_layout(pg.fmt)
capn = pg.sparse_capacity(B, sizes)
head = pg.head
CENTER = planar.head_center_default()      # STM_HEAD_CENTER=0: the output layers over all 25 pixels of each patch map
SPLIT = planar.head_split_default()        # STM_HEAD_SPLIT=0: the mask and track branches at every listed position
OWN = ops.HEAD_CTL_OWN if SPLIT else 0
SHAPES = planar.head_shapes_default() and SPLIT and CENTER and pg.fmt == 1      # STM_HEAD_SHAPES=0: the towers over the whole maps of every listed pixel
print("output layers at the centre pixel only:", CENTER, " mask / track branches at the own positions only:", SPLIT,
      " towers over each entry's kernel footprint:", SHAPES)
K, SEG = len(pg.finals), ops.HEAD_CTL_SEG
SHP = [(c.kh, c.kw) for c in small_l]
W1 = [(kh + 2, kw + 2, (5 - kh) // 2, (5 - kw) // 2) for kh, kw in SHP]
W2 = [(kh, kw, (5 - kh) // 2, (5 - kw) // 2) for kh, kw in SHP]
segn = pg.sparse_segment_capacity(capn)
# the other form of the split head's cen+bbox | mask output layers: two single-group launches per kernel shape (cen+bbox over all positions, mask
# over the own ones) instead of one grouped launch over all positions -- timed beside it, not used by PlanarGraph._sparse_head
def cut_group(sm, g):
    c = planar.PlanarConv(sm.weight[g * P:(g + 1) * P], sm.bias[g * P:(g + 1) * P], 1, (sm.ph, sm.pw), relu=False, fmt=sm.fmt, tile_n=64,
                          group_cout=sm.group_cout[g:g + 1], algo_frac=sm.group_cout[g] / float(P))
    c.wscale = ops._pow2_wscale(sm.weight) if sm.fmt >= 1 else None
    return c
small_1g = [(cut_group(c, 0), cut_group(c, 1)) for c in small_l] if SPLIT and CENTER else []
stages = []
def ev():
    e = torch.cuda.Event(enable_timing=True); e.record(); return e
def shapes_rest(cls, m):
    # PlanarGraph._sparse_patches_shapes from the candidates on: entries in one segment per kernel shape, the towers as gated window sets
    lst, ctl = ops.head_candidates(cls, head.num_classes, thr, segn, [h * w for h, w, _, _ in W1], [h * w for h, w, _, _ in W2], B, sizes, split=True, shapes=True); m("candidates")
    tot = K * segn
    patch = ops.head_patch_gather(up, torch.empty(NP, cw // 32, tot * 81, 32, device=dev, dtype=pdt), 9, segn, B, sizes, lst, ctl, segs=K); m("gather 9x9")
    x1 = torch.empty(NP, 3 * cw // 32, tot * 49, 32, device=dev, dtype=pdt)
    xq = torch.empty(NP, 3 * cw // 32, tot * 25, 32, device=dev, dtype=pdt)
    t1b, t1m, t2b, t2m = pg._split_layers
    t1b.window_segments(patch, tot, 9, 9, W1, x1, 7, (ctl, SEG + 3)); m("t1 patches bbox")
    t1m.window_segments(patch, tot, 9, 9, W1, x1, 7, (ctl, SEG + OWN + 3), out_slab_off=cw // 32); m("t1 patches mask+track")
    ops.head_patch_mask(x1, 7, segn, B, sizes, lst, ctl, segs=K); m("mask 7")
    t2b.window_segments(x1, tot, 7, 7, W2, xq, 5, (ctl, SEG + 4)); m("t2 patches bbox")
    t2m.window_segments(x1, tot, 7, 7, W2, xq, 5, (ctl, SEG + OWN + 4), x_ch_off=cw, out_slab_off=cw // 32); m("t2 patches mask+track")
    ops.head_patch_mask(xq, 5, segn, B, sizes, lst, ctl, segs=K); m("mask 5")
    def centre(c, k, blk, **kw):
        return c(xq, ("img", segn, 5, 5), x_off=k * segn * 25, out="f32", out_f32=torch.empty(segn, c.O, device=dev),
                 window=(0, 0, 1, 1, c.ph - 2, c.pw - 2, 1, 1), gate=(ctl, SEG * (k + 1) + blk + ops.HEAD_CTL_GATE_POS), **kw)
    small = [centre(c, k, 0, kxr=True) for k, c in enumerate(small_l)]; m("small patches x3")
    trk = [centre(c, k, OWN, x_ch_off=2 * cw, kxr=False) for k, c in enumerate(trk_l)]; m("trk patches x3")
    gd = (ctl, 5)
    xx = t1r(up, lv, out="planes", gate=gd); xx = t2r(xx, lv, out="planes", gate=gd); m("dense towers (empty)")
    small_d = [c(xx, lv, out="f32", gate=gd, kxr=True) for c in small_l]
    trk_d = [c(xx, lv, out="f32", x_ch_off=2 * cw, gate=gd) for c in trk_l]; m("dense outputs (empty)")
    ops.head_assemble_sparse(cls, small, trk, small_d, trk_d, B, sizes, head.num_classes, head.mask_dim, head.embed_dim, P, 1, 0, lst, ctl, segn, split=True, shapes=True); m("assemble")
    return ctl
def run_once(record):
    marks = [("start", ev())]
    def m(name):
        marks.append((name, ev()))
    xx = t1c(up, lv, out="planes", splitk=False); m("t1 class")
    xx = t2c(xx, lv, out="planes", splitk=False); m("t2 class")
    cls = [c(xx, lv, out="f32", splitk=False, kxr=True) for c in cls_l]; m("class output layers x3")
    if SHAPES:
        ctl = shapes_rest(cls, m)
        torch.cuda.synchronize()
        if record:
            stages.append([(marks[i][0], marks[i - 1][1].elapsed_time(marks[i][1])) for i in range(1, len(marks))])
        return ctl.tolist()
    lst, ctl = ops.head_candidates(cls, head.num_classes, thr, capn, 49, 25, B, sizes, split=SPLIT); m("candidates")
    patch = ops.head_patch_gather(up, torch.empty(NP, cw // 32, capn * 81, 32, device=dev, dtype=pdt), 9, capn, B, sizes, lst, ctl); m("gather 9x9")
    x1 = torch.empty(NP, 3 * cw // 32, capn * 49, 32, device=dev, dtype=pdt)
    xq = torch.empty(NP, 3 * cw // 32, capn * 25, 32, device=dev, dtype=pdt)
    w1, w2 = (0, 0, 7, 7, 0, 0, 7, 7), (0, 0, 5, 5, 0, 0, 5, 5)
    if SPLIT:       # bbox towers over all listed patches, mask + track towers over the own ones
        t1b, t1m, t2b, t2m = pg._split_layers
        t1b(patch, ("img", capn, 9, 9), out="planes", out_planes=x1, window=w1, gate=(ctl, 3)); m("t1 patches bbox")
        t1m(patch, ("img", capn, 9, 9), out="planes", out_planes=x1, out_slab_off=cw // 32, window=w1, gate=(ctl, OWN + 3)); m("t1 patches mask+track")
    else:
        t1r(patch, ("img", capn, 9, 9), out="planes", out_planes=x1, window=w1, gate=(ctl, 3)); m("t1 patches")
    ops.head_patch_mask(x1, 7, capn, B, sizes, lst, ctl); m("mask 7")
    if SPLIT:
        t2b(x1, ("img", capn, 7, 7), out="planes", out_planes=xq, window=w2, gate=(ctl, 4)); m("t2 patches bbox")
        t2m(x1, ("img", capn, 7, 7), out="planes", out_planes=xq, x_ch_off=cw, out_slab_off=cw // 32, window=w2, gate=(ctl, OWN + 4)); m("t2 patches mask+track")
    else:
        t2r(x1, ("img", capn, 7, 7), out="planes", out_planes=xq, window=w2, gate=(ctl, 4)); m("t2 patches")
    ops.head_patch_mask(xq, 5, capn, B, sizes, lst, ctl); m("mask 5")
    if CENTER:      # one-pixel window launches at the centre of the 5 x 5 maps, one output row per position
        def centre(c, blk, **kw):
            return c(xq, ("img", capn, 5, 5), out="f32", out_f32=torch.empty(capn, c.O, device=dev), window=(0, 0, 1, 1, c.ph - 2, c.pw - 2, 1, 1),
                     gate=(ctl, blk + ops.HEAD_CTL_GATE_POS), **kw)
        small = [centre(c, 0, kxr=True) for c in small_l]; m("small patches x3")
        if small_1g:
            for cb, cm in small_1g:
                o = torch.empty(capn, 2 * P, device=dev)
                cb(xq, ("img", capn, 5, 5), out="f32", out_f32=o, window=(0, 0, 1, 1, cb.ph - 2, cb.pw - 2, 1, 1), gate=(ctl, ops.HEAD_CTL_GATE_POS), kxr=True)
                cm(xq, ("img", capn, 5, 5), out="f32", out_f32=o, out_ch_off=P, x_ch_off=cw, window=(0, 0, 1, 1, cm.ph - 2, cm.pw - 2, 1, 1),
                   gate=(ctl, OWN + ops.HEAD_CTL_GATE_POS), kxr=True)
            m("(small patches as 2 x 3 single-group launches, unused)")
        trk = [centre(c, OWN, x_ch_off=2 * cw, kxr=False) for c in trk_l]; m("trk patches x3")
    else:
        ql = ("levels", capn, [(5, 5)])
        small = [c(xq, ql, out="f32", gate=(ctl, 4), kxr=True) for c in small_l]; m("small patches x3")
        trk = [c(xq, ql, out="f32", x_ch_off=2 * cw, gate=(ctl, OWN + 4)) for c in trk_l]; m("trk patches x3")
    gd = (ctl, 5)
    xx = t1r(up, lv, out="planes", gate=gd); xx = t2r(xx, lv, out="planes", gate=gd); m("dense towers (empty)")
    small_d = [c(xx, lv, out="f32", gate=gd, kxr=True) for c in small_l]
    trk_d = [c(xx, lv, out="f32", x_ch_off=2 * cw, gate=gd) for c in trk_l]; m("dense outputs (empty)")
    out = ops.head_assemble_sparse(cls, small, trk, small_d, trk_d, B, sizes, head.num_classes, head.mask_dim, head.embed_dim, P, *((1, 0) if CENTER else (25, 12)), lst, ctl, capn, split=SPLIT); m("assemble")
    torch.cuda.synchronize()
    if record:
        stages.append([(marks[i][0], marks[i - 1][1].elapsed_time(marks[i][1])) for i in range(1, len(marks))])
        return ctl.tolist()
with torch.no_grad():
    for i in range(6):
        c = run_once(i >= 2)
print("ctl", c)
# the shape mix of this frame's entries (the candidate pass in the shapes form, whatever form is timed): entry (pixel, shape k) is OWN where prior
# (pixel, k) is kept, PARTNER-only where shape k's centerness at that pixel is read with a kept prior elsewhere
if pg.fmt == 1:
    with torch.no_grad():
        xx = t2c(t1c(up, lv, out="planes", splitk=False), lv, out="planes", splitk=False)
        cls = [c_(xx, lv, out="f32", splitk=False, kxr=True) for c_ in cls_l]
        lst_s, ctl_s = ops.head_candidates(cls, head.num_classes, thr, segn, [h * w for h, w, _, _ in W1], [h * w for h, w, _, _ in W2], B, sizes, split=True, shapes=True)
        lst_p, ctl_p = ops.head_candidates(cls, head.num_classes, thr, capn, 49, 25, B, sizes, split=True)
    cs, cp = ctl_s.tolist(), ctl_p.tolist()
    n_k = [cs[SEG * (k + 1) + ops.HEAD_CTL_RAW] for k in range(K)]
    o_k = [cs[SEG * (k + 1) + ops.HEAD_CTL_OWN + ops.HEAD_CTL_RAW] for k in range(K)]
    from collections import Counter
    seen = Counter(m_ for k in range(K) for m_ in lst_s[k * segn:k * segn + cs[SEG * (k + 1) + ops.HEAD_CTL_N]].tolist())
    print("shape mix: positions", cp[ops.HEAD_CTL_RAW], "(own", cp[ops.HEAD_CTL_OWN + ops.HEAD_CTL_RAW], ") entries", sum(n_k), "(own", sum(o_k), ") segment capacity", segn)
    for k in range(K):
        print("  shape %dx%d: entries %d = own %d + partner-only %d" % (SHP[k][0], SHP[k][1], n_k[k], o_k[k], n_k[k] - o_k[k]))
    print("  positions with more than one shape:", sum(1 for v in seen.values() if v > 1), "of", len(seen))
    # tower pixel-layers per step: whole maps (49 + 25 per position; mask + track towers at the own ones) against the windows of each entry's shape
    whole = (49 + 25) * (cp[ops.HEAD_CTL_RAW] + 2 * cp[ops.HEAD_CTL_OWN + ops.HEAD_CTL_RAW])
    wins = sum((W1[k][0] * W1[k][1] + W2[k][0] * W2[k][1]) * (n_k[k] + 2 * o_k[k]) for k in range(K))
    print("  tower pixel-layers x 256-channel branches: whole maps %d, windows %d (%.3f)" % (whole, wins, wins / whole))
for j, (name, _) in enumerate(stages[0]):
    print("%-28s %8.3f ms" % (name, min(s[j][1] for s in stages)))
print("sum", sum(min(s[j][1] for s in stages) for j in range(len(stages[0]))))
# dense head stages
dstages = []
def dense_once(record):
    marks = [("start", ev())]
    def m(name):
        marks.append((name, ev()))
    t1 = pg.tower1(up, lv, out="planes"); m("tower1")
    t2 = pg.tower2(t1, lv, out="planes"); m("tower2")
    outs = [(f.small(t2, lv, out="f32"), f.trk(t2, lv, out="f32", x_ch_off=3 * cw)) for f in pg.finals]; m("outputs")
    ops.head_assemble([o[0] for o in outs], [o[1] for o in outs], B, sizes, head.num_classes, head.mask_dim, head.embed_dim, P); m("assemble")
    torch.cuda.synchronize()
    if record:
        dstages.append([(marks[i][0], marks[i - 1][1].elapsed_time(marks[i][1])) for i in range(1, len(marks))])
with torch.no_grad():
    for i in range(6):
        dense_once(i >= 2)
for j, (name, _) in enumerate(dstages[0]):
    print("dense %-22s %8.3f ms" % (name, min(s[j][1] for s in dstages)))
print("dense sum", sum(min(s[j][1] for s in dstages) for j in range(len(dstages[0]))))
