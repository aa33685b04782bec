"""The training target assignment of the reference's loss (layers/box_utils.py match, :119-197, and encode, :200-235) restated in torch ops
in this project's words: any floating dtype, any device, and the FIRST index wins every maximum tie (what the reference's CPU `max` does; a
device `max` promises no such thing, so the first maximum is taken explicitly).  Checked against the reference itself by
tests/golden/gen_match_golden.py; the CPU tests hold it to the goldens, and scripts/bench_match.py times it on the card as the baseline of
the kernels in csrc/match.hip.

Constants follow the reference's mixed Python-float / tensor arithmetic: pos, pos - 0.1 and (pos + neg) / 2 are formed in double and rounded
to the tensors' dtype once; pos' = pos + mean(cla) is an addition in the tensors' dtype.
"""
import torch


def point_form(priors):
    return torch.cat((priors[:, :2] - priors[:, 2:] / 2, priors[:, :2] + priors[:, 2:] / 2), 1)


def overlaps(boxes, pf):
    """IoU [G, P] in the operand order of stm_iou (csrc/stm_common.h), which is the reference's jaccard."""
    a, b = boxes[:, None, :], pf[None, :, :]
    mx = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp(min=0)
    my = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp(min=0)
    inter = mx * my
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (area_a + area_b - inter)


def first_max(x, dim):
    """(max, index of its first occurrence) along dim."""
    m = x.max(dim, keepdim=True).values
    n = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = n
    ar = torch.arange(n, device=x.device).view(shape)
    idx = torch.where(x == m, ar, n).min(dim).values
    return m.squeeze(dim), idx


def encode(matched, priors):
    g_cxcy = ((matched[:, :2] + matched[:, 2:]) / 2 - priors[:, :2]) / (0.1 * priors[:, 2:])
    g_wh = torch.log((matched[:, 2:] - matched[:, :2]) / priors[:, 2:]) / 0.2
    return torch.cat([g_cxcy, g_wh], 1)


def match(pos, neg, bbox, labels, ids, priors, conf):
    """One image.  bbox [G,4] point form, labels / ids [G] int64, priors [P,4] centre-size, conf [P,C] raw scores.  Returns a dict: loc_t [P,4],
    conf_t, idx_t, ids_t [P] int64, gt_boxes_t [P,4], and for reading a case's margins best_overlap [P] (final), pos2 / neg2 (the thresholds
    applied at the end, 0-dim tensors), multi [P] (where the multi-instance rule fired), n_keep."""
    dt, dev = bbox.dtype, bbox.device
    G, P = bbox.shape[0], priors.shape[0]

    def const(v):
        return torch.tensor(v, dtype=dt, device=dev)

    ov = overlaps(bbox, point_form(priors))
    best, bidx = first_max(ov, 0)
    multi = (ov > const(pos - 0.1)).sum(0) > 1
    best = torch.where(multi, const((pos + neg) / 2), best)
    pos2, neg2 = const(pos), const(neg)
    keep = best > pos2
    n_keep = int(keep.sum())
    if n_keep > 0:
        rows = conf.detach()[keep].to(dt)
        ce = torch.logsumexp(rows, 1) - rows.gather(1, labels[bidx[keep]][:, None])[:, 0]
        cla = 2 / (1 + ce.exp())
        best = best.clone()
        best[keep] = best[keep] + cla
        mean = cla.mean()
        pos2, neg2 = pos2 + mean, neg2 + mean

    # every box is used at least once: G picks on a working copy, the largest remaining overlap first
    work = ov.clone()
    for _ in range(G):
        row_max, row_arg = first_max(work, 1)
        _, j = first_max(row_max, 0)
        i = row_arg[j]
        work.index_fill_(1, i.view(1), -1)
        work.index_fill_(0, j.view(1), -1)
        best.index_fill_(0, i.view(1), 2)
        bidx.index_copy_(0, i.view(1), j.view(1))

    conf_t = labels[bidx].clone()
    conf_t[best < pos2] = -1
    conf_t[best < neg2] = 0
    ids_t = ids[bidx].clone()
    ids_t[best < pos2] = 0
    gt = bbox[bidx]
    return dict(loc_t=encode(gt, priors), conf_t=conf_t, idx_t=bidx, ids_t=ids_t, gt_boxes_t=gt, best_overlap=best, pos2=pos2, neg2=neg2,
                multi=multi, n_keep=n_keep)


def margin(r):
    """min over the priors of |best_overlap - pos'| and |best_overlap - neg'|: how far the case is from a threshold flip."""
    b = r["best_overlap"].double()
    return float(torch.minimum((b - r["pos2"].double()).abs(), (b - r["neg2"].double()).abs()).min())
