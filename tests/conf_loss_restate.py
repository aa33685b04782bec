"""fp64 restatement of the OHEM class-confidence loss conventions (include/stmask_hip.h) for the tests of
layers.select_neg_bboxes / layers.ohem_conf_loss, and the builders of the test cases.

With N = B * P, x = conf_data as [N, C], t = conf_t as [N]:
    lse_i   = m_i + log(sum_c exp(x_ic - m_i)),  m_i the row's own maximum                                (fp64)
    score_i = fp32(lse_i - x_i0) where t_i == 0, exactly 0 elsewhere                                      (an fp32 number: the ranking is on it)
    k       = min(ratio * #(t > 0), N - 1); selected negative iff t_i == 0 and among the k largest scores under (score descending, index ascending)
    weights: positive of image b 1 / max(npos_b, 1), w_neg = ratio * B / num_neg; "reference": by position over the kept rows in index order,
             "aligned": by class
    C       = alpha * sum_i w_i (lse_i - x_{i,t_i}) / (ratio + 1)
    grad    = g * alpha / (ratio + 1) * w_i * (exp(x_ic - lse_i) - [c == t_i])
A label >= C makes that row's term and gradient row NaN.
"""
import numpy as np
import torch

EPS = 2.0 ** -24


def restate(conf_data, conf_t, ratio=3, alpha=1.0, weights="reference", g=1.0):
    B = conf_data.shape[0] if conf_data.dim() == 3 else (conf_t.shape[0] if conf_t.dim() == 2 else 1)
    C = conf_data.shape[-1]
    x = conf_data.detach().double().reshape(-1, C).cpu()
    t = conf_t.reshape(-1).cpu()
    N = x.shape[0]
    P = N // B
    m = x.max(1).values
    lse = m + torch.log(torch.exp(x - m[:, None]).sum(1))
    score = torch.where(t == 0, (lse - x[:, 0]).float(), torch.zeros(N))              # fp32
    num_pos = int((t > 0).sum())
    k = min(ratio * num_pos, N - 1)
    order = np.lexsort((np.arange(N), -score.numpy().astype(np.float64)))             # score descending, index ascending
    topk = torch.zeros(N, dtype=torch.bool)
    topk[torch.from_numpy(order[:k].copy())] = True
    neg = topk & (t == 0)
    pos = t > 0
    keep = pos | neg
    num_neg = int(neg.sum())
    npos_img = pos.view(B, P).sum(1)
    w_pos_img = 1.0 / npos_img.clamp(min=1).double()
    w_neg = ratio * B / num_neg if num_neg else 0.0
    w = torch.zeros(N, dtype=torch.float64)
    img = torch.arange(N) // P
    if weights == "aligned":
        w[pos] = w_pos_img[img[pos]]
        w[neg] = w_neg
    else:
        assert weights == "reference"
        vec = torch.cat([w_pos_img[img[pos]], torch.full((num_neg,), w_neg, dtype=torch.float64)])
        w[keep] = vec
    bad = t >= C
    tc = t.clamp(0, C - 1)
    ce = lse - x.gather(1, tc[:, None])[:, 0]
    ce = torch.where(bad, torch.full_like(ce, float("nan")), ce)
    scale = alpha / (ratio + 1)
    kept = keep.nonzero()[:, 0]
    loss = scale * (w[kept] * ce[kept]).sum() if kept.numel() else torch.zeros((), dtype=torch.float64)
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p)
    onehot[torch.arange(N), tc] = 1.0
    grad = g * scale * w[:, None] * (p - onehot)
    grad[~keep] = 0.0
    grad[keep & bad] = float("nan")
    absmax = x.abs().max(1).values
    ce_fin = torch.where(bad, torch.zeros_like(ce), ce)
    loss_bound = 16 * EPS * scale * (w * (absmax + ce_fin.abs())).sum()
    grad_bound = abs(g) * scale * w * EPS * (8 + (x - lse[:, None]).abs().max(1).values)    # per row, for every element of it
    s_sorted = score.numpy()[order]
    return dict(B=B, P=P, C=C, N=N, lse=lse, score=score, k=k, num_pos=num_pos, num_neg=num_neg, neg=neg, pos=pos, keep=keep, w=w, ce=ce,
                loss=loss, grad=grad, loss_bound=loss_bound, grad_bound=grad_bound,
                margin=float(s_sorted[k - 1] - s_sorted[k]) if 0 < k < N else float("inf"))


def margin(conf_data, conf_t, ratio=3):
    """The gap between the k-th and the (k+1)-th score."""
    return restate(conf_data, conf_t, ratio)["margin"]


def draw_targets(B, P, C, npos, nneutral, gen):
    """conf_t int64 [B, P]: npos[b] positives (classes 1 .. C-1) and nneutral[b] neutrals (-1) at random priors of image b, background elsewhere."""
    t = torch.zeros(B, P, dtype=torch.int64)
    for b in range(B):
        perm = torch.randperm(P, generator=gen)
        t[b, perm[:npos[b]]] = torch.randint(1, C, (npos[b],), generator=gen)
        t[b, perm[npos[b]:npos[b] + nneutral[b]]] = -1
    return t


def draw_logits(B, P, C, seed, scale=2.0):
    return scale * torch.randn(B, P, C, generator=torch.Generator().manual_seed(int(seed)))


def scalar(a):
    """A stored scalar as a Python float, whatever shape the fixture gave it."""
    return float(np.asarray(a).reshape(-1)[0])


def golden_case(z, name):
    """(conf_data, conf_t) of a case of tests/golden/conf_loss_cases.npz: the logits come from the stored seed."""
    B, P, C = (int(v) for v in z[f"{name}__shape"])
    conf_t = torch.from_numpy(z[f"{name}__conf_t"].astype(np.int64)).view(B, P)
    return draw_logits(B, P, C, int(scalar(z[f"{name}__seed"])), scalar(z[f"{name}__scale"])), conf_t


def _score_row(target, C):
    """A logit row (x_0 = -a, the others 0) whose fp64 score log(C - 1 + exp(-a)) + a is `target` (> log(C)); bisection on a."""
    lo, hi = 0.0, 200.0
    for _ in range(200):
        mid = (lo + hi) / 2
        if np.log(C - 1 + np.exp(-mid)) + mid < target:
            lo = mid
        else:
            hi = mid
    row = torch.zeros(C)
    row[0] = -lo
    return row


def constructed_cases():
    """name -> (conf_data [B,P,C] fp32, conf_t [B,P] int64): the cases no generator of the reference can pin (ties, cuts among the zeros)."""
    cases = {}
    gen = torch.Generator().manual_seed(4100)
    # 20 positives of 37 priors: k = 36 exceeds the 17 negatives, the cut falls among the zero scores and num_neg < k
    cases["k_exceeds"] = (draw_logits(1, 37, 5, 4101), draw_targets(1, 37, 5, [20], [0], gen))
    # no positive at all: k = 0, loss exactly 0
    cases["no_pos"] = (draw_logits(2, 37, 41, 4102), draw_targets(2, 37, 41, [0, 0], [3, 1], gen))
    # positives and neutrals only: num_neg = 0 with positives present
    cases["num_neg0"] = (draw_logits(1, 37, 41, 4103), draw_targets(1, 37, 41, [30], [7], gen))
    # logits 30 * randn and one row alternating +80 / -80: the row maximum is needed
    x = draw_logits(2, 300, 41, 4104, 30.0)
    t = draw_targets(2, 300, 41, [6, 5], [4, 4], gen)
    x[0, 17] = 80.0 * (1 - 2 * (torch.arange(41) % 2)).float()
    t[0, 17] = 0
    cases["wide"] = (x, t)
    # four identical negative rows at 255, 256 (a tile border) and 299, 300 (the image border) with the cut between them: 10 scores above, k = 12
    x = draw_logits(2, 300, 41, 4105)
    t = draw_targets(2, 300, 41, [2, 2], [3, 3], gen)
    tied = [255, 256, 299, 300]
    t.view(-1)[tied] = 0
    r = restate(x, t)
    s = r["score"].double().clone()
    s[tied] = -1.0
    top = torch.sort(s, descending=True).values
    x.view(-1, 41)[tied] = _score_row(float(top[9] + top[10]) / 2, 41)
    cases["ties"] = (x, t)
    # true negatives whose fp32 score is exactly 0 (x_0 = 200, the others 0), one at a low and one at a high index, with the cut among the zeros
    x = draw_logits(2, 300, 41, 4106)
    t = draw_targets(2, 300, 41, [80, 80], [0, 0], gen)
    zrow = torch.zeros(41)
    zrow[0] = 200.0
    for i in (3, 590):
        x.view(-1, 41)[i] = zrow
        t.view(-1)[i] = 0
    cases["zero_score"] = (x, t)
    return cases
