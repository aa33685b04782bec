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

The kernels work on tiles of TILE = 256 flattened rows and end in one workgroup of 256 threads that scans the tiles: thread t owns the tiles
[t * chunk, (t + 1) * chunk) with chunk = ceil(tiles / 256) and, likewise, ceil(B / 256) images.  The reference's generators stay below 256 tiles
and 4 images, where every thread owns one tile and the carry from tile to tile inside a thread never runs.  The scan cases of
constructed_cases() exist for that carry (chunk > 1: the tie ranks at the cut, the rank of a kept row behind the positional weights, the search
for the cut tile), for the second trip of the per-image loop (B > 256) and for the score kernel's staging counts that the model's class counts
do not reach (stage_rows(C) in {128, 192}); tests/test_conf_loss_cpu.py pins what each of them reaches.
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24
TILE = 256                              # rows per tile of the kernels, threads of the scanning workgroup
MARGIN = 1e-4                           # the gap the goldens keep at the cut: fp32 rounding of a score cannot move a row across it


def scan_chunk(count):
    """Tiles (or images) that one thread of the scanning workgroup walks, for `count` of them."""
    return -(-count // TILE)


def stage_rows(C):
    """Rows the score kernel stages at a time: as many rows of C | 1 floats as 48 KiB hold, in whole runs of 64, at most a tile."""
    return min(TILE, (12288 // (C | 1)) & ~63)


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


def _late_positives(t, C, rows):
    """Class labels at the flattened rows given (they join whatever draw_targets placed)."""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    t.view(-1)[rows] = 1 + rows % (C - 1)
    return t


# name -> (B, P, C, seed of the logits): arbitrary draws; the seed is the first from x100 on that keeps margin > MARGIN at the cut
SCAN_DRAWS = {
    "rows_chunk2": (8, 15345, 41, 4200),          # the reference's batch of 4 clips: 480 tiles
    "rows_chunk4": (16, 15345, 5, 4300),          # 960 tiles
    "images_300": (300, 37, 5, 4400),             # 44 tiles, 300 images: the per-image loop's second trip, 301 prefix entries to search
    "c81": (2, 300, 81, 4500),                    # stage_rows = 128
    "c60": (2, 300, 60, 4600),                    # stage_rows = 192: stages of 192 and 64 rows; the last tile has 88
}


def _scan_draw(name):
    B, P, C, seed = SCAN_DRAWS[name]
    gen = torch.Generator().manual_seed(seed + 50)
    N = B * P
    x = draw_logits(B, P, C, seed)
    if name == "images_300":                      # 3 images of every 7 without a positive, images past the 256th with some
        t = draw_targets(B, P, C, [(0, 2, 0, 5, 1, 0, 3)[b % 7] for b in range(B)], [b % 3 for b in range(B)], gen)
    elif name in ("c81", "c60"):
        t = draw_targets(B, P, C, [6, 5], [4, 4], gen)
    else:
        # The reference's positional weights give the r-th kept row the weight of the r-th positive's image as long as r < num_pos, so the
        # rank of a kept row matters up to the num_pos-th kept row only.  To carry that far into the scan, the last two images hold most of
        # the positives and, their logits being 8 times the others', all selected negatives; the images before hold a few positives each
        # (one none), among them the first and the last tile's and the last tile of a middle image.
        npos = [(3, 0, 2, 1, 5, 1)[b % 6] for b in range(B - 2)] + [90, 130]
        t = draw_targets(B, P, C, npos, [5] * B, gen)
        late = [0, 3, TILE - 1, TILE, N - 1, N - 2, N - TILE, N - TILE - 1]
        for b in (B // 2, B - 2, B - 1):
            late += [b * P, (b + 1) * P - 1, (b + 1) * P - 7, (b + 1) * P - TILE]
        _late_positives(t, C, late)
        x[:B - 2] *= 0.125
    return x, t


# The tie cases: B = 5, P = 15345, C = 2: 76 725 rows in 300 tiles, chunk = 2: scan thread j owns the tiles 2 j and 2 j + 1.
# tile -> number of identical true-negative rows in it; 37 and 100 lie before tile 101, 160 and 233 behind it, in other threads' chunks.
# The images 0 - 2 (tiles 0 - 179) have logits a hundredth of the others': besides the ties they hold no selected negative, and few positives
# (TIE_EARLY_POSITIVES, at offsets that no tie has), so that the kept rows of tile 161 still rank below num_pos -- where the rank decides the
# weight -- and would not if the ties of tile 160, of which none is taken, were counted as kept on the way from tile 160 to tile 161.
TIE_SHAPE = (5, 15345, 2)
TIE_TILES = {37: 100, 100: 150, 101: 200, 160: 220, 233: 100}
TIE_EARLY_POSITIVES = {0: [0], 37: [0], 100: [9], 101: [0, 252], 161: [0, 9, 18, 90, 252]}        # tile -> offsets, all multiples of 9
# ties taken (krem): 327 = 250 before tile 101 + 77 inside it, the second tile of thread 50's chunk;
# 250: the cut falls exactly behind tile 100 -- no tile is cut, and the first tile that takes nothing is the second of a chunk
TIE_TAKEN = {"ties_across_chunks": 327, "ties_cut_at_tile_end": 250}


def tie_rows():
    """The flattened rows of the tie cases' identical negatives: in each tile of TIE_TILES the first rows whose offset is no multiple of 9."""
    rows = []
    for tile, cnt in TIE_TILES.items():
        rows += [tile * TILE + p for p in range(TILE) if p % 9][:cnt]
    return rows


def _tie_case(name, seed):
    B, P, C = TIE_SHAPE
    x = draw_logits(B, P, C, seed)
    x[:3] *= 0.01
    t = draw_targets(B, P, C, [0, 0, 0, 170, 220], [6] * B, torch.Generator().manual_seed(seed + 50))
    _late_positives(t, C, [tile * TILE + p for tile, offs in TIE_EARLY_POSITIVES.items() for p in offs])
    tied = tie_rows()
    t.view(-1)[tied] = 0
    k = 3 * int((t > 0).sum())
    above = k - TIE_TAKEN[name]                   # scores above the ties' score, so that k cuts TIE_TAKEN[name] ties deep
    s = restate(x, t)["score"].double().clone()
    s[tied] = -1.0
    top = torch.sort(s, descending=True).values
    x.view(-1, C)[tied] = _score_row(float(top[above - 1] + top[above]) / 2, C)
    return x, t


@functools.lru_cache(maxsize=None)
def constructed_cases():
    """name -> (conf_data [B,P,C] fp32, conf_t [B,P] int64): the cases no generator of the reference can pin (ties, cuts among the zeros), and
    the scan cases (module docstring).  Built once and shared: nobody writes into them."""
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
    for name in SCAN_DRAWS:
        cases[name] = _scan_draw(name)
    for name in TIE_TAKEN:
        cases[name] = _tie_case(name, 4700)
    return cases
