#!/usr/bin/env python3
"""Golden values of the training target assignment, from the REFERENCE's own match and encode (layers/box_utils.py:119-235) run in fp32 on the
CPU under STMask_plus_resnet50_config (build container only; the reference is imported the way gen_golden.py imports it):

    python tests/golden/gen_match_golden.py            # writes tests/golden/match_cases.npz

The reference's fp32 and fp64 runs disagree on idx_t (near-equal IoUs on the symmetric prior grid), so the goldens are its fp32 outputs and
idx_t is an exact contract.  Per case the generator asserts that the fp32 restatement (tests/match_restate.py) equals the reference exactly
on conf_t, idx_t and ids_t, and that no prior's best overlap lies within 1e-4 of a final threshold (the cross-entropy path can move a value
by a few fp32 ulp, about 1e-6); seeds are tried in order until one clears that margin, and no prior is excluded from any comparison.

The fixture holds data only.  Priors are prefixes, one level or all of priors.npz and are not stored again.  conf = 2 * randn(P, C) from
torch.Generator().manual_seed(conf_seed); it is stored in full for P <= 300 and otherwise as the seed plus the rows the reference read (the
priors that passed `best > pos`), which the tests compare exactly against what the seed gives them.  loc_t is stored transposed ([4, P]): the
columns repeat along the prior grid and compress.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import gen_golden  # noqa: E402
import match_restate as R  # noqa: E402

C = 41
MARGIN = 1e-4

# name -> (prior set, G, kind)
CASES = [
    ("p37_g1", "prefix37", 1, "near"), ("p37_g5", "prefix37", 5, "near"), ("p300_g1", "prefix300", 1, "near"), ("p300_g5", "prefix300", 5, "near"),
    ("lvl24x40_twin", "p_24x40", 2, "twin"),
    ("full_g1", "all", 1, "free"), ("full_g7", "all", 7, "free"), ("full_g20", "all", 20, "free"), ("full_g40", "all", 40, "free"),
    ("p300_g65", "prefix300", 65, "near"), ("p300_g128", "prefix300", 128, "near"),
    ("p300_tiny", "prefix300", 1, "tiny"), ("p300_multi", "prefix300", 2, "multi"),
]
RAGGED = ("full_g1", "full_g7", "full_g20")      # the B = 3 batch of match_batch is made of these three cases


def prior_set(z, which):
    allp = torch.cat([torch.from_numpy(z[k]) for k in ("p_48x80", "p_24x40", "p_12x20", "p_6x10", "p_3x5")])
    if which == "all":
        return allp
    if which.startswith("prefix"):
        return allp[:int(which[6:])].clone()
    return torch.from_numpy(z[which]).clone()


def draw_boxes(priors, G, kind, g):
    pf = R.point_form(priors)
    if kind == "free":
        c = torch.rand(G, 2, generator=g) * 0.8 + 0.1
        wh = torch.rand(G, 2, generator=g) * 0.45 + 0.04
        return torch.cat((c - wh / 2, c + wh / 2), 1).float()
    k = torch.randint(0, priors.shape[0], (G,), generator=g)
    if kind == "tiny":        # smaller than every prior: no overlap above pos, only the forced match is positive
        c = priors[k, :2] + 0.001
        wh = priors[:, 2:].min() * 0.2
        return torch.cat((c - wh / 2, c + wh / 2), 1).float()
    if kind == "multi":       # two boxes well above pos - 0.1 on the same priors
        b0 = pf[k[:1]] + torch.tensor([[0.001, -0.0007, 0.0013, 0.0004]])
        s = (b0[:, 2:] - b0[:, :2]) * 0.06
        return torch.cat((b0, torch.cat((b0[:, :2] - s, b0[:, 2:] + s), 1))).float()
    if kind == "twin":        # box 1 = box 0 + 0.004: both have the same best prior, the second pick must re-scan its row
        b0 = pf[k[:1]] * 1.0 + torch.tensor([[0.0021, 0.0013, 0.0042, 0.0037]])
        return torch.cat((b0, b0 + 0.004)).float()
    scale = torch.rand(G, 1, generator=g) * 0.7 + 0.7
    c = priors[k, :2] + (torch.rand(G, 2, generator=g) - 0.5) * 0.02
    wh = priors[k, 2:] * scale * (torch.rand(G, 2, generator=g) * 0.3 + 0.85)
    return torch.cat((c - wh / 2, c + wh / 2), 1).float()


def reference_match(ref_match, pos, neg, bbox, labels, ids, priors, conf):
    P = priors.shape[0]
    loc_t, conf_t = torch.zeros(1, P, 4), torch.zeros(1, P, dtype=torch.int64)
    idx_t, ids_t = torch.zeros(1, P, dtype=torch.int64), torch.zeros(1, P, dtype=torch.int64)
    ref_match(pos, neg, bbox.clone(), labels.clone(), ids.clone(), priors.clone(), None, conf.clone(), loc_t, conf_t, idx_t, ids_t, 0)
    return loc_t[0], conf_t[0], idx_t[0], ids_t[0]


def main():
    gen_golden.install_stubs()
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.box_utils import encode as ref_encode, match as ref_match
    assert not (cfg.use_prediction_matching or cfg.use_change_matching or cfg.use_yolo_regressors)
    pos, neg = float(cfg.positive_iou_threshold), float(cfg.negative_iou_threshold)

    z = np.load(os.path.join(HERE, "priors.npz"))
    out = dict(pos=np.float64(pos), neg=np.float64(neg), n_classes=np.int64(C), case_names=np.array([c[0] for c in CASES]),
               case_priors=np.array([c[1] for c in CASES]), ragged=np.array(RAGGED))
    for ci, (name, which, G, kind) in enumerate(CASES):
        priors = prior_set(z, which)
        P = priors.shape[0]
        for trial in range(200):
            seed = 9000 + 1000 * ci + trial
            g = torch.Generator().manual_seed(seed)
            bbox = draw_boxes(priors, G, kind, g)
            labels = torch.randint(1, C, (G,), generator=g)
            ids = torch.randperm(500, generator=g)[:G] + 1
            conf = 2 * torch.randn(P, C, generator=torch.Generator().manual_seed(seed))
            r = R.match(pos, neg, bbox, labels, ids, priors, conf)
            if R.margin(r) <= MARGIN:
                continue
            if kind in ("near", "free") and r["n_keep"] == 0:
                continue
            break
        else:
            raise SystemExit(f"{name}: no seed clears the margin")
        assert bool(((bbox[:, 2] > bbox[:, 0]) & (bbox[:, 3] > bbox[:, 1])).all())
        loc, conf_t, idx_t, ids_t = reference_match(ref_match, pos, neg, bbox, labels, ids, priors, conf)
        assert torch.equal(conf_t, r["conf_t"]) and torch.equal(idx_t, r["idx_t"]) and torch.equal(ids_t, r["ids_t"]), name
        assert torch.equal(loc[:, :2], r["loc_t"][:, :2]), name
        if kind == "tiny":
            assert r["n_keep"] == 0 and int((conf_t > 0).sum()) == 1, name
        if kind == "multi":
            assert bool(r["multi"].any()), name
        if kind == "twin":
            forced = (r["best_overlap"] == 2).nonzero()[:, 0]
            ov = R.overlaps(bbox, R.point_form(priors))
            assert int(ov[0].argmax()) == int(ov[1].argmax()) and forced.numel() == 2, name
        # the conf rows the reference read: the priors whose best overlap passed pos before cla was added
        pre = R.first_max(R.overlaps(bbox, R.point_form(priors)), 0)[0]
        pre = torch.where(r["multi"], torch.tensor((pos + neg) / 2, dtype=torch.float32), pre)
        keep_rows = (pre > torch.tensor(pos, dtype=torch.float32)).nonzero()[:, 0]
        assert keep_rows.numel() == r["n_keep"]
        e = dict(bbox=bbox, labels=labels, ids=ids, conf_seed=np.int64(seed), loc_t_T=loc.t().contiguous(), conf_t=conf_t.to(torch.int16),
                 idx_t=idx_t.to(torch.int16), ids_t=ids_t.to(torch.int16), n_keep=np.int64(r["n_keep"]), n_multi=np.int64(int(r["multi"].sum())),
                 margin=np.float64(R.margin(r)))
        if P <= 300:
            e["conf"] = conf
        else:
            e["conf_rows_idx"] = keep_rows.to(torch.int32)
            e["conf_rows"] = conf[keep_rows]
        out.update({f"{name}__{k}": v for k, v in e.items()})
        print(f"{name}: P={P} G={G} seed={seed} keep={r['n_keep']} multi={int(r['multi'].sum())} positives={int((conf_t > 0).sum())} "
              f"neutral={int((conf_t < 0).sum())} margin={R.margin(r):.2e}")

    g = torch.Generator().manual_seed(801)
    n = 33
    pri = torch.cat((torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g) * 0.5 + 0.02), 1)
    c = torch.rand(n, 2, generator=g)
    wh = torch.rand(n, 2, generator=g) * 0.5 + 0.01
    matched = torch.cat((c - wh / 2, c + wh / 2), 1).float()
    out.update(enc_matched=matched, enc_priors=pri, enc_out=ref_encode(matched.clone(), pri.clone()))
    gen_golden.save("match_cases.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "match_cases.npz"))
    assert size < 1024 * 1024, size


if __name__ == "__main__":
    main()
