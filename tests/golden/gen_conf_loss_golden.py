#!/usr/bin/env python3
"""Golden values of the OHEM class-confidence loss, from the REFERENCE's own select_neg_bboxes and ohem_conf_loss
(layers/modules/multibox_loss.py:402-448) run unchanged in fp32 on the CPU under STMask_plus_resnet50_config (build container only; the
reference is imported the way gen_golden.py imports it):

    python tests/golden/gen_conf_loss_golden.py            # writes tests/golden/conf_loss_cases.npz

select_neg_bboxes asks conf_t.get_device() for a device index, which is -1 on the CPU and makes torch.zeros raise; the generator (and only the
generator) patches Tensor.get_device to return "cpu" while the two methods run.  They are called unbound on a namespace that carries
num_classes and negpos_ratio, so no network and no dataset is built.

The reference's tie order at the cut is an accident of an unstable sort, so per case seeds are tried in order until the gap between the k-th
and the (k+1)-th score exceeds 1e-4.  The generator then asserts that the restatement (tests/conf_loss_restate.py) selects exactly the
reference's set, and that the reference's fp32 losses['C'] and its autograd gradient on the kept rows lie within the restatement's bounds; the
reference's deviation, as a fraction of the bound, is stored per case (dev_loss, dev_grad).

The fixture holds data only: shapes, seeds, targets, the reference's outputs.  The logits are scale * randn(B, P, C) from
torch.Generator().manual_seed(seed) and are not stored.
"""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import gen_golden  # noqa: E402
import conf_loss_restate as R  # noqa: E402

MARGIN = 1e-4
RATIO = 3

# name -> (B, P, C, positives per image, neutrals per image, logit scale)
CASES = [
    ("p37", 1, 37, 41, [4], [2], 2.0),
    ("ragged", 3, 300, 26, [7, 0, 3], [4, 2, 0], 2.0),
    ("c2", 2, 300, 2, [5, 6], [3, 3], 2.0),
    ("c128", 2, 300, 128, [6, 4], [3, 2], 2.0),
    ("full_b2", 2, 15345, 41, [80, 70], [12, 13], 2.0),
]


def reference_run(MBL, alpha, conf, conf_t, C):
    B = conf_t.shape[0]
    ns = types.SimpleNamespace(num_classes=C, negpos_ratio=RATIO)
    ns.select_neg_bboxes = lambda cd, ct: MBL.select_neg_bboxes(ns, cd, ct)
    pos = conf_t > 0
    num_pos_per_img = [pos[i].sum().long() for i in range(B)]
    split = torch.ones(int(pos.sum()), device=conf.device).split(num_pos_per_img)          # :159-161
    pos_weights = torch.cat([cur / torch.clamp(cur.sum(), min=1) for cur in split], dim=0)
    x = conf.clone().requires_grad_(True)
    with mock.patch.object(torch.Tensor, "get_device", lambda self: "cpu"):
        neg = MBL.select_neg_bboxes(ns, x.detach(), conf_t)
        losses = MBL.ohem_conf_loss(ns, pos_weights, x, conf_t, None, None, None, None)
    losses["C"].backward()
    return neg, losses["C"].detach(), x.grad.view(-1, C)


def main():
    gen_golden.install_stubs()
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.modules.multibox_loss import MultiBoxLoss as MBL
    assert not cfg.ohem_use_most_confident and not cfg.use_sigmoid_focal_loss
    alpha = float(cfg.conf_alpha)
    out = dict(case_names=np.array([c[0] for c in CASES]), ratio=np.int64(RATIO), conf_alpha=np.float64(alpha))
    for ci, (name, B, P, C, npos, nneu, scale) in enumerate(CASES):
        for trial in range(200):
            seed = 11000 + 1000 * ci + trial
            conf_t = R.draw_targets(B, P, C, npos, nneu, torch.Generator().manual_seed(seed + 500))
            conf = R.draw_logits(B, P, C, seed, scale)
            r = R.restate(conf, conf_t, RATIO, alpha, "reference")
            if r["margin"] > MARGIN:
                break
        else:
            raise SystemExit(f"{name}: no seed clears the margin")
        neg, loss, grad = reference_run(MBL, alpha, conf, conf_t, C)
        assert torch.equal(neg > 0, r["neg"]), name
        kept = r["keep"].nonzero()[:, 0]
        dev_loss = float((loss.double() - r["loss"]).abs() / r["loss_bound"])
        dev_grad = float(((grad[kept].double() - r["grad"][kept]).abs() / r["grad_bound"][kept, None]).max())
        assert dev_loss <= 1.0 and dev_grad <= 1.0, (name, dev_loss, dev_grad)
        assert float(grad[~r["keep"]].abs().max()) == 0.0, name
        ra = R.restate(conf, conf_t, RATIO, alpha, "aligned")
        out.update({f"{name}__{k}": v for k, v in dict(
            shape=np.array([B, P, C], dtype=np.int64), seed=np.int64(seed), scale=np.float64(scale), conf_t=conf_t.view(-1).to(torch.int16),
            neg=np.packbits(r["neg"].numpy()), loss=loss, kept=kept.to(torch.int32), grad_kept=grad[kept], margin=np.float64(r["margin"]),
            dev_loss=np.float64(dev_loss), dev_grad=np.float64(dev_grad), aligned_over_reference=np.float64(float(ra["loss"] / r["loss"]))).items()})
        print(f"{name}: B={B} P={P} C={C} seed={seed} num_pos={r['num_pos']} k={r['k']} num_neg={r['num_neg']} margin={r['margin']:.2e} "
              f"C={float(loss):.6f} restated={float(r['loss']):.6f} aligned={float(ra['loss']):.6f} dev_loss={dev_loss:.3f} dev_grad={dev_grad:.3f}")
    gen_golden.save("conf_loss_cases.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "conf_loss_cases.npz"))
    assert size < 1024 * 1024, size


if __name__ == "__main__":
    main()
