#!/usr/bin/env python3
"""Golden values of the positive-prior loss terms, from the REFERENCE's own code (layers/modules/multibox_loss.py) run unchanged in fp32 on the
CPU under STMask_plus_resnet50_config (build container only; the reference is imported the way gen_golden.py imports it):

    python tests/golden/gen_pos_loss_golden.py            # writes tests/golden/pos_loss_cases.npz

  losses['BIoU']    decode, MultiBoxLoss.get_DIoU and the three lines :170-172
  losses['center']  MultiBoxLoss.ohem_conf_loss (:450-455; with the get_device patch of gen_conf_loss_golden.py)
  losses['T']       MultiBoxLoss.track_loss (:328-351)
each called unbound on a namespace, with autograd gradients taken (g_b * BIoU + g_c * center in one backward, so that the gradient which
`center` sends to loc_data through its undetached target is part of what is stored).

The generator asserts that the restatements (tests/pos_loss_restate.py) hold the reference's fp32 losses and gradients within their bounds and
stores the reference's deviation as a fraction of the bound per case (dev_*).  For the track cases seeds are tried in order until no pair lies
within 2e-3 of a clamp.

The fixture holds data only: shapes, seeds, targets, the reference's outputs.  The inputs come from the seeded draws of pos_loss_restate.py.
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
import pos_loss_restate as R  # noqa: E402

G_B, G_C, G_T = 0.75, 1.25, 0.75         # the incoming gradients (exact in fp32)
MIN_V = 2e-3


def pos_weights_of(conf_t):
    pos = conf_t > 0
    num_pos_per_img = [pos[i].sum().long() for i in range(conf_t.shape[0])]
    split = torch.ones(int(pos.sum())).split(num_pos_per_img)                              # :159-161
    return [cur / torch.clamp(cur.sum(), min=1) for cur in split]


def reference_box(MBL, decode, cfg, loc, pri, gt, conf_t, cent):
    B, P = conf_t.shape
    ns = types.SimpleNamespace(num_classes=41, negpos_ratio=3)
    ns.select_neg_bboxes = lambda cd, ct: MBL.select_neg_bboxes(ns, cd, ct)
    ns.get_DIoU = lambda a, b: MBL.get_DIoU(ns, a, b)
    priors = (pri if pri.dim() == 3 else pri[None].repeat(B, 1, 1)).contiguous()
    pos = conf_t > 0
    pos_weights = torch.cat(pos_weights_of(conf_t), dim=0)
    x = loc.clone().requires_grad_(True)
    c = cent.clone().requires_grad_(True)
    decoded_loc_p = decode(x[pos].view(-1, 4), priors[pos].view(-1, 4), cfg.use_yolo_regressors)      # :170
    DIoU = ns.get_DIoU(decoded_loc_p, gt[pos])                                                         # :171
    biou = (pos_weights * (1 - DIoU)).sum() * cfg.bboxiou_alpha                                        # :172
    conf = torch.randn(B, P, 41, generator=torch.Generator().manual_seed(1))
    with mock.patch.object(torch.Tensor, "get_device", lambda self: "cpu"):
        center = MBL.ohem_conf_loss(ns, pos_weights, conf, conf_t, c, x, priors, gt)["center"]
    (G_B * biou + G_C * center).backward()
    return biou.detach(), center.detach(), x.grad.view(-1, 4), c.grad.view(-1), DIoU.detach()


def reference_track(MBL, track, conf_t, ids):
    x = track.clone().requires_grad_(True)
    loss = MBL.track_loss(types.SimpleNamespace(), pos_weights_of(conf_t), x, conf_t, ids)
    (G_T * loss).backward()
    return loss.detach(), x.grad.view(-1, track.shape[-1])


def frac(err, bound):
    live = bound > 0
    assert bool((err[~live] == 0).all())
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def main():
    gen_golden.install_stubs()
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.box_utils import decode
    from layers.modules.multibox_loss import MultiBoxLoss as MBL
    assert cfg.use_boxiou_loss and cfg.train_boxes and cfg.train_track and not cfg.use_yolo_regressors and not cfg.ohem_use_most_confident
    ab, ac, at = float(cfg.bboxiou_alpha), float(cfg.center_alpha), float(cfg.track_alpha)
    out = dict(box_names=np.array([c[0] for c in R.BOX_GOLDEN]), track_names=np.array([c[0] for c in R.TRACK_GOLDEN]),
               bboxiou_alpha=np.float64(ab), center_alpha=np.float64(ac), track_alpha=np.float64(at), g_b=np.float64(G_B), g_c=np.float64(G_C),
               g_t=np.float64(G_T))

    for ci, (name, B, P, npos, nneu, per) in enumerate(R.BOX_GOLDEN):
        seed = 21000 + 100 * ci
        conf_t = R.draw_conf_t(B, P, npos, torch.Generator().manual_seed(seed + 50), nneu)
        loc, pri, gt, cent = R.draw_boxes(B, P, seed, per)
        biou, center, gl, gc, diou = reference_box(MBL, decode, cfg, loc, pri, gt, conf_t, cent)
        r = R.restate_box(loc, pri, gt, conf_t, cent, ab, ac, G_B, G_C)
        pos = r["pos"]
        dev = dict(dev_biou=float((biou.double() - r["biou"]).abs() / r["biou_bound"]),
                   dev_center=float((center.double() - r["center"]).abs() / r["center_bound"]),
                   dev_grad_loc=frac((gl.double() - r["grad_loc"]).abs()[pos], r["grad_loc_bound"][pos]),
                   dev_grad_cent=frac((gc.double() - r["grad_cent"]).abs()[pos], r["grad_cent_bound"][pos]))
        assert all(v <= 1.0 for v in dev.values()), (name, dev)
        assert float(gl[~pos].abs().max()) == 0.0 and float(gc[~pos].abs().max()) == 0.0, name
        # the other reading (a detached target) is NOT what the reference computes
        rd = R.restate_box(loc, pri, gt, conf_t, cent, ab, ac, G_B, G_C, detach_target=True)
        assert frac((gl.double() - rd["grad_loc"]).abs()[pos], rd["grad_loc_bound"][pos]) > 100.0, name
        out.update({f"box_{name}__{k}": v for k, v in dict(
            shape=np.array([B, P], dtype=np.int64), seed=np.int64(seed), per_image=np.int64(per), conf_t=conf_t.view(-1).to(torch.int16),
            biou=biou, center=center, grad_loc_pos=gl[pos], grad_cent_pos=gc[pos], diou_min=diou.min(), diou_max=diou.max(),
            **{k: np.float64(v) for k, v in dev.items()}).items()})
        print(f"box {name}: B={B} P={P} n={r['n']} BIoU={float(biou):.6f} (restated {float(r['biou']):.6f}) center={float(center):.6f} "
              f"(restated {float(r['center']):.6f}) DIoU in [{float(diou.min()):.3f}, {float(diou.max()):.3f}] " +
              " ".join(f"{k}={v:.3f}" for k, v in dev.items()))

    for ci, (name, B, P, D, npos, n_ids) in enumerate(R.TRACK_GOLDEN):
        for trial in range(200):
            seed = 23000 + 1000 * ci + trial
            conf_t = R.draw_conf_t(B, P, npos, torch.Generator().manual_seed(seed + 500), 2)
            x, ids = R.draw_track(B, P, D, seed, n_ids)
            r = R.restate_track(x, conf_t, ids, at, G_T)
            if r["min_v"] > MIN_V:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps the pairs off the clamp")
        loss, grad = reference_track(MBL, x, conf_t, ids)
        pos = r["pos"]
        dev_loss = float((loss.double() - r["loss"]).abs() / r["loss_bound"])
        dev_grad = frac((grad.double() - r["grad"]).abs()[pos], r["grad_bound"][pos])
        assert dev_loss <= 1.0 and dev_grad <= 1.0, (name, dev_loss, dev_grad)
        assert float(grad[~pos].abs().max()) == 0.0, name
        out.update({f"track_{name}__{k}": v for k, v in dict(
            shape=np.array([B, P, D], dtype=np.int64), seed=np.int64(seed), n_ids=np.int64(n_ids), conf_t=conf_t.view(-1).to(torch.int16),
            loss=loss, grad_pos=grad[pos], min_v=np.float64(r["min_v"]), dev_loss=np.float64(dev_loss), dev_grad=np.float64(dev_grad)).items()})
        print(f"track {name}: B={B} P={P} D={D} seed={seed} n={r['n']} T={float(loss):.6f} (restated {float(r['loss']):.6f}) "
              f"min_v={r['min_v']:.2e} dev_loss={dev_loss:.3f} dev_grad={dev_grad:.3f}")

    # the clamp case through the reference's fp32 chain: equal weights, track_alpha = 5
    x, conf_t, ids = R.clamp_case()
    with mock.patch.object(cfg, "track_alpha", 5.0):
        loss, grad = reference_track(MBL, x, conf_t, ids)
    out["clamp_loss_alpha5"] = loss
    out["clamp_grad"] = grad
    print(f"clamp case: T={float(loss):.5f}")
    gen_golden.save("pos_loss_cases.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "pos_loss_cases.npz"))
    assert size < 1024 * 1024, size


if __name__ == "__main__":
    main()
