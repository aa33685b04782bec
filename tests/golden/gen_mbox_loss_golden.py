#!/usr/bin/env python3
"""Golden values of the training criterion, from the REFERENCE's own code (layers/modules/multibox_loss.py) run unchanged in fp32 on the CPU
under STMask_plus_resnet50_config (build container only; the reference is imported the way gen_golden.py imports it, with the get_device
patch of gen_conf_loss_golden.py):

    python tests/golden/gen_mbox_loss_golden.py            # writes tests/golden/mbox_loss_cases.npz

Two runs per case of tests/mbox_loss_restate.py:
  1  MultiBoxLoss.lincomb_mask_loss called unbound on a namespace: losses['M'] before the division by the batch size, with the rows it formed
     on its way (recorded by wrapping the names it looks up in its module: generate_mask -- the crop boxes; F.binary_cross_entropy -- the
     per-instance sums; the wrappers pass everything through untouched);
  2  the whole MultiBoxLoss(41, 0.5, 0.4, 3).forward with the seeded stand-in TemporalNet of tests/t2s_loss_restate.py, every term as the
     reference returns it (BIoU, center, C and M after the division by the batch size of :213-214; T, B_shift, M_shift undivided), the
     targets its multibox_loss() assigned, and its autograd gradients of the SUM of all terms w.r.t. loc, conf, mask_coeff, proto, centerness,
     track and the stand-in's parameters (mmcv.ops.roi_align is the CPU oracle and carries no gradient: T2S_concat_feat gets none).

Seeds are tried in order until the case's input conditions hold: the target assignment and the OHEM cut keep a margin (no threshold flip between
two fp32 evaluations), every nonzero mask value lies in [0.05, 0.95], every crop edge stays mbox_loss_restate.EDGE prototype pixels away from an
integer of the crop rule, smooth-L1 of the shift loss stays off its kink and the track loss off its clamp.

Stored per case: the seed, the targets, every loss, the gradients (rows that can be nonzero only), and dev_*: the reference's fp32 deviation from
the restatements as a fraction of their bounds (asserted <= 1 here), e2e_* as the relative deviation of the shift losses and the stand-in's
parameter gradients from the fp64 composition (the yardstick of the end-to-end tolerance, as in t2s_loss_cases.npz).  Data only.
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
import conf_loss_restate as CR  # noqa: E402
import layer_grad_restate as LR  # noqa: E402
import mask_loss_restate as ML  # noqa: E402
import mbox_loss_restate as R  # noqa: E402
import oracle  # noqa: E402
import pos_loss_restate as PR  # noqa: E402
import t2s_loss_restate as T2S  # noqa: E402

MATCH_MARGIN, OHEM_MARGIN, TRACK_MIN_V = 1e-3, 1e-3, 2e-3


class _Proxy:
    def __init__(self, real, **over):
        self._real, self._over = real, over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(self._real, k)


def recording(mod, rec):
    real_gm, real_F = mod.generate_mask, mod.F

    def generate_mask(proto, coeff, bbox=None):
        rec["box"].append(bbox.detach().clone())
        return real_gm(proto, coeff, bbox)

    def binary_cross_entropy(inp, tgt, **k):
        out = real_F.binary_cross_entropy(inp, tgt, **k)
        rec["bce"].append(out.detach().sum(dim=(1, 2)))
        return out

    return mock.patch.object(mod, "generate_mask", generate_mask), mock.patch.object(mod, "F", _Proxy(real_F, binary_cross_entropy=binary_cross_entropy))


def reference_mask_term(mod, case):
    """The reference's lincomb_mask_loss unbound -> (M before / bs, boxes [n,4], bce [n])."""
    B, P = case["conf_t"].shape
    pos = case["conf_t"] > 0
    npi = [pos[i].sum().long() for i in range(B)]
    split = torch.ones(int(pos.sum())).split(npi)
    weights = [cur / torch.clamp(cur.sum(), min=1) for cur in split]                     # :159-161
    rec = dict(box=[], bce=[])
    p1, p2 = recording(mod, rec)
    priors = case["priors"][None].repeat(B, 1, 1)
    with p1, p2:
        out = mod.MultiBoxLoss.lincomb_mask_loss(types.SimpleNamespace(), weights, pos, case["idx_t"], case["ids_t"], case["loc"], case["mask_coeff"],
                                                 None, priors, case["proto"], sum(case["gt_masks"], []), case["gt_boxes_t"],
                                                 sum(case["gt_labels"], []))
    return out["M"].detach(), torch.cat(rec["box"]), torch.cat(rec["bce"])


def reference_forward(mod, case):
    """The whole forward -> (losses, targets the reference assigned, gradients of the sum of all terms)."""
    M = case["mask_coeff"].shape[2]
    B = case["loc"].shape[0]
    pred = R.predictions(case, grad=True)
    pred["priors"] = case["priors"][None].repeat(B, 1, 1)                                # what DataParallel hands the criterion
    net = R.stand_in_net(M)
    crit = mod.MultiBoxLoss(R.NUM_CLASSES, R.POS_T, R.NEG_T, R.RATIO)
    seen = {}
    inner = crit.multibox_loss

    def multibox_loss(*a, **k):
        out = inner(*a, **k)
        seen.update(conf_t=out[1].clone(), ids_t=out[2].clone(), idx_t=out[3].clone())
        return out

    crit.multibox_loss = multibox_loss
    with mock.patch.object(torch.Tensor, "get_device", lambda self: "cpu"):
        losses = crit(net, pred, *R.ground_truth(case))
    losses = {k: v.reshape(-1)[0] for k, v in losses.items()}
    sum(losses.values()).backward()
    grads = {k: pred[k].grad.detach().clone() for k in ("loc", "conf", "mask_coeff", "proto", "centerness", "track")}
    grads.update({f"net.{k}": v.grad.detach().clone() for k, v in net.TemporalNet.named_parameters()})
    return {k: v.detach() for k, v in losses.items()}, seen, grads


def frac(err, bound):
    live = bound > 0
    assert bool((err[~live] == 0).all())
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def find_case(name, spec, tries=400):
    for trial in range(tries):
        seed = R.GOLDEN_SEED0[name] + trial
        case = R.draw_case(spec, seed)
        n_b = (case["conf_t"] > 0).sum(1)
        if case["match_margin"] <= MATCH_MARGIN or int(n_b.min()) < 1 or (spec["big"] is not None and int(n_b[spec["big"][0]]) < 17):
            continue
        if CR.margin(case["conf"], case["conf_t"], R.RATIO) <= OHEM_MARGIN:
            continue
        B = len(spec["G"])
        comp = R.compose(case["loc"], case["mask_coeff"], case["proto"], case["priors"], case["conf_t"], case["idx_t"], sum(case["gt_masks"], []),
                         oracle.decode, R.MASK_ALPHA, 1.0 / B)
        if not comp["pred_ok"] or comp["min_edge"] < R.EDGE:
            continue
        tr = PR.restate_track(case["track"], case["conf_t"], case["ids_t"], R.ALPHAS["track_alpha"], 1.0)
        if tr["min_v"] <= TRACK_MIN_V:
            continue
        t2s = T2S.compose(R.t2s_case(case), R.stand_in_net(spec["M"], double=True).TemporalNet, oracle.decode, R.ALPHAS["boxshift_alpha"],
                          R.ALPHAS["maskshift_alpha"])
        if t2s["n"] == 0 or t2s["min_kink"] <= T2S.KINK:
            continue
        return seed, case, comp, tr, t2s
    raise SystemExit(f"{name}: no seed meets the input conditions")


def main():
    gen_golden.install_stubs()
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    import layers.modules.multibox_loss as mod
    from datasets import activation_func
    assert cfg.mask_proto_crop and cfg.mask_proto_crop_with_pred_box and cfg.mask_proto_mask_activation == activation_func.sigmoid
    assert not (cfg.use_maskiou or cfg.use_maskiou_loss or cfg.mask_proto_coeff_diversity_loss or cfg.use_mask_scoring or cfg.use_yolo_regressors)
    assert cfg.temporal_fusion_module and cfg.train_track and cfg.train_centerness and cfg.use_boxiou_loss and cfg.mask_proto_loss is None
    assert all(float(getattr(cfg, k)) == v for k, v in R.ALPHAS.items()), {k: getattr(cfg, k) for k in R.ALPHAS}
    out = dict(names=np.array(list(R.GOLDEN)), net_seed=np.int64(R.NET_SEED), **{k: np.float64(v) for k, v in R.ALPHAS.items()})

    for name, spec in R.GOLDEN.items():
        seed, case, comp, tr, t2s = find_case(name, spec)
        B, P = case["conf_t"].shape
        Md = spec["M"]
        H, W = spec["HW"]
        rows, img, n_b = comp["rows"], comp["img"], comp["n_b"]
        dev = {}
        # ---- 1: the mask term alone
        M_ref, box_ref, bce_ref = reference_mask_term(mod, case)
        assert torch.equal(box_ref, comp["box"]), name                                  # the crop boxes, bit for bit (oracle.decode + :560-563)
        red = R.restate_reduce(bce_ref, box_ref, comp["w"], n_b[img], H, W, R.MASK_ALPHA)
        dev["dev_M"] = float((M_ref.double() - red["M"]).abs() / red["M_bound"])
        dev["dev_M_inputs"] = float((M_ref.double() - comp["M"]).abs() / comp["M_bound"])
        dev["dev_bce"] = ML.worst_ratio(bce_ref, comp["bce"], comp["bce_mag"])
        # ---- 2: the whole forward
        losses, seen, grads = reference_forward(mod, case)
        for k in ("conf_t", "idx_t", "ids_t"):
            assert torch.equal(seen[k], case[k]), (name, k)                             # match_restate assigned what the reference assigned
        inv = 1.0 / B
        e = R.EPS
        dev["dev_M_forward"] = float((losses["M"].double() - comp["M"] * inv).abs() / (comp["M_bound"] * inv + e * comp["M"].abs() * inv))
        pos = rows
        dev["dev_grad_coeff"] = LR.worst_ratio(grads["mask_coeff"], comp["grad_coeff"], comp["grad_coeff_mag"])
        dev["dev_grad_proto"] = LR.worst_ratio(grads["proto"], comp["grad_proto"], comp["grad_proto_mag"])
        bx = PR.restate_box(case["loc"], case["priors"], case["gt_boxes_t"], case["conf_t"], case["centerness"], R.ALPHAS["bboxiou_alpha"],
                            R.ALPHAS["center_alpha"], inv, inv)
        dev["dev_BIoU"] = float((losses["BIoU"].double() - bx["biou"] * inv).abs() / (bx["biou_bound"] * inv + e * bx["biou"].abs() * inv))
        dev["dev_center"] = float((losses["center"].double() - bx["center"] * inv).abs() / (bx["center_bound"] * inv + e * bx["center"].abs() * inv))
        dev["dev_grad_loc"] = frac((grads["loc"].view(-1, 4).double() - bx["grad_loc"]).abs()[bx["pos"]], bx["grad_loc_bound"][bx["pos"]])
        dev["dev_grad_cent"] = frac((grads["centerness"].view(-1).double() - bx["grad_cent"]).abs()[bx["pos"]], bx["grad_cent_bound"][bx["pos"]])
        cf = CR.restate(case["conf"], case["conf_t"], R.RATIO, R.ALPHAS["conf_alpha"], "reference", inv)
        dev["dev_C"] = float((losses["C"].double() - cf["loss"] * inv).abs() / (cf["loss_bound"] * inv + e * cf["loss"].abs() * inv))
        gconf = grads["conf"].view(-1, R.NUM_CLASSES).double()
        dev["dev_grad_conf"] = float(((gconf - cf["grad"]).abs().max(1).values[cf["keep"]] / cf["grad_bound"][cf["keep"]]).max())
        assert not gconf[~cf["keep"]].any(), name
        dev["dev_T"] = float((losses["T"].double() - tr["loss"]).abs() / tr["loss_bound"])
        gtr = grads["track"].view(-1, R.EMBED).double()
        dev["dev_grad_track"] = frac((gtr - tr["grad"]).abs()[tr["pos"]], tr["grad_bound"][tr["pos"]])
        dev["e2e_loss"] = max(float((losses["B_shift"].double() - t2s["B"]).abs() / t2s["B"].abs()),
                              float((losses["M_shift"].double() - t2s["M"]).abs() / t2s["M"].abs()))
        dev["e2e_grad"] = max(float((grads[f"net.{k}"].double() - g).abs().max() / g.abs().max()) for k, g in t2s["grads"].items())
        assert all(v <= 1.0 for k, v in dev.items() if k.startswith("dev_")), (name, dev)
        nz = lambda g, width: g.reshape(-1, width)                                        # noqa: E731
        keep = dict(seed=np.int64(seed), shape=np.array([B, P, Md, *spec["proto"], H, W], dtype=np.int64), n=np.int64(comp["n"]),
                    conf_t=case["conf_t"].reshape(-1).to(torch.int16), idx_t=case["idx_t"].reshape(-1).to(torch.int16),
                    ids_t=case["ids_t"].reshape(-1).to(torch.int16), M_unbound=M_ref, ref_box=box_ref, ref_bce=bce_ref,
                    grad_loc_pos=nz(grads["loc"], 4)[pos], grad_mask_coeff_pos=nz(grads["mask_coeff"], Md)[pos],
                    grad_centerness_pos=nz(grads["centerness"], 1)[pos], grad_track_pos=nz(grads["track"], R.EMBED)[pos],
                    conf_rows=torch.nonzero(cf["keep"]).reshape(-1).to(torch.int32), grad_conf_rows=nz(grads["conf"], R.NUM_CLASSES)[cf["keep"]],
                    grad_proto=grads["proto"], match_margin=np.float64(case["match_margin"]), min_edge=np.float64(comp["min_edge"]))
        assert not nz(grads["loc"], 4)[conf_rows_not(pos, B * P)].any() and not nz(grads["mask_coeff"], Md)[conf_rows_not(pos, B * P)].any(), name
        keep.update({f"loss_{k}": v for k, v in losses.items()})
        keep.update({f"grad_{k.replace('.', '_')}": v for k, v in grads.items() if k.startswith("net.")})
        out.update({f"{name}__{k}": v for k, v in {**keep, **{k: np.float64(v) for k, v in dev.items()}}.items()})
        print(f"{name}: seed={seed} B={B} P={P} n={comp['n']} n_b={n_b.tolist()} " + " ".join(f"{k}={float(v):.5f}" for k, v in losses.items()))
        print("    " + " ".join(f"{k}={v:.3g}" for k, v in dev.items()))
    gen_golden.save("mbox_loss_cases.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "mbox_loss_cases.npz"))
    assert size < 1000 * 1000, size


def conf_rows_not(pos_rows, N):
    m = torch.ones(N, dtype=torch.bool)
    m[pos_rows] = False
    return m


if __name__ == "__main__":
    main()
