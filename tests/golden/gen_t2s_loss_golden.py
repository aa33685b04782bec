#!/usr/bin/env python3
"""Golden values of the temporal-fusion loss, from the REFERENCE's own code: MultiBoxLoss.track_to_segment_loss (layers/modules/multibox_loss.py
:247-326) called unbound on a namespace, unchanged, in fp32 on the CPU under STMask_plus_resnet50_config (build container only; the reference is
imported the way gen_golden.py imports it, so mmcv.ops.roi_align is the CPU oracle and carries no gradient: concat_feat gets none there):

    python tests/golden/gen_t2s_loss_golden.py            # writes tests/golden/t2s_loss_cases.npz

`net.TemporalNet` is the seeded stand-in of tests/t2s_loss_restate.py in fp32.  What the method forms on its way is recorded by wrapping the names
it looks up in its module (decode: the priors it selected, i.e. `pos`; F.smooth_l1_loss: `gt_bboxes_reg[pos]`; generate_mask: `bbox_t_next`, i.e.
`pos_idx_t`; F.binary_cross_entropy: the per-instance sums; the stand-in: bbox_reg) -- the wrappers pass everything through untouched.

Stored per case: the seed and shapes, the reference's two losses, its autograd gradients w.r.t. the stand-in's parameters, the targets it formed,
the rows its reductions saw (the stand-in's bbox_reg and the BCE sums), and its deviation from the restatement: dev_reg / dev_B / dev_M as fractions of the derived bounds (asserted <= 1), e2e_loss /
e2e_grad as the relative deviation from the fp64 composition (|x - x64| / |x64| for a loss, max |g - g64| / max |g64| per parameter tensor),
which is the yardstick of the end-to-end tolerance of tests/test_gpu_t2s_loss.py.  The fixture holds data only.
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
import oracle  # noqa: E402
import t2s_loss_restate as R  # noqa: E402


class _Proxy:
    def __init__(self, real, **over):
        self._real, self._over = real, over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(self._real, k)


def reference_run(mod, case, net32):
    """-> (B, M, parameter gradients or None, record)."""
    rec = dict(priors_p=[], reg=[], box_next=[], bce=[], bbox_reg=[])
    real_decode, real_gm, real_F = mod.decode, mod.generate_mask, mod.F

    def decode(loc, priors, *a, **k):
        rec["priors_p"].append(priors.detach().clone())
        return real_decode(loc, priors, *a, **k)

    def smooth_l1_loss(inp, tgt, **k):
        rec["reg"].append(tgt.detach().clone())
        return real_F.smooth_l1_loss(inp, tgt, **k)

    def generate_mask(proto, coeff, bbox=None):
        rec["box_next"].append(bbox.detach().clone())
        return real_gm(proto, coeff, bbox)

    def binary_cross_entropy(inp, tgt, **k):
        out = real_F.binary_cross_entropy(inp, tgt, **k)
        rec["bce"].append(out.detach().sum(dim=(1, 2)))
        return out

    def temporal_net(x):
        a, b = net32(x)
        rec["bbox_reg"].append(a.detach().clone())
        return a, b

    for p in net32.parameters():
        p.grad = None
    with mock.patch.object(mod, "decode", decode), mock.patch.object(mod, "generate_mask", generate_mask), \
            mock.patch.object(mod, "F", _Proxy(real_F, smooth_l1_loss=smooth_l1_loss, binary_cross_entropy=binary_cross_entropy)):
        losses = mod.MultiBoxLoss.track_to_segment_loss(types.SimpleNamespace(), types.SimpleNamespace(TemporalNet=temporal_net),
                                                        case["concat_feat"], case["loc_ref"], case["ids_t"], case["mask_coeff_ref"],
                                                        case["proto_next"], case["priors"], case["gt_bboxes"], case["gt_ids"], case["gt_masks"])
    B, M = losses["B_shift"], losses["M_shift"]
    grads = None
    if B.requires_grad and bool(torch.isfinite(B + M).all()):
        (B + M).sum().backward()
        grads = {k: v.grad.detach().clone() for k, v in net32.named_parameters()}
    return B.detach().reshape(-1)[0], M.detach().reshape(-1)[0], grads, rec


def frac(err, bound):
    live = bound > 0
    assert bool((err[~live] == 0).all())
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def main():
    gen_golden.install_stubs()
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    import layers.modules.multibox_loss as mod
    from datasets import activation_func
    assert cfg.maskshift_loss and cfg.mask_proto_crop and not cfg.use_yolo_regressors and cfg.mask_proto_mask_activation == activation_func.sigmoid
    ab, am = float(cfg.boxshift_alpha), float(cfg.maskshift_alpha)
    assert (ab, am) == (R.ALPHA_B, R.ALPHA_M), (ab, am)
    out = dict(names=np.array(list(R.GOLDEN)), boxshift_alpha=np.float64(ab), maskshift_alpha=np.float64(am), net_seed=np.int64(R.NET_SEED))

    for name, spec in R.GOLDEN.items():
        seed = R.find_seed(name, oracle.decode)
        case = R.golden_case(name, seed)
        bs, P = case["ids_t"].shape
        net32 = R.StandInNet(R.C_FEAT, spec["M"], R.NET_SEED)
        B, M, grads, rec = reference_run(mod, case, net32)
        comp = R.compose(case, R.StandInNet(R.C_FEAT, spec["M"], R.NET_SEED).double(), oracle.decode, ab, am)
        t, rows, n = comp["targets"], comp["rows"], comp["n"]
        keep = dict(seed=np.int64(seed), shape=np.array([bs, P, spec["M"], *spec["HW"]], dtype=np.int64), B=B, M=M, n=np.int64(n),
                    pos_rows=rows.to(torch.int32))
        dev = {}
        if n == 0:
            assert float(B) == 0.0 and float(M) == 0.0 and not rec["priors_p"], name
        else:
            # the targets the reference formed: pos (from the priors it selected), gt_bboxes_reg[pos], pos_idx_t (from bbox_t_next)
            clips = [i for i in range(bs) if bool(t["pos"][i].any())]
            assert len(rec["priors_p"]) == len(clips), name
            ref_rows, ref_k = [], []
            for i, pp, bn in zip(clips, rec["priors_p"], rec["box_next"]):
                for row, b in zip(pp, bn):
                    (p,) = torch.nonzero((case["priors"] == row).all(1)).reshape(-1).tolist()
                    ref_rows.append(i * P + p)
                    ref_k.append(torch.nonzero((case["gt_bboxes"][i][1] == b).all(1)).reshape(-1).tolist()[0])
            ref_reg = torch.cat(rec["reg"])
            assert ref_rows == rows.tolist(), name
            assert ref_k == t["k_local"].reshape(-1)[rows].tolist(), name
            assert torch.equal(ref_reg[:, :2], t["reg01"].reshape(-1, 2)[rows]), name
            reg64, regb = t["reg"].reshape(-1, 4)[rows], t["reg_bound"].reshape(-1, 4)[rows]
            finite = torch.isfinite(reg64)
            assert torch.equal(ref_reg.double()[~finite], reg64[~finite]), name          # log(0) = -inf on both sides
            err = torch.where(finite, ref_reg.double() - reg64, torch.zeros_like(reg64)).abs()
            dev["dev_reg"] = frac(err[:, 2:][finite[:, 2:]], regb[:, 2:][finite[:, 2:]])
            # the two reductions given the reference's own rows
            bbox_reg, bce = torch.cat(rec["bbox_reg"]), torch.cat(rec["bce"])
            H, W = spec["HW"]
            rl = R.restate_losses(bbox_reg, ref_reg, bce, comp["box_next"], comp["w"], comp["n_i"][comp["clip"]], bs, H, W, ab, am)
            if bool(torch.isfinite(rl["B"])):
                dev["dev_B"] = float((B.double() - rl["B"]).abs() / rl["B_bound"])
                dev["dev_M"] = float((M.double() - rl["M"]).abs() / rl["M_bound"])
                dev["e2e_loss"] = max(float((B.double() - comp["B"]).abs() / comp["B"].abs()), float((M.double() - comp["M"]).abs() / comp["M"].abs()))
                dev["e2e_grad"] = max(float((grads[k].double() - g).abs().max() / g.abs().max()) for k, g in comp["grads"].items())
                keep.update({f"grad_{k.replace('.', '_')}": v for k, v in grads.items()})
                assert comp["min_kink"] > R.KINK, name
            else:
                assert float(B) == float("inf") and float(M) == float("inf") and float(rl["B"]) == float("inf") and float(rl["M"]) == float("inf"), name
            keep.update(ref_reg=ref_reg, ref_k_local=np.array(ref_k, dtype=np.int32), ref_bbox_reg=bbox_reg, ref_bce=bce)
        assert all(v <= 1.0 for k, v in dev.items() if k.startswith("dev_")), (name, dev)
        out.update({f"{name}__{k}": v for k, v in {**keep, **{k: np.float64(v) for k, v in dev.items()}}.items()})
        print(f"{name}: seed={seed} bs={bs} P={P} n={n} B_shift={float(B):.6f} (composition {float(comp['B']):.6f}) M_shift={float(M):.6f} "
              f"(composition {float(comp['M']):.6f}) " + " ".join(f"{k}={v:.3g}" for k, v in dev.items()))
    gen_golden.save("t2s_loss_cases.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "t2s_loss_cases.npz"))
    assert size < 1024 * 1024, size


if __name__ == "__main__":
    main()
