#!/usr/bin/env python3
"""Golden vectors of the reference's TRAIN-mode forward (STMask.py:285-309), made by importing the reference's own Python (build container only).

    python tests/golden/gen_train_forward_golden.py      # writes tests/golden/model_train_{r50_fca,r50_ada,r50_ali}.npz

The reference's STMask in .train() on 2 clips x 2 frames at 128x192 (synthetic.synthetic_clip seeds 0 and 1) with synthetic.fill_state_dict(net, 0),
under torch.no_grad(), the third-party ops served by the CPU oracle as in gen_golden.py (whose stub preamble is reused by import).  Stored: loc,
centerness and the priors' shape in full; conf, mask_coeff, track, proto strided (STRIDES below); T2S_concat_feat strided over channels plus the 121
correlation channels of clip 0 in full; the running statistics of backbone.bn1 and of the last BatchNorm2d of backbone.layers after the call.

dev_<key>: the largest difference between that fp32 run and a second run of the same net after .double() (same weights, the oracle ops cast to
fp32 and back): the reference's own rounding deviation, the yardstick the device run is held to (tests/test_gpu_train_forward.py)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import install_stubs, save  # noqa: E402  (also puts the repository root on sys.path)

import oracle.oracle as orc  # noqa: E402
from stmask_amd import synthetic  # noqa: E402

HW = (128, 192)
STRIDES = {"conf": 8, "mask_coeff": 8, "track": 32, "proto": 3, "t2s_channels": 4}


def strided(out):
    """The stored view of every key (the tests take the same views of their own outputs: tests/train_forward_views.py restates STRIDES)."""
    s = STRIDES
    return {"loc": out["loc"], "centerness": out["centerness"], "conf": out["conf"][:, ::s["conf"]], "mask_coeff": out["mask_coeff"][:, ::s["mask_coeff"]],
            "track": out["track"][:, ::s["track"]], "proto": out["proto"][:, ::s["proto"], ::s["proto"]],
            "T2S_concat_feat": out["T2S_concat_feat"][:, ::s["t2s_channels"]], "T2S_corr_clip0": out["T2S_concat_feat"][0, :121]}


def bn_stats(net):
    bns = [(n, m) for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and n.startswith("backbone.layers.")]
    first, (last_name, last) = net.backbone.bn1, bns[-1]
    return last_name, {"bn_first_mean": first.running_mean, "bn_first_var": first.running_var, "bn_last_mean": last.running_mean,
                       "bn_last_var": last.running_var}


def gen(cfg_name, tag):
    from datasets.config import cfg, set_cfg
    set_cfg(cfg_name)
    cfg.temporal_fusion_module = True
    import STMask as stmask_mod
    net = stmask_mod.STMask()
    net.train()
    synthetic.fill_state_dict(net, seed=0)
    x = torch.stack([synthetic.synthetic_clip(2, HW[0], HW[1], seed=s) for s in (0, 1)])          # [2, 2, 3, H, W]
    with torch.no_grad():
        out = net(x)
    keys = sorted(out)
    last_name, stats = bn_stats(net)
    stats = {k: v.clone() for k, v in stats.items()}
    got = {k: v.clone() for k, v in strided(out).items()}
    # ---- the same net in fp64: the oracle's C entry points take and return fp32, so they are wrapped to hand back the caller's dtype
    real_dc, real_cp = orc.deform_conv, orc.corr_patch
    orc.deform_conv = lambda x_, *a, **k: real_dc(x_, *a, **k).to(x_.dtype)
    orc.corr_patch = lambda f1, *a, **k: real_cp(f1, *a, **k).to(f1.dtype)
    try:
        synthetic.fill_state_dict(net, seed=0)                   # (the first call moved the running statistics)
        net.double()
        with torch.no_grad():
            out64 = net(x.double())
    finally:
        orc.deform_conv, orc.corr_patch = real_dc, real_cp
    dev = {f"dev_{k}": np.array(float((v.double() - strided(out64)[k]).abs().max())) for k, v in got.items()}
    print(tag, {k: float(v) for k, v in dev.items()})
    save(f"model_train_{tag}.npz", frames_hw=np.array(HW), keys=np.array(keys), priors_shape=np.array(out["priors"].shape),
         bn_last_name=np.array(last_name), **{k: v.float() for k, v in got.items()}, **stats, **dev)
    assert os.path.getsize(os.path.join(HERE, f"model_train_{tag}.npz")) < 1000 * 1000


def main():
    install_stubs()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for cfg_name, tag in (("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada"),
                          ("STMask_plus_resnet50_ali_config", "r50_ali")):
        if not sys.argv[1:] or tag in sys.argv[1:]:
            gen(cfg_name, tag)


if __name__ == "__main__":
    main()
