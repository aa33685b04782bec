"""Shared by tests/test_train_forward_cpu.py and tests/test_gpu_train_forward.py: the inputs of the train-forward goldens and the strided views
tests/golden/gen_train_forward_golden.py stored (STRIDES restated from it)."""
import torch

from stmask_amd import synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask

CASES = [("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada"), ("STMask_plus_resnet50_ali_config", "r50_ali")]
STRIDES = {"conf": 8, "mask_coeff": 8, "track": 32, "proto": 3, "t2s_channels": 4}
KEYS = ["T2S_concat_feat", "centerness", "conf", "loc", "mask_coeff", "priors", "proto", "track"]
VIEW_KEYS = ["loc", "centerness", "conf", "mask_coeff", "track", "proto", "T2S_concat_feat", "T2S_corr_clip0"]


def golden_input(g):
    h, w = [int(v) for v in g["frames_hw"]]
    return torch.stack([synthetic.synthetic_clip(2, h, w, seed=s) for s in (0, 1)])


def train_net(name, dev="cpu"):
    net = STMask(get_cfg(name))
    synthetic.fill_state_dict(net, seed=0)
    return net.to(dev).train()


def strided(out):
    s = STRIDES
    return {"loc": out["loc"], "centerness": out["centerness"], "conf": out["conf"][:, ::s["conf"]], "mask_coeff": out["mask_coeff"][:, ::s["mask_coeff"]],
            "track": out["track"][:, ::s["track"]], "proto": out["proto"][:, ::s["proto"], ::s["proto"]],
            "T2S_concat_feat": out["T2S_concat_feat"][:, ::s["t2s_channels"]], "T2S_corr_clip0": out["T2S_concat_feat"][0, :121]}


def bn_stats(net, g):
    last = dict(net.named_modules())[str(g["bn_last_name"].reshape(-1)[0])]
    first = net.backbone.bn1
    return {"bn_first_mean": first.running_mean, "bn_first_var": first.running_var, "bn_last_mean": last.running_mean, "bn_last_var": last.running_var}
