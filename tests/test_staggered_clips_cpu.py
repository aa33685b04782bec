"""Per-clip is_first / active of BatchedClipPipeline on the CPU (the kernels served by the oracle, as in test_host_model_cpu): slot 0 switches
video at t = 4, slot 2 idles at t = 2..3 and starts a video at t = 4, slot 1 runs through.  Slot 1 is bit-identical to a run with a scalar
is_first at t = 0 only, slots 0 and 2 from t = 4 on to a run with a scalar reset at t = 4, and the idle slot reports nothing.  (The GPU
counterpart, with FCB-ada, graph replay and the module-path semantics, is tests/test_gpu_staggered_clips.py.)"""
import pytest
import torch

from oracle.cpu_path import oracle_ops
from stmask_amd import synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.pipeline import BatchedClipPipeline

H, W, T = 128, 192, 7


def batches():
    A, A2 = synthetic.synthetic_clip(4, H, W, seed=0), synthetic.synthetic_clip(3, H, W, seed=3)
    B, C, C2 = synthetic.synthetic_clip(T, H, W, seed=5), synthetic.synthetic_clip(2, H, W, seed=9), synthetic.synthetic_clip(3, H, W, seed=11)
    z = torch.zeros(3, H, W)
    return [torch.stack([A[t] if t < 4 else A2[t - 4], B[t], C[t] if t < 2 else (z if t < 4 else C2[t - 4])]) for t in range(T)]


def drive(net, xs, firsts, actives):
    pipe = BatchedClipPipeline(net, 3)
    declared = set(vars(pipe))
    out = []
    for t, x in enumerate(xs):
        y = pipe.step(x, is_first=firsts[t], active=actives[t])
        out.append((y.clone(), pipe.detections(), list(pipe.prev_n)))
    assert set(vars(pipe)) == declared          # all state is declared in __init__: no step creates an attribute
    return out


def same(r1, r2, b):
    d1, d2 = r1[1][b], r2[1][b]
    return torch.equal(r1[0][b], r2[0][b]) and d1.keys() == d2.keys() and all(torch.equal(d1[k], d2[k]) for k in d1)


@pytest.mark.parametrize("tf", [True, False], ids=["r50_fca_tf", "r50_non_tf"])
def test_staggered_clips_are_isolated_on_cpu(tf):
    cfg = get_cfg("STMask_plus_resnet50_config")
    cfg.temporal_fusion_module = tf
    net = STMask(cfg)
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    xs = batches()
    firsts = [True, [False] * 3, [False] * 3, [False] * 3, [True, False, True], [False] * 3, [False] * 3]
    actives = [None, None, [True, True, False], [True, True, False], None, None, None]
    with oracle_ops(), torch.no_grad():
        stag = drive(net, xs, firsts, actives)
        ref = drive(net, xs, [True] + [False] * (T - 1), [None] * T)
        rst = drive(net, xs, [t in (0, 4) for t in range(T)], [None] * T)
        lists = drive(net, xs[:3], [[True] * 3, [False] * 3, torch.zeros(3, dtype=torch.bool)], [None, [True] * 3, None])
    n1 = 0
    for t in range(T):
        assert same(stag[t], ref[t], 1), t
        n1 += stag[t][1][1]["box"].shape[0]
        if t < 4:
            assert same(stag[t], ref[t], 0), t
        else:
            assert same(stag[t], rst[t], 0) and same(stag[t], rst[t], 2), t
        if t in (2, 3):
            y, d, n = stag[t]
            assert not y[2].any() and n[2] == 0 and (not d[2] or d[2]["box"].shape[0] == 0), t
    assert n1 > 10
    for t in range(3):
        assert all(same(lists[t], ref[t], b) for b in range(3)) and lists[t][2] == ref[t][2], t
    with pytest.raises(ValueError):
        BatchedClipPipeline(net, 3).step(xs[0], is_first=[True, False])
