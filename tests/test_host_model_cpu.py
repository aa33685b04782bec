"""CPU-only parity of the host-side mirror (model wiring, heads, candidate generation, Fast-NMS plumbing, stateful
tracker) against goldens captured from the REFERENCE's own Python (tests/golden/gen_golden.py).  The four third-party
ops and the fused kernels are served by the oracle here (oracle.cpu_path), exactly as they were when the goldens were
generated, so any difference is a host-logic difference."""
import pytest
import torch

from conftest import load_golden
from oracle.cpu_path import oracle_ops
from stmask_amd import synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask

CASES = [("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada"),
         ("STMask_plus_resnet50_ali_config", "r50_ali"), ("STMask_plus_base_ali_config", "r101_ali")]


def run_clip(net, frames, dev="cpu"):
    outs = []
    with torch.no_grad():
        for t in range(frames.shape[0]):
            meta = [{"is_first": t == 0, "video_id": 0, "frame_id": t}]
            outs.append(net(frames[t:t + 1].to(dev), img_meta=meta)[0]["detection"])
    return outs


def check_clip_against_golden(outs, g, tol_box=1e-4, tol_mask=1e-4, exact_ids=True):
    for t, det in enumerate(outs):
        n_ref = g[f"t{t}_box"].shape[0]
        assert det["box"].shape[0] == n_ref, (t, det["box"].shape[0], n_ref)
        if n_ref == 0:
            continue
        assert torch.equal(det["class"].cpu(), g[f"t{t}_class"])
        if exact_ids:
            assert torch.equal(det["box_ids"].cpu(), g[f"t{t}_box_ids"])
        assert (det["box"].cpu() - g[f"t{t}_box"]).abs().max() < tol_box
        assert (det["score"].cpu() - g[f"t{t}_score"]).abs().max() < tol_box
        d = det["mask"].cpu() - g[f"t{t}_mask"]
        assert d.abs().max() < tol_mask and d.pow(2).sum(dim=(1, 2)).sqrt().max() < tol_mask * 10


@pytest.mark.parametrize("name,tag", CASES)
def test_model_matches_reference_on_cpu(name, tag):
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = STMask(get_cfg(name))
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0)
    with oracle_ops(), torch.no_grad():
        fpn_outs, po = net.forward_single(frames[:1])
        assert torch.equal(po["priors"][0], g["f0_priors"])
        for k, gk in [("loc", "f0_loc"), ("conf", "f0_conf_logits"), ("mask_coeff", "f0_mask_coeff"),
                      ("centerness", "f0_centerness"), ("proto", "f0_proto")]:
            assert (po[k][0] - g[gk]).abs().max() < 1e-5, k
        assert (po["track"][0][::7] - g["f0_track_s"]).abs().max() < 1e-5
        assert (fpn_outs[1][0, ::16] - g["f0_P4"]).abs().max() < 1e-5
        outs = run_clip(net, frames)
    check_clip_against_golden(outs, g, tol_box=1e-5, tol_mask=1e-5)


@pytest.mark.parametrize("name,tag", CASES[:2])
def test_batched_pipeline_matches_reference_on_cpu(name, tag):
    """BatchedClipPipeline (all clips in concatenated tensors, fused detect, one TF chain) == the reference's per-clip
    Detect_TF / Track_TF on its own clip, and two different clips batched together do not interact."""
    from stmask_amd.pipeline import BatchedClipPipeline, ClipPipeline
    from stmask_amd.dist import unpack_detections
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = STMask(get_cfg(name))
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    T = int(g["n_frames"])
    clip0 = synthetic.synthetic_clip(T, h, w, seed=0)
    clip1 = synthetic.synthetic_clip(T, h, w, seed=5)
    with oracle_ops(), torch.no_grad():
        pipe = BatchedClipPipeline(net, 2)
        ref_pipe = ClipPipeline(net, 2)
        for t in range(T):
            frames = torch.stack([clip0[t], clip1[t]])
            packed = pipe.step(frames)
            ref = ref_pipe.step(frames)
            dets = pipe.detections()
            # clip 0 against the reference golden
            n_ref = g[f"t{t}_box"].shape[0]
            assert dets[0]["box"].shape[0] == n_ref
            assert torch.equal(dets[0]["box_ids"], g[f"t{t}_box_ids"]) and torch.equal(dets[0]["class"], g[f"t{t}_class"])
            assert (dets[0]["box"] - g[f"t{t}_box"]).abs().max() < 1e-5
            assert (dets[0]["mask"] - g[f"t{t}_mask"]).abs().max() < 1e-5
            # both clips against the per-clip reference-shaped driver, and the packed (sync-free) output
            for b in range(2):
                assert torch.equal(dets[b]["box_ids"], ref[b]["box_ids"])
                assert (dets[b]["box"] - ref[b]["box"]).abs().max() < 1e-5
                assert (dets[b]["score"] - ref[b]["score"]).abs().max() < 1e-6
                un = unpack_detections(packed[b])
                n = min(len(ref[b]["box_ids"]), packed.shape[1])
                assert torch.equal(un["box_ids"][:n], ref[b]["box_ids"][:n]) and torch.equal(un["class"][:n], ref[b]["class"][:n])
                assert (un["box"][:n] - ref[b]["box"][:n]).abs().max() < 1e-5


def test_batchnorm_folding_keeps_reference_parity():
    """fuse.fold_batchnorm (53 BN kernels folded into conv / DCN weights) keeps the clip output within 1e-4 of the
    reference goldens, and is exact algebra on a bottleneck with non-trivial BN statistics."""
    from stmask_amd.backbone import Bottleneck
    from stmask_amd.fuse import fold_batchnorm
    name, tag = CASES[0]
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = STMask(get_cfg(name))
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0)
    assert fold_batchnorm(net) == 53
    assert not any(isinstance(m, torch.nn.BatchNorm2d) for m in net.modules())
    with oracle_ops(), torch.no_grad():
        outs = run_clip(net, frames)
    check_clip_against_golden(outs, g, tol_box=1e-4, tol_mask=1e-4)

    torch.manual_seed(0)
    blk = Bottleneck(16, 4, downsample=torch.nn.Sequential(torch.nn.Conv2d(16, 16, 1, bias=False),
                                                           torch.nn.BatchNorm2d(16)))
    blk.eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 2)
            m.weight.data.normal_()
            m.bias.data.normal_()
    x = torch.randn(2, 16, 9, 11)
    ref = blk(x.clone())

    class _BB:
        bn1, conv1, layers = torch.nn.Identity(), None, [[blk]]

    class _Net:
        training, backbone = False, _BB

    assert fold_batchnorm(_Net) == 4
    assert (blk(x.clone()) - ref).abs().max() < 1e-5


@pytest.mark.parametrize("name,tag", CASES[:2])
def test_optimized_inference_graph_keeps_reference_parity(name, tag):
    """fuse.optimize_for_inference (BN folded, conv bias + residual + ReLU as one epilogue pass) against the goldens."""
    from stmask_amd.fuse import optimize_for_inference
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = STMask(get_cfg(name))
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    keys_before = sorted(net.state_dict().keys())
    n_bn, n_fused = optimize_for_inference(net)
    assert n_bn == 53 and n_fused >= 60
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0)
    with oracle_ops(), torch.no_grad():
        outs = run_clip(net, frames)
    check_clip_against_golden(outs, g, tol_box=1e-4, tol_mask=1e-4)
    # parameter names survive (only BatchNorm entries disappear, conv biases appear)
    keys_after = set(net.state_dict().keys())
    assert all(k in keys_after for k in keys_before if ".bn" not in k and "downsample.1" not in k and "bn1" not in k)


def test_non_tf_detect_track_matches_reference_on_cpu():
    """Row a18: Detect.detect + Track.track (detection.py:98-137, track.py:56-179) over a 3-frame clip against the golden
    the reference's own methods produced (gen_golden.py model_nontf: Detect.__call__ itself raises KeyError('bbox_idx') at
    detection.py:91, so the generator drives detect(batch_idx, ...) and track(det, meta) directly, as __call__ would)."""
    g = load_golden("model_r50_fca_nontf.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    cfg = get_cfg("STMask_plus_resnet50_config")
    cfg.temporal_fusion_module = False
    net = STMask(cfg)
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0)
    with oracle_ops(), torch.no_grad():
        outs = run_clip(net, frames)
    for t, det in enumerate(outs):
        n_ref = g[f"t{t}_box"].shape[0]
        assert det["box"].shape[0] == n_ref and n_ref > 10, (t, det["box"].shape[0], n_ref)
        assert torch.equal(det["class"], g[f"t{t}_class"]) and torch.equal(det["box_ids"], g[f"t{t}_box_ids"])
        assert (det["box"] - g[f"t{t}_box"]).abs().max() < 1e-5 and (det["score"] - g[f"t{t}_score"]).abs().max() < 1e-5
        assert (det["mask_coeff"] - g[f"t{t}_mask_coeff"]).abs().max() < 1e-5
        assert (det["mask"] != g[f"t{t}_mask"]).sum() <= 2        # binary masks (track.py:88)
    assert outs[1]["box"].shape[0] < g["t1_nms_box"].shape[0]     # the clip exercises remove_false_inst (track.py:171-177)


def test_non_tf_detect_track_path_is_self_consistent():
    """Row a18, internal consistency besides the golden above: frame-0 detections get ids 0..n-1, ids persist on an
    unchanged second frame."""
    cfg = get_cfg("STMask_plus_resnet50_config")
    cfg.temporal_fusion_module = False
    net = STMask(cfg)
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    x = synthetic.synthetic_clip(1, 128, 192, seed=0)
    with oracle_ops(), torch.no_grad():
        d0 = net(x, img_meta=[{"is_first": True}])[0]["detection"]
        d1 = net(x, img_meta=[{"is_first": False}])[0]["detection"]
    n = d0["box"].shape[0]
    assert n > 5 and torch.equal(d0["box_ids"], torch.arange(n))
    assert d1["box"].shape[0] == n and torch.equal(d1["box_ids"], d0["box_ids"])   # identical frame -> same ids
    assert torch.equal(d1["box"], d0["box"]) and d0["mask"].shape == (n, 32, 48)


@pytest.mark.parametrize("fixture,zero_companion", [("model_full_tf16_r50_fca.npz", ()), ("model_full_tf_gaps_r50_fca.npz", (6,))])
def test_batched_pipeline_long_clip_matches_reference_on_cpu(fixture, zero_companion):
    """The benchmark's 16-frame full-size clip, and a clip with gaps (no detections on the first frame, first detections on a non-first frame, two
    frames without detections, re-matching after them), through BatchedClipPipeline beside a second clip, against the reference's own eval forward
    (gen_golden.py gen_model_full_tf): the host-side greedy matching, the frames-since-match counters, the keep rule and the packed output over the
    frames where the age-out, the score decay and the pixel rule first decide.  In the gaps clip, frame 6 has no detection in EITHER clip
    (the step keeps the shifted masks' bit words), frame 7 none in clip 0 alone."""
    from long_clip_check import golden_clips, rules_decided, run_long_clip
    from stmask_amd.pipeline import BatchedClipPipeline
    g = load_golden(fixture)
    net = STMask(get_cfg("STMask_plus_resnet50_config"))
    net.eval()
    synthetic.fill_state_dict(net, seed=0, bg_bias=synthetic.BENCH_BG_BIAS)
    decided, rematched = rules_decided(g)
    assert decided >= {2, 3} and rematched > 0, (decided, rematched)
    clips = golden_clips(g, zero_companion)
    with oracle_ops(), torch.no_grad():
        rep = run_long_clip(fixture, BatchedClipPipeline(net, 2), g, clips, tol=1e-5, mask_rms=1e-5, mask_abs=1e-5,
                            zero_companion=zero_companion)
    assert rep[f"t{int(g['n_frames']) - 1}"]["state_rows"] > 100
