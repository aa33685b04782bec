"""GPU parity against goldens captured from the REFERENCE's own Python (tests/golden/gen_golden.py), unconditional:

* head outputs / prototypes of the small clips at the tolerance the run achieves (north_star: protos within 1e-4);
* every clip frame: instances matched by box IoU, matched fraction asserted, box and soft-mask deltas asserted on EVERY pair;
* row a18 (Detect.detect / Track.track without temporal fusion) against its golden;
* one full-size frame per config (384x640 for R50-FCA / R50-FCB(ada) / R101-FCB(ali), and BASELINE config 5's
  736x1280 R101-FCB(ali) with N_p = 58 860 priors) through the planar inference graph: checksums, strided slices, detections;
* decode: per-fixture count of elements that differ from the reference's torch.exp path, and the proof that the HIP-decoded
  boxes give the reference's own NMS keep set.

Measured deltas are appended to gpurun_out/parity_report.json (scratch) so the tolerances written here can be audited.
"""
import json
import os

import pytest
import torch

import oracle
from conftest import ROOT, load_golden, ulp_diff
from stmask_amd import ops, synthetic
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from test_host_model_cpu import CASES, run_clip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def report(name, **vals):
    path = os.path.join(ROOT, "gpurun_out", "parity_report.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = {k: (float(v) if not isinstance(v, (list, str, dict)) else v) for k, v in vals.items()}
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def build(name, bg_bias=None, planar=None, temporal_fusion=True):
    cfg = get_cfg(name)
    cfg.temporal_fusion_module = temporal_fusion
    net = STMask(cfg)
    net.eval()
    synthetic.fill_state_dict(net, seed=0, bg_bias=bg_bias)
    net = net.to(DEV)
    if planar:
        from stmask_amd.fuse import optimize_for_inference
        optimize_for_inference(net, planar=True, planes=planar)
        net = net.to(memory_format=torch.channels_last)
        if temporal_fusion:
            net.TemporalNet = net.TemporalNet.to(memory_format=torch.contiguous_format)
    return net


def match_instances(got_box, got_cls, ref_box, ref_cls, thr=0.5):
    """Greedy one-to-one matching by box IoU (same class): returns (got rows, ref rows)."""
    if got_box.shape[0] == 0 or ref_box.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    iou = oracle.jaccard(got_box.contiguous(), ref_box.contiguous())
    iou = iou * (got_cls.view(-1, 1) == ref_cls.view(1, -1)).float()
    gi, ri, used = [], [], set()
    for i in torch.argsort(iou.max(dim=1).values, descending=True).tolist():
        order = torch.argsort(iou[i], descending=True).tolist()
        for j in order:
            if iou[i, j] <= thr:
                break
            if j not in used:
                used.add(j)
                gi.append(i)
                ri.append(j)
                break
    return torch.tensor(gi, dtype=torch.int64), torch.tensor(ri, dtype=torch.int64)


def soft_mask_delta(got, ref):
    """Soft masks are sigmoid outputs inside the crop box and exactly 0 outside.  A box that moves by 1e-6 can move the crop
    edge by one pixel row / column, which is a discontinuity of the reference's own function, not an error: compare the values
    where both sides are inside their crop, and count the pixels where only one side is (bounded by the box perimeter)."""
    both = (got != 0) & (ref != 0)
    d = (got - ref) * both
    n = both.sum(dim=(1, 2)).clamp(min=1)
    rms = (d.pow(2).sum(dim=(1, 2)) / n).sqrt()
    edge = ((got != 0) ^ (ref != 0)).sum(dim=(1, 2))
    return rms, d.abs().amax(dim=(1, 2)), edge


def check_frame(tag, det, g_box, g_cls, g_mask, min_frac, tol_box, tol_rms, tol_abs):
    n_ref = g_box.shape[0]
    n_got = det["box"].shape[0] if det["box"].numel() else 0
    if n_ref == 0:
        assert n_got <= 1, (tag, n_got)
        return dict(n_ref=0, n_got=n_got, matched=0)
    assert n_got > 0, tag
    gb, gc = det["box"].cpu(), det["class"].cpu()
    gi, ri = match_instances(gb, gc, g_box, g_cls)
    frac = len(gi) / n_ref
    assert frac >= min_frac and n_got - len(gi) <= max(1, round((1 - min_frac) * n_ref)), (tag, n_got, n_ref, len(gi))
    bd = (gb[gi] - g_box[ri]).abs().max().item()
    assert bd < tol_box, (tag, bd)
    rms, mx, edge = soft_mask_delta(det["mask"].cpu()[gi], g_mask[ri])
    assert rms.max().item() < tol_rms and mx.max().item() < tol_abs, (tag, rms.max().item(), mx.max().item())
    h, w = g_mask.shape[1:]
    assert edge.max().item() <= 2 * (h + w), (tag, edge.max().item())
    return dict(n_ref=n_ref, n_got=n_got, matched=len(gi), box=bd, mask_rms=rms.max().item(), mask_abs=mx.max().item(),
                crop_edge_pixels=int(edge.max()))


# ------------------------------------------------------------------------------------------------- small clips
# x max(1, |ref|max).  Measured on the MI355X (gpurun_out/parity_report.json, round 2): loc 1.3e-6, conf 1.1e-6, mask_coeff 1.5e-6,
# centerness 8.4e-6 (tanh of a 1-channel conv: the R101 trunk is the worst case), proto 1.5e-6 -- tolerances = ~6x that
HEAD_TOL = {"loc": 1e-5, "conf": 1e-5, "mask_coeff": 1e-5, "centerness": 5e-5, "proto": 1e-5}


@pytest.mark.parametrize("planar", [None, "fp16x2"])
@pytest.mark.parametrize("name,tag", CASES)
def test_head_outputs_match_reference_tight(name, tag, planar):
    """north_star: protos within 1e-4 of the reference (absolute, values are O(1)); the other head outputs at the same level
    relative to their range.  Module path (dense-conv library) and the planar fp16x2 inference graph."""
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = build(name, planar=planar)
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0).cuda()
    x = frames[:1].contiguous(memory_format=torch.channels_last) if planar else frames[:1]
    with torch.no_grad():
        fpn_outs, po = net.forward_single(x)
    assert torch.equal(po["priors"][0].cpu(), g["f0_priors"])
    errs = {}
    for k, gk in [("loc", "f0_loc"), ("conf", "f0_conf_logits"), ("mask_coeff", "f0_mask_coeff"),
                  ("centerness", "f0_centerness"), ("proto", "f0_proto")]:
        ref = g[gk]
        errs[k] = (po[k][0].cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    errs["P4"] = (fpn_outs[1][0, ::16].cpu() - g["f0_P4"]).abs().max().item()
    errs["track"] = (po["track"][0][::7].cpu() - g["f0_track_s"]).abs().max().item()
    report(f"head_{tag}_{planar or 'module'}", **errs)
    for k, tol in HEAD_TOL.items():
        assert errs[k] < tol, (k, errs[k])
    assert errs["P4"] < 8e-5 and errs["track"] < 3e-6, errs            # measured 1.5e-5 (|P4| ~ 10) / 4.9e-7
    assert (po["proto"][0].cpu() - g["f0_proto"]).abs().max().item() < 1e-4      # north_star, absolute


@pytest.mark.parametrize("planar", [None, "fp16x2"])
@pytest.mark.parametrize("name,tag", CASES)
def test_clip_detections_match_reference_every_pair(name, tag, planar):
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = build(name, planar=planar)
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0)
    if planar:
        frames = frames.contiguous(memory_format=torch.channels_last)
    outs = run_clip(net, frames, DEV)
    rep = {}
    for t, det in enumerate(outs):
        # measured: every instance matched, boxes 3.6e-7, mask RMS 1.6e-5, mask max-abs 3.9e-5, no crop-edge pixel
        r = check_frame((tag, t), det, g[f"t{t}_box"], g[f"t{t}_class"], g[f"t{t}_mask"], min_frac=0.98, tol_box=3e-6,
                        tol_rms=1e-4, tol_abs=2e-4)
        rep[f"t{t}"] = r
        # the tracker's ids: where the instance sets agree completely they must be the reference's
        if r["n_ref"] and r["matched"] == r["n_ref"] == r["n_got"]:
            assert det["box_ids"].cpu().tolist() == g[f"t{t}_box_ids"].tolist(), (tag, t)
    report(f"clip_{tag}_{planar or 'module'}", **rep)


# ------------------------------------------------------------------------------------------------- the pipeline bench.py times
@pytest.mark.parametrize("name,tag", [CASES[0], CASES[1], CASES[3]])
def test_batched_graph_pipeline_matches_reference_every_frame(name, tag):
    """The pipeline bench.py times -- BatchedClipPipeline over the planar fp16x2 inference graph, trunk replayed from HIP graphs,
    next frame's trunk prefetched on the side stream, tracker kernels of csrc/tracker.hip, deferred masks -- DIRECTLY against the
    reference's clip goldens, every frame: instances matched one to one, tracker ids, boxes 3e-6, soft masks 1e-4 RMS.  Two clips
    per step (the golden clip and another one: batching must not couple them); the clip is run as many times as it takes for the last
    pass to be replayed from the captured graphs on every frame (the first two trunks of a pipeline run eager, the next N_GRAPH_SLOTS
    capture one slot each)."""
    from stmask_amd.pipeline import BatchedClipPipeline
    g = load_golden(f"model_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    T = int(g["n_frames"])
    net = build(name, planar="fp16x2")
    clips = torch.stack([synthetic.synthetic_clip(T, h, w, seed=s) for s in (0, 3)]).cuda()
    frames = [clips[:, t].contiguous(memory_format=torch.channels_last) for t in range(T)]
    pipe = BatchedClipPipeline(net, 2)
    pipe.use_graph = True
    rep = {}
    n_rounds = -(-(2 + BatchedClipPipeline.N_GRAPH_SLOTS) // T) + 1
    for rnd in range(n_rounds):
        for t in range(T):
            nxt = frames[t + 1] if t + 1 < T else frames[0]            # the next pass starts with frame 0 again
            pipe.step(frames[t], is_first=(t == 0), next_frames=nxt)
            det = pipe.detections()[0]
            r = check_frame((tag, rnd, t), det, g[f"t{t}_box"], g[f"t{t}_class"], g[f"t{t}_mask"], min_frac=0.98, tol_box=3e-6,
                            tol_rms=1e-4, tol_abs=2e-4)
            if r["n_ref"] and r["matched"] == r["n_ref"] == r["n_got"]:
                assert det["box_ids"].cpu().tolist() == g[f"t{t}_box_ids"].tolist(), (tag, rnd, t)
                r["ids_checked"] = True
            rep[f"pass{rnd}_t{t}"] = r
    assert pipe.graph_active and len(pipe._graphs) == BatchedClipPipeline.N_GRAPH_SLOTS
    assert any(r.get("ids_checked") for k, r in rep.items() if k.startswith(f"pass{n_rounds - 1}"))
    report(f"batched_graph_{tag}", **rep)


# ------------------------------------------------------------------------------------------------- row a18
def test_non_tf_detect_track_matches_reference():
    """Detect.detect + Track.track (detection.py:98-137, track.py:56-179) on a 3-frame clip: after-NMS sets, tracker ids and
    binary masks against the golden the reference's own methods produced (gen_golden.py model_nontf)."""
    g = load_golden("model_r50_fca_nontf.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    net = build("STMask_plus_resnet50_config", temporal_fusion=False)
    frames = synthetic.synthetic_clip(int(g["n_frames"]), h, w, seed=0)
    outs = run_clip(net, frames, DEV)
    rep = {}
    for t, det in enumerate(outs):
        ref_box, ref_cls, ref_ids = g[f"t{t}_box"], g[f"t{t}_class"], g[f"t{t}_box_ids"]
        gb, gc = det["box"].cpu(), det["class"].cpu()
        gi, ri = match_instances(gb, gc, ref_box, ref_cls)
        n_ref = ref_box.shape[0]
        assert len(gi) >= 0.9 * n_ref and abs(gb.shape[0] - n_ref) <= max(1, n_ref // 10), (t, gb.shape[0], n_ref, len(gi))
        assert (gb[gi] - ref_box[ri]).abs().max() < 2e-4
        assert (det["score"].cpu()[gi] - g[f"t{t}_score"][ri]).abs().max() < 2e-4
        # binary masks (track.py:88: gt(0.5).float()): pixels may flip only where the soft value sits on the threshold
        gm, rm = det["mask"].cpu()[gi], g[f"t{t}_mask"][ri]
        flips = (gm != rm).sum(dim=(1, 2))
        assert flips.max().item() <= 2 * (gm.shape[1] + gm.shape[2]) and flips.float().mean().item() < 8, (t, flips.max().item())
        same = gb.shape[0] == n_ref == len(gi)
        if same:
            assert det["box_ids"].cpu()[gi].tolist() == ref_ids[ri].tolist(), t
        rep[f"t{t}"] = dict(n_ref=n_ref, n_got=gb.shape[0], matched=len(gi), max_flips=int(flips.max()), ids_checked=bool(same))
    assert any(r["ids_checked"] for r in rep.values())
    report("nontf_r50_fca", **rep)


# ------------------------------------------------------------------------------------------------- full size
FULL = [("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada"),
        ("STMask_plus_base_ali_config", "r101_ali"), ("STMask_plus_base_ali_config", "r101_ali_736x1280")]


@pytest.mark.parametrize("name,tag", FULL)
def test_full_size_frame_matches_reference(name, tag):
    """One full-size frame (the benchmark's weights) through the planar fp16x2 inference graph against the reference's forward:
    float64 checksums and strided slices of every head output, then the frame's detections.  The 736x1280 case is
    BASELINE config 5's geometry: R101-DCN FCB(ali), P3..P7 = 92x160 .. 6x10, N_p = 58 860 priors, proto 184x320."""
    g = load_golden(f"model_full_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    step = int(g["row_step"])
    net = build(name, bg_bias=synthetic.BENCH_BG_BIAS, planar="fp16x2")
    frame = synthetic.synthetic_clip(1, h, w, seed=0).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        fpn_outs, po = net.forward_single(frame)
    full = {"loc": po["loc"][0], "conf_logits": po["conf"][0], "mask_coeff": po["mask_coeff"][0],
            "centerness": po["centerness"][0], "track": po["track"][0], "proto": po["proto"][0], "P4": fpn_outs[1][0]}
    assert full["loc"].shape[0] == int(g["n_priors"])
    if h == 736:
        assert full["loc"].shape[0] == 58860 and tuple(po["proto"].shape[1:3]) == (184, 320)
    rep = {}
    for k, v in full.items():
        s, sa, mx = [float(x) for x in g[f"sum_{k}"]]
        v64 = v.double()
        # sum |.| is well conditioned: relative 1e-5; the signed sum is compared against the same scale
        rep[f"sumabs_{k}"] = abs(v64.abs().sum().item() - sa) / sa
        rep[f"sum_{k}"] = abs(v64.sum().item() - s) / sa
        assert rep[f"sumabs_{k}"] < 1e-6 and rep[f"sum_{k}"] < 1e-6, (k, rep)      # measured <= 2e-7
    slices = {"loc": full["loc"][::step], "conf_logits": full["conf_logits"][::step], "mask_coeff": full["mask_coeff"][::step],
              "centerness": full["centerness"][::step], "track": full["track"][::step, ::8], "proto": full["proto"][::4, ::4],
              "P4": full["P4"][::16]}
    for k, v in slices.items():
        ref = g[f"s_{k}"]
        rep[f"slice_{k}"] = (v.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert rep[f"slice_{k}"] < (5e-5 if k == "centerness" else 1e-5), (k, rep[f"slice_{k}"])   # measured 8e-6 / 1.1e-6
    assert (slices["proto"].cpu() - g["s_proto"]).abs().max().item() < 1e-4                    # north_star, absolute
    # detections of the frame (is_first: no temporal fusion yet, every detection is reported)
    with torch.no_grad():
        det = net(frame, img_meta=[{"is_first": True, "video_id": 0, "frame_id": 0}])[0]["detection"]
    n_ref_all = int(g["det_n"])
    n_got = det["box"].shape[0] if det["box"].numel() else 0
    assert abs(n_got - n_ref_all) <= max(1, n_ref_all // 50), (n_got, n_ref_all)       # measured: equal
    ref_box, ref_cls = g["det_box"], g["det_class"]
    gi, ri = match_instances(det["box"].cpu(), det["class"].cpu(), ref_box, ref_cls)
    assert len(gi) == ref_box.shape[0], (len(gi), ref_box.shape[0])                  # all 48 stored detections found
    assert (det["box"].cpu()[gi] - ref_box[ri]).abs().max() < 5e-6
    assert (det["score"].cpu()[gi] - g["det_score"][ri]).abs().max() < 5e-6
    rms, mx, edge = soft_mask_delta(det["mask"].cpu()[gi], g["det_mask"][ri])
    assert rms.max().item() < 1e-4 and mx.max().item() < 2e-4, (rms.max().item(), mx.max().item())   # measured 2.7e-5 / 4.9e-5
    rep.update(n_ref=n_ref_all, n_got=n_got, matched=len(gi), mask_rms=rms.max().item(), mask_abs=mx.max().item())
    report(f"full_{tag}", **rep)


def test_config5_batched_pipeline_at_736x1280():
    """BASELINE config 5 through the pipeline bench.py runs (BatchedClipPipeline, fused detect over N_p = 58 860 priors,
    temporal fusion on the 46x80 P4 level) for three frames of two clips: runs, finite, ids persist, and the first frame's
    detections equal the reference's full-size golden."""
    from stmask_amd.pipeline import BatchedClipPipeline
    g = load_golden("model_full_r101_ali_736x1280.npz")
    net = build("STMask_plus_base_ali_config", bg_bias=synthetic.BENCH_BG_BIAS, planar="fp16x2")
    clips = torch.stack([synthetic.synthetic_clip(3, 736, 1280, seed=s) for s in (0, 1)]).cuda()
    pipe = BatchedClipPipeline(net, 2)
    for t in range(3):
        packed = pipe.step(clips[:, t].contiguous(memory_format=torch.channels_last), is_first=(t == 0))
        dets = pipe.detections()
        assert torch.isfinite(packed).all()
        if t == 0:
            gi, ri = match_instances(dets[0]["box"].cpu(), dets[0]["class"].cpu(), g["det_box"], g["det_class"])
            assert len(gi) >= 0.95 * g["det_box"].shape[0]
            rms, mx, _ = soft_mask_delta(dets[0]["mask"].cpu()[gi], g["det_mask"][ri])
            assert rms.max().item() < 1e-4 and dets[0]["mask"].shape[1:] == (184, 320)
        for d in dets:
            assert d["box"].shape[0] > 0 and torch.isfinite(d["mask"]).all()
    assert sum(pipe.prev_n) >= sum(d["box"].shape[0] for d in dets)


def test_config5_fp16x1_backbone_at_736x1280_against_reference():
    """BASELINE config 5 at ITS OWN setting: R101-DCN FCB(ali), 736x1280 tensor (720x1280 image), the ResNet backbone's
    convolutions on ONE fp16 plane (planes="fp16x1": v_mfma_f32_16x16x32_f16, fp32 accumulate), FPN / proto-net / heads fp32-
    equivalent -- against the reference's full-size golden.  This is NOT an fp32-equivalent graph; stated tolerances: head
    outputs within 2e-2 of their range against the reference (fp16 activations through 101 layers; measured ~3e-3 at the small
    sizes), >= 85 % of the reference's stored detections found (IoU > 0.5, same class), their boxes within 2e-2 (normalised
    coordinates; measured 3e-4) and soft masks within 5e-2 RMS (measured 1.8e-2 .. 2.9e-2 for the worst instance, depending on
    which kernels carry the fp16 stem: the masks are sigmoids of a 32-term product sum of fp16-perturbed prototypes and coefficients)."""
    g = load_golden("model_full_r101_ali_736x1280.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    assert (h, w) == (736, 1280)
    step = int(g["row_step"])
    net = build("STMask_plus_base_ali_config", bg_bias=synthetic.BENCH_BG_BIAS, planar="fp16x1")
    assert net._planar_backbone.fmt == 2 and net._planar.fmt == 1
    frame = synthetic.synthetic_clip(1, h, w, seed=0).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        fpn_outs, po = net.forward_single(frame)
    assert po["loc"].shape[1] == 58860 and tuple(po["proto"].shape[1:3]) == (184, 320)
    slices = {"loc": po["loc"][0][::step], "conf_logits": po["conf"][0][::step], "mask_coeff": po["mask_coeff"][0][::step],
              "proto": po["proto"][0][::4, ::4], "P4": fpn_outs[1][0][::16]}
    rep = {}
    for k, v in slices.items():
        ref = g[f"s_{k}"]
        assert torch.isfinite(v).all(), k
        rep[f"slice_{k}"] = (v.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert 1e-6 < rep[f"slice_{k}"] < 2e-2, (k, rep[f"slice_{k}"])       # fp16-level, and really not the fp32-equivalent path
    with torch.no_grad():
        det = net(frame, img_meta=[{"is_first": True, "video_id": 0, "frame_id": 0}])[0]["detection"]
    ref_box, ref_cls = g["det_box"], g["det_class"]
    gi, ri = match_instances(det["box"].cpu(), det["class"].cpu(), ref_box, ref_cls)
    n_ref_all = int(g["det_n"])
    n_got = det["box"].shape[0] if det["box"].numel() else 0
    assert len(gi) >= 0.85 * ref_box.shape[0], (len(gi), ref_box.shape[0])
    assert abs(n_got - n_ref_all) <= max(2, round(0.15 * n_ref_all)), (n_got, n_ref_all)
    bd = (det["box"].cpu()[gi] - ref_box[ri]).abs().max().item()
    rms, mx, _ = soft_mask_delta(det["mask"].cpu()[gi], g["det_mask"][ri])
    assert bd < 2e-2 and rms.max().item() < 5e-2, (bd, rms.max().item())
    rep.update(n_ref=n_ref_all, n_got=n_got, stored_ref=int(ref_box.shape[0]), matched=len(gi), box=bd, mask_rms=rms.max().item(),
               mask_abs=mx.max().item())
    report("full_r101_ali_736x1280_fp16x1", **rep)


# ------------------------------------------------------------------------------------------------- decode vs reference
@pytest.mark.parametrize("p", ["c0_", "c1_", "c2_"])
def test_decode_difference_from_reference_is_counted_and_harmless(golden_postproc, p):
    """The reference decodes with torch.exp on the CPU (MKL VML, <= 1 ULP, not reproducible op for op); the HIP kernel uses the
    correctly rounded exp the oracle defines.  Per fixture: how many of the 1023 x 4 decoded values differ from the
    reference's (a handful, by 1 ULP of w / h), and the consequence that matters: candidate boxes decoded ON THE GPU, run
    through the GPU Fast NMS, give exactly the reference's keep set, classes and scores."""
    g = golden_postproc
    loc, pri, ref = g[p + "loc"], g["priors"], g[p + "boxes"]
    got = ops.decode(loc.to(DEV), pri.to(DEV)).cpu()
    diff = got != ref
    n_diff, n_rows = int(diff.sum()), int(diff.any(dim=1).sum())
    ulp = ulp_diff(got[:, 2:] - got[:, :2], ref[:, 2:] - ref[:, :2]).max().item()
    report(f"decode_{p}", elements=got.numel(), differing_elements=n_diff, differing_boxes=n_rows, max_ulp_wh=ulp,
           max_abs=(got - ref).abs().max().item())
    assert n_diff <= 0.03 * got.numel() and ulp <= 4
    # reference keep set = rows of its candidate list that survive its NMS (gen_golden.py: Detect_TF.detect)
    keep_idx, cand_ref, cc_box = g[p + "keep_idx"], g[p + "cand_box"], g[p + "cc_box"]
    ref_keep = [int(torch.nonzero((cand_ref == b).all(dim=1))[0]) for b in cc_box]
    cand_hip = got[keep_idx]
    idx, cls, sc, bx, cnt = ops.cc_fast_nms(g[p + "cand_conf"].to(DEV), cand_hip.to(DEV), g[p + "cand_centerness"].to(DEV), 0.5, 200)
    n = int(cnt)
    assert idx[:n].cpu().tolist() == ref_keep, "HIP-decoded boxes changed the NMS keep set"
    assert torch.equal(cls[:n].cpu(), g[p + "cc_class"]) and torch.equal(sc[:n].cpu(), g[p + "cc_score"])
    # ... and no IoU decision of the 200 x 200 triangle sits within the decode difference of the threshold
    top = torch.argsort(g[p + "cand_conf"][:, 1:].max(1).values * g[p + "cand_centerness"], descending=True)[:200]
    iou_ref, iou_hip = oracle.jaccard(cand_ref[top], cand_ref[top]), oracle.jaccard(cand_hip[top], cand_hip[top])
    assert torch.equal(iou_ref <= 0.5, iou_hip <= 0.5)
    # the fused kernel (decode + threshold + NMS in one chain) agrees as well
    cen = g[p + "centerness"].view(1, -1)
    f_idx, f_cls, f_sc, f_bx, f_cnt = ops.detect_cc(loc[None].to(DEV), pri.to(DEV), g[p + "conf"][None].to(DEV), cen.to(DEV), 0.05, 0.5, 200)
    assert int(f_cnt[0]) == n and f_idx[0, :n].cpu().tolist() == keep_idx[torch.tensor(ref_keep)].tolist()


@pytest.mark.parametrize("graph", ["off", "auto"])
def test_pipeline_is_bit_reproducible_run_to_run(graph):
    """Two passes of the benchmark's pipeline (16 clips) over the same clips on one net give bit-equal detection blocks at every step -- with the eager
    trunk on the side stream beside the tracker tail (rounds 3-5's default at this size) and with the trunk replayed from HIP graphs, two trunks in
    flight on two side streams (round 6's default: every slot has its own pool and workspaces, so concurrent replays share nothing).  Round 3's chain
    kernel once failed this one pass in ten (a counted wait on its LDS-DMA ring: DESIGN section 4, "Bottleneck chain"); `bench.py --world2-one-gpu`
    is the stricter form with a second process."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(["--clips", "16", "--steps", "6", "--warmup", "2", "--graph", graph])
    dev = torch.device("cuda:0")
    net = bench.build_net(args, dev)
    keeps = []
    for _ in range(2):
        run = bench.Runner(args, dev, 0, 1, 16, net=net)
        run.keep = []
        run.timed(args.warmup, args.steps)
        torch.cuda.synchronize()
        assert run.pipe.graph_active == (graph == "auto") and (graph == "off" or run.pipe.prefetch_depth == 2)
        keeps.append([k.clone() for k in run.keep])
        del run
    assert len(keeps[0]) == len(keeps[1]) >= 8          # (under graphs the runner adds capture steps in front of the timed region)
    for t, (a, b) in enumerate(zip(*keeps)):
        assert torch.equal(a, b), f"step {t}: max abs diff {(a - b).abs().max().item()}"


def test_trunk_branches_in_the_graph_are_bit_equal_to_the_plain_order(monkeypatch):
    """PlanarGraph.run puts proto-net beside the shared head and P6 / P7 beside the finer FPN levels on a second stream while the trunk's HIP graph
    is captured (small batches only: planar.TRUNK_BRANCHES).  Same kernels on the same data, separate split-K scratch per branch: the detection
    blocks of every step must equal those of the plain order bit for bit."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    from stmask_amd import planar
    args = bench.parse_args(["--clips", "2", "--steps", "6", "--warmup", "3"])
    dev = torch.device("cuda:0")
    net = bench.build_net(args, dev)
    keeps = []
    for branches in (0, 2):
        monkeypatch.setattr(planar, "TRUNK_BRANCHES", branches)
        run = bench.Runner(args, dev, 0, 1, 2, net=net)
        run.keep = []
        run.timed(args.warmup, args.steps)
        torch.cuda.synchronize()
        assert run.pipe.graph_active, "the trunk was not replayed from a graph: the branches were not exercised"
        keeps.append([k.clone() for k in run.keep])
        del run
    assert len(keeps[0]) == len(keeps[1]) >= 9          # warm-up + timed steps (+ the untimed steps during which the remaining graph slots are captured)
    for t, (a, b) in enumerate(zip(*keeps)):
        assert torch.equal(a, b), f"step {t}: max abs diff {(a - b).abs().max().item()}"


# ------------------------------------------------------------------------------------------------- full-size temporal fusion
FULL_TF = [("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada"), ("STMask_plus_base_ali_config", "r101_ali")]


@pytest.mark.parametrize("name,tag", FULL_TF)
def test_full_size_temporal_fusion_clip_matches_reference(name, tag):
    """Frames 0..2 of a FULL-SIZE 384x640 clip (the benchmark's weights) through the pipeline bench.py times, against the reference's own eval forward
    (gen_golden.py model_full_tf): frame 0 detects, frames 1-2 run CandidateShift (TF_utils.py:12-51) and Track_TF.track (track_TF.py:50-181) on the
    whole tracked set (~40 instances on R50-FCA, 120-200 on FCB-ada, ~100 on R101-FCB(ali)).  Checked per frame: the tracker's WHOLE state row by row (row = instance id:
    classes and frames-since-match counters equal, boxes / scores 5e-6, every soft mask's float64 sum and > 0.5 pixel count), then the reported
    instances (ids equal, boxes 5e-6, the stored soft masks 1e-4 RMS).  Two clips per step: batching must not couple them."""
    from stmask_amd.pipeline import BatchedClipPipeline
    g = load_golden(f"model_full_tf_{tag}.npz")
    h, w = [int(v) for v in g["frames_hw"]]
    T, n_masks = int(g["n_frames"]), int(g["n_masks"])
    net = build(name, bg_bias=synthetic.BENCH_BG_BIAS, planar="fp16x2")
    clips = torch.stack([synthetic.synthetic_clip(T, h, w, seed=s) for s in (0, 2)]).cuda()
    frames = [clips[:, t].contiguous(memory_format=torch.channels_last) for t in range(T)]
    pipe = BatchedClipPipeline(net, 2)
    rep = {}
    for t in range(T):
        pipe.step(frames[t], is_first=(t == 0), next_frames=frames[t + 1] if t + 1 < T else None)
        det = pipe.detections()[0]
        # -- the tracker's state of clip 0: rows [0, prev_n[0])
        n = pipe.prev_n[0]
        ref_n = g[f"t{t}_state_box"].shape[0]
        assert n == ref_n, (tag, t, n, ref_n)
        # rows whose match hangs on a comparison closer than fragile_eps (1e-4) IN THE REFERENCE'S OWN VALUES are recorded in the golden and excused;
        # with these weights there are none (smallest margin 8e-4), so every row is compared
        fragile = set(int(v) for v in g[f"t{t}_fragile_rows"].tolist())
        assert len(fragile) <= max(1, n // 50) and not bool(g[f"t{t}_count_fragile"]), (tag, t, sorted(fragile))
        ok = torch.tensor([i not in fragile for i in range(n)])
        st = {k: pipe.prev[k][:n].cpu() for k in ("box", "score", "class", "mask")}
        assert st["class"][ok].tolist() == g[f"t{t}_state_class"][ok].tolist(), (tag, t)
        assert [v for i, v in enumerate(pipe.tracked[0]) if i not in fragile] == [int(v) for i, v in enumerate(g[f"t{t}_state_tracked_mask"].tolist())
                                                                                    if i not in fragile], (tag, t)
        sb = (st["box"] - g[f"t{t}_state_box"])[ok].abs().max().item()
        ss = (st["score"] - g[f"t{t}_state_score"])[ok].abs().max().item()
        assert sb < 5e-6 and ss < 5e-6, (tag, t, sb, ss)
        ms, ref_ms = st["mask"].double(), g[f"t{t}_state_mask_sums"]
        area = ref_ms[:, 0].clamp(min=1.0)
        d_sum = ((ms.sum(dim=(1, 2)) - ref_ms[:, 0]).abs() / area)[ok].max().item()
        d_cnt = ((ms > 0.5).double().sum(dim=(1, 2)) - ref_ms[:, 2]).abs()[ok].max().item()
        # a crop edge may move by one pixel row / column when a box moves by 1e-6 (soft_mask_delta): the sums get the perimeter's worth of slack
        assert d_sum < 2e-2 and d_cnt <= 2 * (ms.shape[1] + ms.shape[2]), (tag, t, d_sum, d_cnt)
        # -- the reported instances
        if fragile:
            continue
        assert det["box_ids"].cpu().tolist() == g[f"t{t}_box_ids"].tolist(), (tag, t)
        assert det["class"].cpu().tolist() == g[f"t{t}_class"].tolist(), (tag, t)
        bd = (det["box"].cpu() - g[f"t{t}_box"]).abs().max().item()
        assert bd < 5e-6, (tag, t, bd)
        rms, mx, edge = soft_mask_delta(det["mask"].cpu()[:n_masks], g[f"t{t}_mask"])
        assert rms.max().item() < 1e-4 and mx.max().item() < 2e-4, (tag, t, rms.max().item(), mx.max().item())
        rep[f"t{t}"] = dict(state_rows=n, reported=len(g[f"t{t}_box_ids"]), state_box=sb, state_score=ss, mask_sum_rel=d_sum, mask_count=d_cnt, box=bd,
                            mask_rms=rms.max().item(), mask_abs=mx.max().item(), crop_edge_pixels=int(edge.max()))
    assert rep[f"t{T - 1}"]["state_rows"] > rep["t0"]["state_rows"]          # the later frames DID run the temporal fusion on a grown tracked set
    report(f"full_tf_{tag}", **rep)
