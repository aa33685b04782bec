#!/usr/bin/env python3
"""Generate golden vectors by importing the REFERENCE's own Python (build container only).

    python tests/golden/gen_golden.py            # writes tests/golden/*.npz
    python tests/golden/gen_golden.py model_full_tf model_full_tf16 model_full_tf_gaps model_full_tf_r101   # the full-size TF clips (CPU, ~2 min)

The reference (/root/reference) never travels to the GPU box; only the small .npz files
written here do.  They hold inputs + the outputs of the reference's torch code for the
hot-path functions:

  postproc.npz   decode / center_size / jaccard / sanitize_coordinates_hw / crop /
                 generate_candidate / Detect_TF.detect (cross-class and per-class) /
                 generate_mask / mask_iou on seeded synthetic head outputs
  priors.npz     PredictionModule_FC.make_priors for the five 384x640 level sizes
  fcb_ali.npz    FeatureAlign "ali" offset construction for 3x3 / 3x5 / 5x3
  model_*.npz    STMask.forward (eval) over a seeded 3-frame clip at reduced size for the
                 benchmark configs, with the four third-party ops replaced by the CPU
                 oracle (dcn_v2 / mmcv / spatial_correlation_sampler are not installed
                 anywhere -- "parity unpinned" for those, see oracle/stm_oracle.c)

The reference has no CPU path (STMask.py:15, TF_utils.py:105,109), so the stub preamble
below fakes the CUDA-only bits; nothing of the reference is copied.
"""
import collections
import collections.abc
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

import oracle  # noqa: E402
from stmask_amd import synthetic  # noqa: E402


# ----------------------------------------------------------------------------- stubs
def install_stubs():
    sys.path.insert(0, REF)
    collections.Sequence = collections.abc.Sequence
    np.int = int
    np.float = float
    torch.cuda.current_device = lambda: "cpu"  # TF_utils.py:105,109 pass it as device=

    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return None

    def stub(name, **kw):
        m = _Any(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m

    stub("dcn_v2", DCN=oracle.OracleDCN, DCNv2=oracle.OracleDCN)
    mm = stub("mmcv")
    mm.is_str = lambda x: isinstance(x, str)
    mm.is_list_of = lambda a, b: True
    stub("mmcv.ops", DeformConv2d=oracle.OracleDeformConv2d, roi_align=oracle.roi_align)
    stub("mmcv.runner")
    stub("mmcv.parallel", DataContainer=object)
    stub("spatial_correlation_sampler", spatial_correlation_sample=oracle.spatial_correlation_sample)
    for n in ["cocoapi", "cocoapi.PythonAPI", "cocoapi.PythonAPI.pycocotools", "pycocotools", "pycocotools.mask",
              "cv2", "pyximport"]:
        stub(n)
    sys.modules["pyximport"].install = lambda *a, **k: None
    stub("cocoapi.PythonAPI.pycocotools.ytvos", YTVOS=object)
    stub("cocoapi.PythonAPI.pycocotools.ytvoseval", YTVOSeval=object)
    stub("pycocotools.coco", COCO=object)
    stub("pycocotools.cocoeval", COCOeval=object)
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")
    stub("utils.cython_nms", nms=None)
    import matplotlib  # noqa: F401  (reference imports pyplot at module scope)


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.ascontiguousarray(v)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB, keys={sorted(out)}")


# ----------------------------------------------------------------------------- post-processing
def synth_head_outputs(n_priors_hw, seed, n_hot=400):
    """Seeded synthetic head outputs shaped like forward_single's: loc, softmaxed conf, centerness,
    mask_coeff, track; priors come from the reference's own make_priors."""
    g = torch.Generator().manual_seed(seed)
    N = sum(h * w for h, w in n_priors_hw) * 3
    loc = torch.randn(N, 4, generator=g) * torch.tensor([1.0, 1.0, 1.5, 1.5])
    logits = torch.randn(N, 41, generator=g)
    hot = torch.randperm(N, generator=g)[:n_hot]
    cls = torch.randint(1, 41, (n_hot,), generator=g)
    logits[hot, cls] += torch.rand(n_hot, generator=g) * 6 + 2
    conf = torch.softmax(logits, -1)
    centerness = torch.tanh(torch.randn(N, 1, generator=g) + 1.0)
    coeff = torch.randn(N, 32, generator=g)
    track = torch.nn.functional.normalize(torch.randn(N, 128, generator=g), dim=-1)
    return loc, conf, centerness, coeff, track


def gen_postproc():
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.box_utils import decode, center_size, jaccard, sanitize_coordinates_hw, crop, mask_iou
    from layers.mask_utils import generate_mask
    from layers.functions import Detect_TF, generate_candidate
    from layers.modules import PredictionModule_FC

    # priors from the reference's own Python loop (prediction_head_FC.py:224-247)
    levels = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]  # reduced pyramid: 1023 priors
    pm = PredictionModule_FC.__new__(PredictionModule_FC)
    pm.pred_aspect_ratios = cfg.backbone.pred_aspect_ratios[0]
    pm.pred_scales = cfg.backbone.pred_scales[0]
    priors = torch.cat([pm.make_priors(h, w, "cpu") for h, w in levels], 1)  # [1,N,4]

    out = {}
    for case, (seed, n_hot) in enumerate([(11, 300), (12, 40), (13, 900)]):
        loc, conf, cen, coeff, track = synth_head_outputs(levels, seed, n_hot)
        g = torch.Generator().manual_seed(100 + seed)
        proto = torch.relu(torch.randn(24, 40, 32, generator=g))
        boxes = decode(loc, priors[0])
        preds = {"loc": loc[None], "conf": conf[None], "priors": priors, "mask_coeff": coeff[None],
                 "track": track[None], "centerness": cen[None], "proto": proto[None],
                 "T2S_feat": torch.zeros(1, 1, 2, 2), "fpn_feat": torch.zeros(1, 1, 2, 2)}
        cand = generate_candidate(preds)[0]
        keep_idx = torch.nonzero(conf[:, 1:].max(1)[0] > cfg.eval_conf_thresh).view(-1)
        det = Detect_TF(cfg.num_classes, bkg_label=0, top_k=cfg.nms_top_k, conf_thresh=cfg.nms_conf_thresh,
                        nms_thresh=cfg.nms_thresh)
        cc = det.detect(dict(cand))
        det.use_cross_class_nms = False
        pc = det.detect(dict(cand))
        masks = generate_mask(cand["proto"], cc["mask_coeff"], cc["box"])
        masks_nocrop = generate_mask(cand["proto"], cc["mask_coeff"][:5], None)
        bin_m = masks.gt(0.5).float()
        miou = mask_iou(bin_m[: min(20, len(bin_m))], bin_m)
        p = f"c{case}_"
        out.update({
            p + "loc": loc, p + "conf": conf, p + "centerness": cen, p + "mask_coeff": coeff,
            p + "track": track[:, :8], p + "proto": proto, p + "boxes": boxes,
            p + "center_size": center_size(boxes), p + "keep_idx": keep_idx,
            p + "cand_box": cand["box"], p + "cand_conf": cand["conf"], p + "cand_centerness": cand["centerness"],
            p + "cc_box": cc["box"], p + "cc_class": cc["class"], p + "cc_score": cc["score"],
            p + "cc_mask_coeff": cc["mask_coeff"], p + "cc_centerness": cc["centerness"],
            p + "pc_box": pc["box"], p + "pc_class": pc["class"], p + "pc_score": pc["score"],
            p + "masks": masks, p + "masks_nocrop": masks_nocrop, p + "mask_iou": miou,
            p + "jaccard": jaccard(cand["box"][:64], cand["box"][:96]),
            p + "sanitize_hw": sanitize_coordinates_hw(cc["box"], 24, 40),
        })
    out["priors"] = priors[0]
    out["levels"] = np.array(levels)
    # crop boundary known-answer case (boxes touching 0 / 1, swapped corners)
    kb = torch.tensor([[0.0, 0.0, 1.0, 1.0], [0.5, 0.25, 0.25, 0.75], [0.0, 0.0, 0.024, 0.04],
                       [0.98, 0.97, 1.0, 1.0], [0.3, 0.3, 0.3, 0.3]])
    ones = torch.ones(24, 40, 5)
    cm, _ = crop(ones, kb)
    out["crop_boxes"] = kb
    out["crop_mask"] = cm.permute(2, 0, 1).contiguous()
    save("postproc.npz", **out)


def gen_postproc_nontf():
    """Row a18's per-class Fast NMS: the reference's own Detect.fast_nms (detection.py:211-261) -- which, unlike Detect_TF.fast_nms, ranks by the
    raw class confidences WITHOUT centerness -- on the stored inputs of postproc.npz (outputs only go into postproc_nontf.npz)."""
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.functions import Detect
    z = np.load(os.path.join(HERE, "postproc.npz"))
    out = {}
    for case in range(3):
        p = f"c{case}_"
        conf, boxes = torch.from_numpy(z[p + "conf"]), torch.from_numpy(z[p + "boxes"])
        coeff = torch.from_numpy(z[p + "mask_coeff"])
        track = torch.nn.functional.normalize(torch.randn(conf.shape[0], 8), dim=-1)        # (carried along only)
        keep = conf[:, 1:].max(1)[0] > cfg.nms_conf_thresh                                   # Detect.detect, detection.py:104-108
        det = Detect(cfg.num_classes, bkg_label=0, top_k=cfg.nms_top_k, conf_thresh=cfg.nms_conf_thresh, nms_thresh=cfg.nms_thresh)
        r = det.fast_nms(boxes[keep], coeff[keep], track[keep], conf[keep, 1:].t().contiguous(), det.nms_thresh, det.top_k)
        out.update({p + "pcn_box": r["box"], p + "pcn_class": r["class"], p + "pcn_score": r["score"], p + "pcn_mask_coeff": r["mask_coeff"]})
    save("postproc_nontf.npz", **out)


def gen_priors():
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.modules import PredictionModule_FC
    pm = PredictionModule_FC.__new__(PredictionModule_FC)
    pm.pred_aspect_ratios = cfg.backbone.pred_aspect_ratios[0]
    pm.pred_scales = cfg.backbone.pred_scales[0]
    out = {}
    for h, w in [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]:
        out[f"p_{h}x{w}"] = pm.make_priors(h, w, "cpu")[0]
    save("priors.npz", **out)


def gen_fcb_ali():
    from datasets.config import set_cfg
    set_cfg("STMask_plus_resnet50_ali_config")
    from layers.modules import FeatureAlign
    out = {}
    g = torch.Generator().manual_seed(5)
    loc = torch.randn(2, 4, 6, 10, generator=g)
    out["loc"] = loc
    for kh, kw in [(3, 3), (3, 5), (5, 3)]:
        fa = FeatureAlign(8, 8, kernel_size=(kh, kw), deformable_groups=1, use_pred_offset=False)
        captured = {}
        fa.conv_adaption.forward = lambda x, off, _c=captured: (_c.__setitem__("off", off.clone()), x)[1]
        fa(torch.zeros(2, 8, 6, 10), loc)
        out[f"off_{kh}x{kw}"] = captured["off"]
    save("fcb_ali.npz", **out)


# ----------------------------------------------------------------------------- whole model
def gen_model(cfg_name, tag, hw=(128, 192), n_frames=3, temporal_fusion=True):
    from datasets.config import cfg, set_cfg
    set_cfg(cfg_name)
    cfg.temporal_fusion_module = temporal_fusion  # False: the reference's Detect / Track path (STMask.py:323-327)
    import STMask as stmask_mod
    net = stmask_mod.STMask()
    net.eval()
    sd = synthetic.fill_state_dict(net, seed=0)
    frames = synthetic.synthetic_clip(n_frames, hw[0], hw[1], seed=0)
    out = {"frames_hw": np.array(hw), "n_frames": np.array(n_frames)}
    out["state_keys"] = np.array(sorted(sd.keys()))
    out["state_shapes"] = np.array([str(tuple(sd[k].shape)) for k in sorted(sd.keys())])
    with torch.no_grad():
        fpn_outs, po = net.forward_single(frames[:1])
        out["f0_loc"] = po["loc"][0]
        out["f0_conf_logits"] = po["conf"][0]
        out["f0_mask_coeff"] = po["mask_coeff"][0]
        out["f0_centerness"] = po["centerness"][0]
        out["f0_track_s"] = po["track"][0][::7]
        out["f0_proto"] = po["proto"][0]
        out["f0_priors"] = po["priors"][0]
        out["f0_P4"] = fpn_outs[1][0, ::16]
        for t in range(n_frames):
            meta = [{"is_first": t == 0, "video_id": 0, "frame_id": t}]
            res = net(frames[t:t + 1], img_meta=meta)[0]["detection"]
            for k in ("box", "score", "class", "box_ids", "mask_coeff", "mask", "centerness"):
                v = res.get(k, torch.zeros(0))
                v = torch.zeros(0) if v is None else v
                out[f"t{t}_{k}"] = v
            print(tag, "frame", t, "n_out", len(res["box"]))
    save(f"model_{tag}.npz", **out)


def gen_model_nontf(cfg_name, tag, hw=(128, 192), n_frames=3):
    """Row a18: the reference's non-TF post-processing, Detect.detect (detection.py:98-137) + Track.track (track.py:56-179).
    Detect.__call__ cannot run (it reads result['bbox_idx'], detection.py:91, a key cc_fast_nms never sets), so its body is
    driven from here exactly as __call__ does it (detection.py:69-90) minus that line: transpose conf, decode, detect(batch_idx,
    ...), result['proto'] = proto; then Track.track(result, meta) per frame as STMask.forward does (STMask.py:323-327)."""
    from datasets.config import cfg, set_cfg
    set_cfg(cfg_name)
    cfg.temporal_fusion_module = False
    import STMask as stmask_mod
    from layers.box_utils import decode
    net = stmask_mod.STMask()
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    frames = synthetic.synthetic_clip(n_frames, hw[0], hw[1], seed=0)
    out = {"frames_hw": np.array(hw), "n_frames": np.array(n_frames)}
    with torch.no_grad():
        for t in range(n_frames):
            _, po = net.forward_single(frames[t:t + 1])
            po["conf"] = torch.softmax(po["conf"], -1)
            po["mask_coeff"] = cfg.mask_proto_coeff_activation(po["mask_coeff"])      # STMask.py:324
            pri = po["priors"].squeeze(0)
            conf_t = po["conf"].view(1, pri.size(0), -1).transpose(2, 1).contiguous()   # detection.py:77-78
            boxes = decode(po["loc"][0], pri)
            res = net.detect.detect(0, conf_t, boxes, po["centerness"], po["mask_coeff"], po["track"], po["proto"], None)
            res["proto"] = po["proto"][0]
            out[f"t{t}_nms_box"], out[f"t{t}_nms_class"], out[f"t{t}_nms_score"] = res["box"], res["class"], res["score"]
            res = net.Track.track(res, {"is_first": t == 0, "video_id": 0, "frame_id": t})
            for k in ("box", "score", "class", "box_ids", "mask_coeff", "mask"):
                v = res.get(k, torch.zeros(0))
                out[f"t{t}_{k}"] = torch.zeros(0) if v is None else v
            print(tag, "frame", t, "n_nms", len(out[f"t{t}_nms_box"]), "n_out", len(res["box"]))
    save(f"model_{tag}.npz", **out)


def gen_model_full(cfg_name, tag, hw=(384, 640), row_step=16):
    """ONE full-size frame through the reference's STMask.forward (eval, oracle ops plugged in) at the benchmark's
    own weights (synthetic.BENCH_BG_BIAS).  Stored: float64 checksums (sum, sum |.|) of every head output, strided slices of
    them, and the frame's detections (boxes / classes / scores / soft masks)."""
    from datasets.config import cfg, set_cfg
    set_cfg(cfg_name)
    cfg.temporal_fusion_module = True
    import STMask as stmask_mod
    net = stmask_mod.STMask()
    net.eval()
    synthetic.fill_state_dict(net, seed=0, bg_bias=synthetic.BENCH_BG_BIAS)
    frame = synthetic.synthetic_clip(1, hw[0], hw[1], seed=0)
    out = {"frames_hw": np.array(hw), "row_step": np.array(row_step)}
    with torch.no_grad():
        fpn_outs, po = net.forward_single(frame)
        full = {"loc": po["loc"][0], "conf_logits": po["conf"][0], "mask_coeff": po["mask_coeff"][0],
                "centerness": po["centerness"][0], "track": po["track"][0], "proto": po["proto"][0], "P4": fpn_outs[1][0]}
        for k, v in full.items():
            out[f"sum_{k}"] = np.array([v.double().sum().item(), v.double().abs().sum().item(), float(v.abs().max())])
        for k in ("loc", "conf_logits", "mask_coeff", "centerness"):
            out[f"s_{k}"] = full[k][::row_step]
        out["s_track"] = full["track"][::row_step, ::8]
        out["s_proto"] = full["proto"][::4, ::4]
        out["s_P4"] = full["P4"][::16]
        out["n_priors"] = np.array(full["loc"].shape[0])
        res = net(frame, img_meta=[{"is_first": True, "video_id": 0, "frame_id": 0}])[0]["detection"]
        n = min(len(res["box"]), 48)
        for k in ("box", "score", "class", "box_ids", "mask_coeff", "mask", "centerness"):
            out[f"det_{k}"] = res[k][:n]
        out["det_n"] = np.array(len(res["box"]))
        print(tag, "full-size frame", hw, "priors", full["loc"].shape[0], "detections", len(res["box"]))
    save(f"model_full_{tag}.npz", **out)


FRAGILE_EPS = 1e-4
SCORE_EPS = 1e-5


def _row_mask_stats(m):
    """float64 (sum, sum of squares, count > 0.5) of every soft mask [n, h, w]."""
    m = m.double()
    return torch.stack([m.sum(dim=(1, 2)), m.pow(2).sum(dim=(1, 2)), (m > 0.5).double().sum(dim=(1, 2))], 1)


def gen_model_full_tf(cfg_name, name, hw=(384, 640), frame_src=3, clip_seed=0, n_masks=32, mask_frames=None, expect=None, coeff_sums=False):
    """a FULL-SIZE clip through the reference's eval forward (STMask.py:310-329) with the benchmark's weights: the first frame
    detects, the later ones run CandidateShift (TF_utils.py:12-51: correlation, RoIAlign, TemporalNet, decode, lincomb on the current prototypes)
    and Track_TF.track (track_TF.py:50-181: comp scores, greedy resolution, ids, keep rule) on the whole tracked set.

    frame_src: the frames fed, as indices into synthetic_clip(max + 1, *hw, seed=clip_seed) with -1 for an all-zero frame (no detections with these
    weights), or an int T for frames 0..T-1.  Stored per frame: every tracked instance's box / score / class / id / coefficients / centerness, float64
    checksums (sum, sum of squares, count of pixels > 0.5) of EVERY soft mask, the first n_masks reported soft masks whole on mask_frames (default:
    every frame), checksums of the frame's head outputs, the tracker's whole state after the frame, which rows the keep rule (track_TF.py:160-164)
    dropped for one condition alone (only_cond1 / 2 / 3), the rows excused from exact comparison (see below) and which branch of Track_TF.track ran
    (spied: CandidateShift calls, prev_candidate before / after).  expect: {frame: branch} the generator asserts.  coeff_sums (the long clips, to keep
    the files small): every row's 32 mask coefficients are stored as their float64 (sum, sum |.|) -- *_mask_coeff_sums -- and the reported rows'
    centerness is left out.

    The default clip seed 0 gives no count-fragile frame for the shipped fixtures; if a change of weights makes one appear, the generator stops:
    pick another clip seed here rather than loosening the test."""
    from datasets.config import cfg, set_cfg
    set_cfg(cfg_name)
    cfg.temporal_fusion_module = True
    import STMask as stmask_mod
    net = stmask_mod.STMask()
    net.eval()
    synthetic.fill_state_dict(net, seed=0, bg_bias=synthetic.BENCH_BG_BIAS)
    src = list(range(frame_src)) if isinstance(frame_src, int) else list(frame_src)
    clip = synthetic.synthetic_clip(max(src) + 1, hw[0], hw[1], seed=clip_seed)
    frames = torch.stack([clip[s] if s >= 0 else torch.zeros_like(clip[0]) for s in src])
    n_frames = len(src)
    mask_frames = list(range(n_frames)) if mask_frames is None else list(mask_frames)
    out = {"frames_hw": np.array(hw), "n_frames": np.array(n_frames), "n_masks": np.array(n_masks), "fragile_eps": np.array(FRAGILE_EPS)}
    extra = {"frame_src": np.array(src, dtype=np.int64), "clip_seed": np.array(clip_seed), "mask_frames": np.array(mask_frames, dtype=np.int64),
             "score_eps": np.array(SCORE_EPS)}
    # Which rows of the tracker state hang on a near-tie.  Track_TF.track decides by argmax over comp scores (track_TF.py:125) and, among detections that
    # pick the same object, by det_score > best (track_TF.py:141); with 120-200 overlapping instances some of those comparisons are closer than the
    # ~1e-6 by which two correct fp32 implementations of the trunk differ.  Recorded from the reference's OWN values, per frame: the rows whose outcome
    # a perturbation below FRAGILE_EPS could change (the test compares all other rows exactly) and whether the row COUNT could change.
    # (fragile_rows: the matching decisions of that frame alone; excused_rows: every kind -- matching, the score threshold of cond3 within SCORE_EPS,
    # a > 0.5 pixel count of cond2 that a pixel within FRAGILE_EPS of 0.5 could move across 1 -- and sticky: a row once fragile stays excused.)
    import layers.functions.track_TF as ttf
    seen = {}
    real_ccs, real_shift = ttf.compute_comp_scores, ttf.CandidateShift

    def spy(match_ll, bbox_scores, *a, **k):
        comp = real_ccs(match_ll, bbox_scores, *a, **k)
        seen["comp"], seen["score"] = comp.clone(), bbox_scores.view(-1).clone()
        return comp

    def spy_shift(*a, **k):
        seen["shift"] = seen.get("shift", 0) + 1
        return real_shift(*a, **k)

    tracker = net.Track_TF
    real_track = tracker.track

    def spy_track(net_, candidate, img_meta, img=None):
        seen["n_cand"] = candidate["box"].nelement() // 4 if candidate["box"].dim() else 0
        seen["prev_before"] = tracker.prev_candidate is not None and not img_meta["is_first"]
        r = real_track(net_, candidate, img_meta, img=img)
        seen["prev_after"] = tracker.prev_candidate is not None
        return r

    real_fs = net.forward_single

    def spy_fs(x):
        fpn_outs, po = real_fs(x)
        seen["sums"] = {k: po[k][0].double() for k in ("loc", "conf", "mask_coeff", "centerness", "proto")}
        seen["sums"] = {k: np.array([v.sum().item(), v.abs().sum().item()]) for k, v in seen["sums"].items()}
        return fpn_outs, po

    ttf.compute_comp_scores, ttf.CandidateShift = spy, spy_shift
    tracker.track = spy_track
    net.forward_single = spy_fs
    excused, branches, any_count_fragile, prev_tm = set(), [], False, []
    with torch.no_grad():
        for t in range(n_frames):
            seen.clear()
            res = net(frames[t:t + 1], img_meta=[{"is_first": t == 0, "video_id": 0, "frame_id": t}])[0]["detection"]
            for k in ("loc", "conf", "mask_coeff", "centerness", "proto"):
                out[f"t{t}_sum_{k}"] = seen["sums"][k]
            # which branch of Track_TF.track ran (track_TF.py:56-66 / 88-93 / 96-156), from the spies, not inferred from the outputs
            shifted, matched = seen.get("shift", 0), "comp" in seen
            if seen["n_cand"] == 0 and not seen["prev_before"]:
                br = "empty_first"                  # :56-58, nothing tracked and nothing detected
                assert shifted == 0 and not matched and not seen["prev_after"]
            elif seen["n_cand"] == 0:
                br = "empty_shift"                  # :61-66, CandidateShift and no matching
                assert shifted == 1 and not matched and seen["prev_after"]
            elif not seen["prev_before"]:
                br = "first" if t == 0 else "first_late"   # :88-93 (first_late: is_first False, prev_candidate None)
                assert shifted == 0 and not matched and seen["prev_after"]
            else:
                br = "match"
                assert shifted == 1 and matched
            branches.append(br)
            if expect is not None and t in expect:
                assert br == expect[t], (name, t, br, expect[t])
            n_rep = len(res["box"]) if res["box"].nelement() else 0
            for k in ("box", "score", "class", "box_ids", "mask_coeff", "centerness"):
                v = res.get(k, torch.zeros(0))
                out[f"t{t}_{k}"] = v if n_rep else v.new_zeros((0,) + ((4,) if k == "box" else (32,) if k == "mask_coeff" else ()))
            if n_rep:
                out[f"t{t}_mask_sums"] = _row_mask_stats(res["mask"])
            else:
                out[f"t{t}_mask_sums"] = torch.zeros(0, 3, dtype=torch.float64)
            if t in mask_frames:
                out[f"t{t}_mask"] = res["mask"][:n_masks] if n_rep else torch.zeros(0, hw[0] // 4, hw[1] // 4)
            # the tracker's whole state after the frame (row = instance id): what CandidateShift moved and Track_TF.track matched / appended,
            # including the instances the keep rule (track_TF.py:168-178) holds back from the output
            st = tracker.prev_candidate
            if st is None:
                n_st = 0
                for k, shp in (("box", (0, 4)), ("score", (0,)), ("class", (0,)), ("mask_coeff", (0, 32)), ("tracked_mask", (0,))):
                    out[f"t{t}_state_{k}"] = torch.zeros(shp, dtype=torch.int64 if k == "class" else torch.float32)
                out[f"t{t}_state_mask_sums"] = torch.zeros(0, 3, dtype=torch.float64)
            else:
                n_st = len(st["box"])
                for k in ("box", "score", "class", "mask_coeff", "tracked_mask"):
                    out[f"t{t}_state_{k}"] = st[k].clone()          # (the next frame updates matched rows IN PLACE: track_TF.py:150)
                out[f"t{t}_state_mask_sums"] = _row_mask_stats(st["mask"])
            fragile, count_fragile, min_margin = set(), False, float("inf")
            if "comp" in seen:
                comp, dsc = seen["comp"], seen["score"]
                n_prev = comp.shape[1] - 1
                top2v, top2i = comp.topk(2, dim=1)
                cm = top2v[:, 0] - top2v[:, 1]
                mid = top2i[:, 0]
                new_rank = torch.cumsum((mid == 0).long(), 0) - 1                      # appended row of a new object = n_prev + rank
                for i in range(comp.shape[0]):
                    if cm[i] < FRAGILE_EPS:
                        for j in top2i[i].tolist():
                            if j == 0:
                                count_fragile = True
                            else:
                                fragile.add(j - 1)
                        if mid[i] == 0:
                            fragile.add(n_prev + int(new_rank[i]))
                for obj in range(n_prev):
                    c = torch.nonzero(mid == obj + 1).view(-1)
                    if len(c) > 1:
                        sc = dsc[c].sort(descending=True).values
                        if sc[0] - sc[1] < FRAGILE_EPS:
                            fragile.add(obj)
                        min_margin = min(min_margin, float(sc[0] - sc[1]))
                min_margin = min(min_margin, float(cm.min()))
            out[f"t{t}_fragile_rows"] = np.array(sorted(fragile), dtype=np.int64)
            out[f"t{t}_count_fragile"] = np.array(count_fragile)
            out[f"t{t}_min_margin"] = np.array(min_margin)
            any_count_fragile |= count_fragile
            # the keep rule's three conditions on the state (track_TF.py:160-164), and which rows fail exactly one of them
            only = {1: [], 2: [], 3: []}
            score_margin = float("inf")
            if n_st:
                tm = st["tracked_mask"]
                c1 = tm <= 10
                cnt = (st["mask"] > 0.5).sum([1, 2])
                c2 = cnt > 1
                c3 = st["score"] > cfg.eval_conf_thresh
                for i, (a, b, c) in enumerate(zip(c1.tolist(), c2.tolist(), c3.tolist())):
                    if [a, b, c].count(False) == 1:
                        only[[a, b, c].index(False) + 1].append(i)
                d3 = (st["score"] - cfg.eval_conf_thresh).abs()
                score_margin = float(d3.min())
                fragile |= set(torch.nonzero(d3 < SCORE_EPS).view(-1).tolist())
                lo = (st["mask"] > 0.5 + FRAGILE_EPS).sum([1, 2])
                hi = (st["mask"] > 0.5 - FRAGILE_EPS).sum([1, 2])
                fragile |= set(torch.nonzero((lo > 1) != (hi > 1)).view(-1).tolist())
                rem = [int(v) for v in torch.nonzero((tm == 0) & (torch.tensor(prev_tm + [0] * (n_st - len(prev_tm))) >= 5)).view(-1)] if t else []
            else:
                rem = []
            excused |= fragile
            for c in (1, 2, 3):
                extra[f"t{t}_only_cond{c}"] = np.array(only[c], dtype=np.int64)
            extra[f"t{t}_excused_rows"] = np.array(sorted(excused), dtype=np.int64)
            extra[f"t{t}_rematched"] = np.array(rem, dtype=np.int64)
            extra[f"t{t}_score_margin"] = np.array(score_margin)
            prev_tm = [int(v) for v in st["tracked_mask"].tolist()] if n_st else []
            print(f"{name} frame {t:2d} {br:11s} cand {seen['n_cand']:3d} state {n_st:3d} reported {n_rep:3d} age>10 {int((~c1).sum()) if n_st else 0:3d} "
                  f"rematched(>=5) {len(rem):2d} score<=thr {int((~c3).sum()) if n_st else 0:3d} pix<=1 {int((~c2).sum()) if n_st else 0:3d} "
                  f"only c1/c2/c3 {len(only[1])}/{len(only[2])}/{len(only[3])} excused {len(excused)} margins match {min_margin:.1e} score {score_margin:.1e}")
    ttf.compute_comp_scores, ttf.CandidateShift = real_ccs, real_shift
    tracker.track, net.forward_single = real_track, real_fs
    if any_count_fragile:
        raise SystemExit(f"{name}: a frame's row COUNT hangs on a comparison closer than {FRAGILE_EPS}: pick another clip seed for this fixture")
    extra["branches"] = np.array(branches)
    out.update(extra)
    if coeff_sums:
        for k in [k for k in out if re.fullmatch(r"t\d+_(state_)?mask_coeff", k)]:
            v = torch.as_tensor(out.pop(k)).double()
            out[k + "_sums"] = torch.stack([v.sum(1), v.abs().sum(1)], 1)
        for k in [k for k in out if re.fullmatch(r"t\d+_centerness", k)]:
            del out[k]
    save(name, **out)
    return branches


# Frames of the gaps fixture (-1: all zeros, no detections): nothing detected on the first frame (track_TF.py:56-58), the first detections on a
# non-first frame (:88-93 with prev_candidate None), two frames without detections (:61-66, CandidateShift alone), then re-matching after the gap.
GAPS_FRAMES = (-1, 1, 2, 3, 4, 5, -1, -1, 8, 9, 10, 11)
GAPS_BRANCHES = {0: "empty_first", 1: "first_late", 2: "match", 6: "empty_shift", 7: "empty_shift", 8: "match", 11: "match"}


from synth_results import synth_video_results  # noqa: E402  (tests/golden/synth_results.py, shared with the test)


def gen_results_json():
    """Row f2: the reference's own bbox2result_with_id + results2json_videoseg (layers/eval_utils.py) on seeded inputs."""
    import json
    sys.modules["mmcv"].dump = lambda obj, path: json.dump(obj, open(path, "w"))
    from layers import eval_utils
    classes = ["c%d" % i for i in range(40)]
    frames = synth_video_results()
    results = [eval_utils.bbox2result_with_id(det, meta, classes) for det, meta in frames]
    per_frame = [{str(k): (v if k in ("video_id", "frame_id") else
                           {"bbox": v["bbox"].tolist(), "label": int(v["label"]), "score": float(v["score"]),
                            "category": v["category"]}) for k, v in r.items()} for r in results]
    out = os.path.join(HERE, "_tmp_results_dir", "results.json")   # the reference makedirs(out_file[:-13])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    eval_utils.results2json_videoseg(results, out)
    records = json.load(open(out))
    os.remove(out)
    os.rmdir(os.path.dirname(out))
    with open(os.path.join(HERE, "results_json.json"), "w") as f:
        json.dump({"per_frame": per_frame, "records": records}, f)
    print("wrote results_json.json:", len(records), "records")


def main():
    install_stubs()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["postproc", "priors", "fcb_ali", "model"]
    if "postproc" in which:
        gen_postproc()
    if "postproc_nontf" in which:
        gen_postproc_nontf()
    if "priors" in which:
        gen_priors()
    if "fcb_ali" in which:
        gen_fcb_ali()
    if "model" in which:
        gen_model("STMask_plus_resnet50_config", "r50_fca")
        gen_model("STMask_plus_resnet50_ada_config", "r50_ada")
        gen_model("STMask_plus_resnet50_ali_config", "r50_ali")
    if "results_json" in which:
        gen_results_json()
    if "model_nontf" in which:
        gen_model_nontf("STMask_plus_resnet50_config", "r50_fca_nontf")
    if "model_full" in which:
        gen_model_full("STMask_plus_resnet50_config", "r50_fca")
        gen_model_full("STMask_plus_resnet50_ada_config", "r50_ada")
        gen_model_full("STMask_plus_base_ali_config", "r101_ali")
    if "model_full_tf" in which:
        gen_model_full_tf("STMask_plus_resnet50_config", "model_full_tf_r50_fca.npz")
        gen_model_full_tf("STMask_plus_resnet50_ada_config", "model_full_tf_r50_ada.npz")
    if "model_full_tf_r101" in which:
        gen_model_full_tf("STMask_plus_base_ali_config", "model_full_tf_r101_ali.npz")
    if "model_full_tf16" in which:
        # the benchmark's clip length (bench.py --frames 16)
        for cfg_name, tag in (("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada")):
            gen_model_full_tf(cfg_name, f"model_full_tf16_{tag}.npz", frame_src=16, n_masks=16, mask_frames=(0, 11, 15),
                              coeff_sums=True)
    if "model_full_tf_gaps" in which:
        gen_model_full_tf("STMask_plus_resnet50_config", "model_full_tf_gaps_r50_fca.npz", frame_src=GAPS_FRAMES, n_masks=16, mask_frames=(1, 7, 11),
                          expect=GAPS_BRANCHES, coeff_sums=True)
    if "model_full_720p" in which:
        gen_model_full("STMask_plus_base_ali_config", "r101_ali_736x1280", hw=(736, 1280), row_step=64)
    if "model_extra" in which:
        gen_model("STMask_plus_base_ali_config", "r101_ali", hw=(96, 160), n_frames=2)


if __name__ == "__main__":
    main()
