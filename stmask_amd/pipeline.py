"""Batched clip pipeline: many independent video clips advance one frame per step on one GPU.

forward_single has no cross-frame dependence, so frame t of all local clips goes through the trunk
and heads as ONE batch; the temporal-fusion / tracker stage is per clip in the reference (previous-frame features and
tracker state, track_TF.py:52-54,96-100).  Two drivers:

* ``ClipPipeline``        -- reference-shaped: one ``Track_TF`` per clip, the layer API of ``stmask_amd.layers``
                             (what a user of the reference's eval loop gets; ~4 host syncs per clip and frame).
* ``BatchedClipPipeline`` -- same arithmetic, but the state of all clips lives in concatenated tensors and every stage
                             is ONE launch for all clips: fused decode + threshold + Fast NMS (no sync), one lincomb
                             launch for all detections (per-row prototype index), one correlation / RoIAlign /
                             TemporalNet / decode / lincomb chain for all tracked instances, one cross matrix for the
                             matching scores.  Two small device->host reads per STEP (detection counts, match ids).

This file holds the step and the tracker state with its transitions (per-clip drop, snapshot, range fallback).  Where the trunk of a
frame comes from -- eager or a graph ring, prefetched on side streams -- is ``trunk.TrunkRunner``, the base class; what the tracker
decides on the host between the two reads is ``track_host`` (pure functions on lists).
"""
import os
import sys
import time

import torch
import torch.nn.functional as F

from . import fuse, ops, track_host
from .dist import DET_COLS
from .layers import Track_TF, generate_candidate
from .trunk import TrunkRunner, concurrent_side_streams, trunk_stream_count  # noqa: F401  (dist.py and the tests import the two functions from here)

ROI_CHUNKS = (256, 128, 64)  # TemporalNet only ever sees these RoI batch sizes: three dense-conv shapes in total


class _StageTimer:
    """Optional per-stage wall-clock breakdown (STM_PIPE_TIMING=1): synchronises around every stage, so only for
    diagnosis -- never enabled in a timed benchmark run."""

    def __init__(self):
        self.on = os.environ.get("STM_PIPE_TIMING", "0") == "1"
        self.acc, self.t0 = {}, None

    def tic(self):
        if self.on:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()

    def toc(self, name):
        if self.on and self.t0 is not None:          # (a step that has not called tic -- the non-TF one -- has no stages)
            torch.cuda.synchronize()
            t = time.perf_counter()
            self.acc[name] = self.acc.get(name, 0.0) + (t - self.t0)
            self.t0 = t


class ClipPipeline:
    def __init__(self, net, n_clips):
        self.net = net
        self.cfg = net.cfg
        if not self.cfg.temporal_fusion_module:
            raise NotImplementedError("ClipPipeline drives the temporal-fusion configs (all STMask_plus_* configs)")
        self.trackers = [Track_TF(cfg=self.cfg) for _ in range(n_clips)]
        self.t = 0

    @torch.no_grad()
    def step(self, frames, is_first=None):
        """frames [n_clips,3,H,W] = the next frame of every clip -> list of per-clip detection dicts."""
        net, cfg = self.net, self.cfg
        first = (self.t == 0) if is_first is None else is_first
        fpn_outs, pred = net.forward_single(frames)
        pred["conf"] = F.softmax(pred["conf"], -1)
        pred["fpn_feat"] = fpn_outs[net.correlation_selected_layer]
        pred["T2S_feat"] = pred["T2S_feat"][net.correlation_selected_layer]
        candidates = generate_candidate(pred, cfg=cfg)
        out = []
        for i, cand in enumerate(candidates):
            det = net.Detect_TF.detect(cand, is_output_candidate=True)
            meta = {"is_first": first, "video_id": i, "frame_id": self.t}
            out.append(self.trackers[i].track(net, det, meta, img=None))
        self.t += 1
        return out


_ROW_KEYS = ("box", "mask_coeff", "track", "class", "score", "centerness", "mask")


class _TrackedRows(dict):
    """The tracked set's row tensors.  After a tracker update the soft masks of the merged set are not gathered (61 KB per row,
    rewritten from the prototypes at the next step anyway; the keep rule reads their bit words): `rows["mask"]` gathers them on
    first use from the two sources and the gather plan of that update."""

    _deferred = None            # (prev_mask, det_mask, plan, n_prev, host plan) of a mask not gathered yet

    def defer_mask(self, prev_mask, det_mask, plan, n_prev, plan_host=None):
        self._deferred = (prev_mask, det_mask, plan, n_prev, plan_host)
        dict.pop(self, "mask", None)

    def deferred_mask(self):
        """(prev_mask, det_mask, plan, n_prev, host plan) of a mask not gathered yet, else None."""
        return None if dict.__contains__(self, "mask") else self._deferred

    def _materialize(self):
        if not dict.__contains__(self, "mask") and self._deferred is not None:
            a, b, plan, n_prev, _ = self._deferred
            dict.__setitem__(self, "mask", ops.gather_rows2([a], [b], plan, n_prev)[0])
            self._deferred = None

    def __getitem__(self, key):
        if key == "mask":
            self._materialize()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        self._materialize()
        return dict.keys(self)

    def values(self):
        self._materialize()
        return dict.values(self)

    def items(self):
        self._materialize()
        return dict.items(self)

    def __iter__(self):
        self._materialize()
        return dict.__iter__(self)

    def __setitem__(self, key, value):
        if key == "mask":
            self._deferred = None
        dict.__setitem__(self, key, value)

    def __contains__(self, key):
        return dict.__contains__(self, key) or (key == "mask" and self._deferred is not None)


class BatchedClipPipeline(TrunkRunner):
    """All clips' tracker state concatenated (rows sorted by clip); per-clip row ranges are host integers.  device_tracker=True (temporal
    fusion only): the tracker's counters and decisions stay on the device, the row counts reach the host one step late (_settle)."""

    def __init__(self, net, n_clips, device_tracker=False):
        # temporal-fusion configs (self.tf): Detect_TF + Track_TF (CandidateShift, soft masks, the keep rule) -- _step_tf; without the module the
        # reference runs Detect + Track (detection.py:98-137, track.py:56-179: binary masks, the (mask_ious > 0.3).sum() < 2 update gate, the
        # frame's own detections as output) -- _step_nontf
        super().__init__(net, n_clips, _StageTimer())
        self.range_fallback = True  # an fp16 plane graph that leaves its range is replaced by the bf16x3 graph and the step repeated (see step)
        self.fell_back = False
        self._last = None           # non-TF: the last step's detections (rows, ids, clip ranges) for detections()
        self.t = 0
        # device_tracker: the tracker's per-row state lives on the device alone (_tm_dev, _off_dev) and its decisions are kernels
        # (ops.track_resolve_tf, ops.track_drop_plan): no per-row host structure is built in a step.  The new row counts come back one step
        # late (_settle); until then the row tensors stand at their capacity, rows + detections.  Opt-in; temporal-fusion nets only.
        self.device_tracker = bool(device_tracker)
        if self.device_tracker and not self.tf:
            raise ValueError("BatchedClipPipeline: device_tracker needs a temporal-fusion net (the tracker without the module decides on the host)")
        self._unsettled = None      # device_tracker: (pinned new offsets [B + 1], event) of a step whose row counts the host has not read yet
        self._off_pin = [None, None]
        self._n_resolved = 0
        self._cnt_dev = None        # device_tracker: this step's detection counts as they stand on the device (after the clamp and the idle mask)
        self._drop_pin = []         # device_tracker: ring of (pinned int32 [B], event of the copy that last read it) for the per-clip drop flags
        self._n_drops = 0
        self.prev = None            # dict of concatenated row tensors
        self.prev_n = [0] * n_clips  # tracked instances per clip
        self.prev_feat = None       # (P4 [B,256,h,w], T2S [B,256,h,w]) of the previous frame
        self.tracked = [[] for _ in range(n_clips)]  # host-side "frames since last match" counters
        self._bits = None           # > 0.5 bit words of the tracked set's masks, as of the last tracker update (the keep rule counts pixels on them)
        self._prev_bits = None      # TF: ... of the tracked set shifted onto this step's prototypes (_shift_prev), for the mask IoU
        self._off_dev = None        # device int32 [B + 1]: first row of every clip in the tracked set (_upload_meta, _drop_clips)
        self._tm_dev = None         # device int32: self.tracked, concatenated (_upload_meta)
        self._idle_masks = {}        # inactive-slot pattern -> device bool [B] (see step's `active`)
        self._idle_dev = None
        # Workload knob of the benchmark ("a max_instances cap to study n ~ 5-10, the realistic regime"), NOT
        # a reference semantic: the reference's tracker never prunes (track_TF.py:132-165).  n > 0: at most n detections per frame
        # (the best-scoring ones: Fast NMS returns them sorted) and at most n tracked instances per clip (an unmatched detection
        # opens a new track only while the clip holds fewer).  0 = the reference's behaviour.
        self.max_instances = 0

    # -- the state a reader outside a step sees: settled first (a no-op without device_tracker) ----------------------------
    @property
    def prev(self):
        self._settle()
        return self._prev

    @prev.setter
    def prev(self, v):
        self._prev = v

    @property
    def prev_n(self):
        self._settle()
        return self._prev_n

    @prev_n.setter
    def prev_n(self, v):
        self._prev_n = v

    @property
    def tracked(self):
        """Per clip the frames-since-last-match counters of its rows (host lists; with device_tracker a read-back of _tm_dev)."""
        if not self.device_tracker:
            return self._tracked
        self._settle()
        if self._prev is None or self._tm_dev is None or sum(self._prev_n) == 0:
            return [[] for _ in range(self.B)]
        tm, off = self._tm_dev.tolist(), track_host.clip_offsets(self._prev_n)
        return [tm[off[b]:off[b + 1]] for b in range(self.B)]

    @tracked.setter
    def tracked(self, v):
        self._tracked = v

    def _settle(self):
        """device_tracker: take in the row counts of the last tracker update -- wait for the copy of its new offsets, set prev_n, and narrow
        every row tensor, the bit words, the counters and a deferred mask plan to the real rows (views: nothing is copied).  Runs at the start
        of the next step and whenever prev / prev_n / tracked are read."""
        pend = self._unsettled
        if pend is None:
            return
        self._unsettled = None
        buf, ev = pend
        ev.synchronize()
        off = buf.tolist()
        self._prev_n = [off[b + 1] - off[b] for b in range(self.B)]
        R, prev = off[-1], self._prev
        if prev is None:                                    # (the set was taken away from outside in the meantime)
            return
        for k in list(dict.keys(prev)):
            dict.__setitem__(prev, k, dict.__getitem__(prev, k)[:R])
        if prev._deferred is not None:
            a, b_, plan, n_prev, host_plan = prev._deferred
            prev._deferred = (a, b_, plan[:R], n_prev, host_plan)
        self._bits, self._tm_dev = self._bits[:R], self._tm_dev[:R]

    # -- stage helpers ------------------------------------------------------------------------------------------------
    def _roi_feats(self, P4_prev, P4, T2S_prev, T2S, rois):
        P = self.cfg.correlation_patch_size
        corr = ops.corr_patch(P4_prev, P4, P, 1, scale=1.0 / P4.shape[1], leaky_slope=0.1)
        corr = corr.view(P4.shape[0], P * P, P4.shape[2], P4.shape[3])
        feats = F.relu(torch.cat([corr, T2S_prev, T2S], dim=1))
        roi_feats = ops.roi_align(feats, rois, 7)
        self.timer.toc("tf_corr_roi")
        return roi_feats

    def _shift_prev(self, P4, T2S, proto, dev):
        """CandidateShift (TF_utils.py:12-51) for every tracked instance of every clip in one chain."""
        net, cfg, prev = self.net, self.cfg, self.prev
        clip_of_row = prev["clip"]
        P4_prev, T2S_prev = self.prev_feat
        P = cfg.correlation_patch_size
        fh, fw = P4.shape[2:]
        rois = ops.shift_rois(prev["box"], clip_of_row, fh, fw)      # (clip, sanitised box in feature-map pixels)
        ptn = getattr(net, "_planar_temporal", None)
        a_prev, a_cur = T2S_prev.permute(0, 2, 3, 1), T2S.permute(0, 2, 3, 1)
        if (ptn is not None and ptn.ncorr == P * P and a_prev.is_contiguous() and a_cur.is_contiguous()
                and 2 * T2S.shape[1] + P * P == ptn.cin):
            # fused planes: ReLU + concatenation + RoIAlign + channel padding + split in one kernel: the RoI features leave as the planes
            # TemporalNet's first convolution reads (the feature maps are channels_last views of the head's fp32 output; the
            # correlation volume is written channels-last too, so a sample's 121 displacements are 4 cache lines, not 121)
            # (P4 is a channels_last view of the FPN's fp32 output: the correlation kernel reads it in place)
            corr = ops.corr_patch_nhwc(P4_prev, P4, P, scale=1.0 / P4.shape[1], leaky_slope=0.1)
            xp = ops.roi_align_planes(a_prev, a_cur, corr, rois, 7, fmt=ptn.fmt, corr_nhwc=P * P)
            self.timer.toc("tf_corr_roi")
            loc_shift, coeff_shift = ptn.forward_planes(xp, rois.shape[0])
        elif ptn is not None:      # planar convolution: any RoI count, one launch per layer
            loc_shift, coeff_shift = ptn(self._roi_feats(P4_prev, P4, T2S_prev, T2S, rois))
        else:
            roi_feats = self._roi_feats(P4_prev, P4, T2S_prev, T2S, rois)
            n = roi_feats.shape[0]
            n_pad = -(-n // ROI_CHUNKS[-1]) * ROI_CHUNKS[-1]
            if n_pad != n:  # rows are independent: zero rows change nothing
                roi_feats = torch.cat([roi_feats, roi_feats.new_zeros(n_pad - n, *roi_feats.shape[1:])], 0)
            # fixed-shape blocks (greedy 256 / 128 / 64): the dense-conv library (MIOpen) selects / builds kernels per
            # shape and the tracked set changes size every frame -- three shapes mean that cost is paid three times
            outs, i = [], 0
            while i < n_pad:
                c = next(c for c in ROI_CHUNKS if c <= n_pad - i)
                outs.append(net.TemporalNet(roi_feats[i:i + c]))
                i += c
            loc_shift = torch.cat([o[0] for o in outs], 0)[:n]
            coeff_shift = torch.cat([o[1] for o in outs], 0)[:n]
        self.timer.toc("tf_temporalnet")
        # decode(loc_shift, center_size(box)) / coeff += shift / score *= 0.95 in one launch, in place on the tracked rows
        ops.shift_apply_(loc_shift, coeff_shift, prev["box"], prev["mask_coeff"], prev["score"], 0.95)
        # masks of the shifted instances on the CURRENT prototypes, and their > 0.5 bits for this step's mask IoU (one pass)
        prev["mask"], self._prev_bits = ops.lincomb_sigmoid_crop_bits(proto, prev["mask_coeff"], prev["box"], clip_of_row)
        self.timer.toc("tf_masks")
        if self.device_tracker:
            self._tm_dev = self._tm_dev + 1                 # a new tensor: a snapshot of the old one stays valid
            return
        for b in range(self.B):
            self.tracked[b] = [v + 1 for v in self.tracked[b]]

    def _detect(self, pred):
        """Decode + confidence threshold + Fast NMS for every frame of the batch, no host sync -> (prior_idx [B, cap], cls, score, box, count [B]).
        Cross-class Fast NMS (the default, detection_TF.py:85-134: cap = nms_top_k) or -- Detect_TF.use_cross_class_nms = False, the reference's
        per-class variant (detection_TF.py:136-204, README "mAP*" column: cap = max_num_detections) -- one launch pair for all frames."""
        cfg, net = self.cfg, self.net
        priors = pred["priors"].squeeze(0)
        det = net.Detect_TF if self.tf else net.detect
        if getattr(det, "use_cross_class_nms", True):
            # (the softmax of STMask.py:314 is taken per row inside the candidate pass: no pass over the [B, N, 41] logits of its own)
            return ops.detect_cc(pred["loc"], priors, pred["conf"], pred["centerness"], cfg.eval_conf_thresh, cfg.nms_thresh, cfg.nms_top_k, logits=True)
        # (per-class ranking: conf * centerness in Detect_TF.fast_nms, detection_TF.py:139-141; the raw confidences in the non-TF Detect.fast_nms,
        # detection.py:211-212)
        return ops.detect_pc(pred["loc"], priors, F.softmax(pred["conf"], -1), pred["centerness"] if self.tf else None, cfg.eval_conf_thresh, cfg.nms_thresh,
                             cfg.nms_top_k, cfg.max_num_detections)

    @torch.no_grad()
    def step(self, frames, is_first=None, next_frames=None, active=None):
        """frames [B,3,H,W] -> packed detections [B, top_k, 40] (stmask_amd.dist layout) without a final sync, plus the
        per-clip tracked-instance counts (host ints).  next_frames (optional): the frames the NEXT call will be given -- or a list: those of the
        next call, of the one after it, ... (the same tensor OBJECTS the later calls pass as `frames`); their trunks are started on side streams
        while this step's tracker logic runs (_prefetch_trunk).

        is_first: None (True on the first step), a bool for every clip, or B bools (a list / tuple / CPU bool tensor [B]): clip b starts a new
        video on this frame -- its tracked rows are dropped before anything reads them and the reference's first-frame rule applies to it alone
        (track_TF.py:86-93, track.py:92-97), while the other clips keep their state.  active: None (all) or B bools; an inactive slot reports
        nothing (its detection count is 0 on the device, its tracked rows are dropped, its packed rows are zero) -- a serving loop with fewer
        videos than slots (stmask_amd.serve) gives it a frame of zeros.

        fp16 plane graphs carry |activation| <= 65504 only; their producers raise a sticky device flag beyond that, which arrives with the step's
        first host read (ops.RangeError).  The step is then NOT lost: the tracker state it had touched is put back, the inference graph is rebuilt
        with bf16x3 planes (fp32's range; weights repacked from the same modules, in-process), the step is repeated on it and the pipeline stays
        there (`fell_back`; logged once on stderr).  range_fallback = False restores the raise."""
        self._settle()
        first, resets = self._first_flags(is_first)
        idle = self._idle_flags(active, frames.device)
        if first:
            self.prev, self.prev_n, self.prev_feat = None, [0] * self.B, None
            self.tracked = [[] for _ in range(self.B)]
        drop = sorted(set(resets) | set(idle))
        snap = self._snapshot() if (self.range_fallback and self._range_guarded()) else None
        self._drop_clips(drop, frames.device)
        try:
            return self._step(frames, first, next_frames)
        except ops.RangeError:
            if snap is None:
                raise
            self._fall_back(snap)
            self._drop_clips(drop, frames.device)
            return self._step(frames, first, next_frames)

    def _clip_flags(self, v, what):
        if torch.is_tensor(v):
            if v.device.type != "cpu" or v.dtype != torch.bool or tuple(v.shape) != (self.B,):
                raise ValueError(f"BatchedClipPipeline.step: {what} must be a CPU bool tensor of shape [{self.B}], got {v.dtype} {tuple(v.shape)} on {v.device}")
            v = v.tolist()
        v = [bool(x) for x in v]
        if len(v) != self.B:
            raise ValueError(f"BatchedClipPipeline.step: {what} has {len(v)} entries for {self.B} clips")
        return v

    def _first_flags(self, is_first):
        """-> (reset every clip, [clips that reset alone]).  An all-True / all-False sequence is the scalar form."""
        if is_first is None:
            return self.t == 0, []
        if (torch.is_tensor(is_first) and is_first.dim() == 0) or not hasattr(is_first, "__len__"):
            return bool(is_first), []
        f = self._clip_flags(is_first, "is_first")
        if all(f) or not any(f):
            return f[0], []
        return False, [b for b in range(self.B) if f[b]]

    def _idle_flags(self, active, dev):
        """-> [inactive clips]; sets self._idle_dev (device bool [B], or None when every clip is active) for the detection-count mask."""
        self._idle_dev = None
        if active is None:
            return []
        a = self._clip_flags(active, "active")
        if all(a):
            return []
        key = (dev, tuple(a))
        if key not in self._idle_masks:
            self._idle_masks[key] = torch.tensor([not x for x in a], dtype=torch.bool).to(dev)
        self._idle_dev = self._idle_masks[key]
        return [b for b in range(self.B) if not a[b]]

    def _drop_clips(self, clips, dev):
        """Per-clip reset: the tracked rows of `clips` leave the concatenated set before CandidateShift reads it -- every row tensor and the
        masks' bit words in ONE gather_rows2 launch (<= 8 tensors), a deferred soft-mask gather (_TrackedRows) stays deferred with its plan
        composed on the host; the clip row offsets and the plan(s) go to the device in one copy.  New tensors: the set before the drop stays
        intact for _fall_back.  The clips then hold nothing, and the pn == 0 branches of the tracker apply the first-frame rule to them."""
        if not clips:
            return
        if self.device_tracker:
            return self._drop_clips_dev(clips, dev)
        prev_n = list(self.prev_n)
        for b in clips:
            self.tracked[b] = []
            self.prev_n[b] = 0
        if self.prev is None or not any(prev_n[b] for b in clips):
            return
        keep, n_rows = track_host.keep_rows(prev_n, set(clips)), sum(prev_n)
        if not keep:
            self.prev, self._bits, self._prev_bits = None, None, None
            return
        prev = self.prev
        deferred = prev.deferred_mask() if isinstance(prev, _TrackedRows) else None
        mask_plan = [deferred[4][r] for r in keep] if deferred is not None and deferred[4] is not None else None
        if deferred is not None and mask_plan is None:
            prev["mask"]                                  # (a deferral without a host plan: gather it now)
            deferred = None
        off = track_host.clip_offsets(self.prev_n)
        meta = torch.tensor(off + keep + (mask_plan or []), dtype=torch.int32).to(dev, non_blocking=True)
        nb, nk = len(off), len(keep)
        self._off_dev, keep_dev = meta[:nb], meta[nb:nb + nk]
        keys = [k for k in dict.keys(prev) if k != "mask"]
        srcs = [dict.__getitem__(prev, k) for k in keys] + [self._bits]
        rows = ops.gather_rows2(srcs, [t[:0] for t in srcs], keep_dev, n_rows)
        kept = _TrackedRows() if self.tf else {}
        for k, t in zip(keys, rows[:-1]):
            kept[k] = t
        if self.tf:
            if deferred is not None:
                a, b_, _, n_prev, _ = deferred
                kept.defer_mask(a, b_, meta[nb + nk:], n_prev, mask_plan)
            elif dict.__contains__(prev, "mask"):
                m = dict.__getitem__(prev, "mask")
                kept.defer_mask(m, m[:0], keep_dev, n_rows, keep)
        self.prev, self._bits, self._prev_bits = kept, rows[-1], None

    def _drop_clips_dev(self, clips, dev):
        """_drop_clips with device_tracker: the keep plan is ops.track_drop_plan's (the host sizes it from the clips' row counts and uploads
        one flag per clip, cached per pattern), the counters are gathered with the rows, and a deferred soft-mask gather stays deferred with
        its plan composed on the device."""
        prev_n = list(self._prev_n)
        for b in clips:
            self._prev_n[b] = 0
        if self._prev is None or not any(prev_n[b] for b in clips):
            return
        n_rows, n_keep = sum(prev_n), sum(self._prev_n)
        if not n_keep:
            self._prev, self._bits, self._prev_bits, self._tm_dev, self._off_dev = None, None, None, None, None
            return
        keep_dev, self._off_dev = ops.track_drop_plan(self._off_dev, self._drop_flags(clips, dev), n_keep)
        prev = self._prev
        deferred = prev.deferred_mask() if isinstance(prev, _TrackedRows) else None
        keys = [k for k in dict.keys(prev) if k != "mask"]
        srcs = [dict.__getitem__(prev, k) for k in keys] + [self._bits, self._tm_dev]
        rows = ops.gather_rows2(srcs, [t[:0] for t in srcs], keep_dev, n_rows)
        kept = _TrackedRows()
        for k, t in zip(keys, rows[:-2]):
            kept[k] = t
        if deferred is not None:
            a, b_, plan, n_prev, _ = deferred
            kept.defer_mask(a, b_, plan.index_select(0, keep_dev.long()), n_prev)
        elif dict.__contains__(prev, "mask"):
            m = dict.__getitem__(prev, "mask")
            kept.defer_mask(m, m[:0], keep_dev, n_rows)
        self._prev, self._bits, self._tm_dev, self._prev_bits = kept, rows[-2], rows[-1], None

    def _drop_flags(self, clips, dev):
        """Device int32 [B], 1 where the clip drops its rows: B ints through one of four pinned buffers, copied without a wait (a buffer is
        written again only after the copy that read it has finished: an event four drops old).  Nothing is cached per pattern -- a server's
        slots reset in ever new combinations."""
        slot = self._n_drops % 4
        self._n_drops += 1
        if len(self._drop_pin) <= slot:
            self._drop_pin.append([torch.empty(self.B, dtype=torch.int32).pin_memory(), None])
        buf, ev = self._drop_pin[slot]
        if ev is not None:
            ev.synchronize()
        gone = set(clips)
        buf.copy_(torch.tensor([int(b in gone) for b in range(self.B)], dtype=torch.int32))
        flags = buf.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._drop_pin[slot][1] = ev
        return flags

    def _range_guarded(self):
        g = getattr(self.net, "_planar", None)
        return g is not None and getattr(self.net, "_planar_planes", "bf16x3") != "bf16x3"

    def _snapshot(self):
        """What a step mutates IN PLACE before its first host read (CandidateShift's decode / coefficient shift / score decay on the tracked rows)
        plus the host-side counters: enough to repeat the step."""
        prev = self.prev
        rows = None
        if self.tf and prev is not None and sum(self.prev_n):
            rows = tuple(prev[k].clone() for k in ("box", "mask_coeff", "score"))
        # (a per-clip reset replaces the tracked set by new tensors before the step: the set, its counts, bit words and offsets are kept as they were)
        state = (prev, list(self.prev_n), self._bits, self._prev_bits, self._off_dev)
        if self.device_tracker:
            return rows, self._tm_dev, self.t, state        # (the counters are a device tensor no step writes in place)
        return rows, [list(t) for t in self.tracked], self.t, state

    def _fall_back(self, snap):
        net = self.net
        self._pending = []
        torch.cuda.synchronize()                      # nothing enqueued on the fp16 graph may raise the flag after it has been cleared
        flag = ops._range_flags.get(torch.cuda.current_device())
        if flag is not None:
            flag.zero_()
        sys.stderr.write(f"stmask_amd: step {self.t}: an activation left the range of the {getattr(net, '_planar_planes', 'fp16')} planar format (|x| > 65504); "
                         "rebuilding the inference graph with bf16x3 planes, repeating the step and staying there (half the convolution rate)\n")
        if getattr(net, "_planar_bf16x3", None) is None:
            net._planar_bf16x3 = fuse.build_planar(net, "bf16x3")
        fuse.attach_planar(net, net._planar_bf16x3)
        self._reset_graphs()
        rows, tracked, t, state = snap
        self.prev, self.prev_n, self._bits, self._prev_bits, self._off_dev = state[0], list(state[1]), state[2], state[3], state[4]
        if rows is not None:
            for k, v in zip(("box", "mask_coeff", "score"), rows):
                self.prev[k].copy_(v)
        if self.device_tracker:
            self._tm_dev, self.t = tracked, t
        else:
            self.tracked, self.t = tracked, t
        self.fell_back = True

    def _step(self, frames, first, next_frames):
        if self.tf:
            return self._step_tf(frames, next_frames)
        return self._step_nontf(frames, first, next_frames)

    def _detections(self, pred, mask_coeff, max_instances=0):
        """The front both steps share once they hold the trunk's outputs: detect -> (max_instances clamp) -> idle mask -> host read 1 -> the
        detections of all clips, concatenated (rows sorted by clip), in one gather kernel.  -> (det rows, counts per clip, the rows' NMS
        scores as host floats).  mask_coeff: the coefficients the rows carry (raw, or tanh'ed on the non-TF path)."""
        idx, cls, score, box, cnt = self._detect(pred)
        if max_instances > 0:
            cnt = torch.clamp(cnt, max=max_instances)
        if self._idle_dev is not None:
            cnt = cnt.masked_fill(self._idle_dev, 0)                   # inactive slots detect nothing
        if self.device_tracker:
            counts, host_scores = ops.counts_to_host(cnt), None       # host read 1 without the scores: the resolution reads det["score"] on the device
            self._cnt_dev = cnt
        else:
            counts, host_scores = ops.counts_to_host(cnt, extra=score)  # host read 1: B counts + the fp16 range flag + the NMS scores
        self.timer.toc("detect")
        top_k = idx.shape[1]                              # slots per frame of the detector's outputs (nms_top_k, or max_num_detections per class-wise NMS)
        det = ops.gather_detections(idx, cls, score, box, cnt, mask_coeff, pred["track"], pred["centerness"], sum(counts))
        if host_scores is None:
            return det, counts, None
        det_scores = [float(host_scores[b * top_k + j]) for b in range(self.B) for j in range(counts[b])]   # row order of det
        return det, counts, det_scores

    def _match_scores(self, det, det_bits, prev_bits, n_pixels):
        """Matching scores of the detections against the tracked set for all clips at once -> (match ids [D]: 0 or 1 + the tracked row, mask IoU
        [D, Pn]); pairs from different clips can never match.  Needs this step's clip offsets on the device (_off_dev)."""
        prev = self.prev
        miou = ops.mask_iou_bits(det_bits, prev_bits, n_pixels, group1=det["clip"], group2=prev["clip"])   # same-clip pairs only
        # (the embedding dot products of the same-clip pairs are taken inside the kernel)
        match = ops.match_scores_embed(det["track"], prev["track"], miou, det["box"], prev["box"], det["score"], det["class"], prev["class"],
                                       det["clip"], self._off_dev, self.cfg.match_coeff, 0.3)
        return match, miou

    def _step_tf(self, frames, next_frames):
        net = self.net
        dev = frames.device
        tmr = self.timer
        tmr.tic()
        if getattr(net, "_planar", None) is not None and tmr.on:
            net._planar.timer = tmr      # finer stages inside the trunk
        fpn_outs, pred, dropped = self._take_trunk(frames)
        tmr.toc("trunk")
        # A dropped prefetch under graph replay leaves the round-robin one slot ahead: the slot the NEXT replay overwrites is then
        # the one holding the previous frame's P4 / T2S, which CandidateShift below still reads -- so in that step the next trunk
        # must not start before _shift_prev is enqueued (the late position), whatever prefetch_early says.
        if self.prefetch_early and not (dropped and self.graph_active):
            # start the next trunk right away: it then also shares the GPU with this step's temporal-fusion convolutions
            # (more throughput, but kernels of the two streams stretch each other: per-kernel timings stop being clean)
            self._prefetch_trunk(next_frames)
            next_frames = None
        P4 = fpn_outs[net.correlation_selected_layer]
        T2S = pred["T2S_feat"][net.correlation_selected_layer]
        proto = pred["proto"]
        # CandidateShift of the tracked set needs this frame's features but not its detections: enqueue it first, then
        # start the next frame's trunk on the second stream -- everything that follows in this step (detection, two host
        # reads, matching, tracker update: ~200 tiny launches) then runs beside that trunk, while the two big kernel groups
        # (temporal-fusion convolutions, trunk) never share the GPU
        Pn = sum(self.prev_n) if self.prev is not None else 0
        if Pn:
            self._shift_prev(P4, T2S, proto, dev)
        self._prefetch_trunk(next_frames)
        det, counts, det_scores = self._detections(pred, pred["mask_coeff"], self.max_instances)
        D = sum(counts)
        if D:
            det["mask"], det_bits = ops.lincomb_sigmoid_crop_bits(proto, det["mask_coeff"], det["box"], det["clip"])
        else:
            det["mask"], det_bits = proto.new_zeros(0, proto.shape[1], proto.shape[2]), None
        tmr.toc("det_gather_masks")
        if self.device_tracker:
            return self._update_dev(det, det_bits, counts, Pn, P4, T2S, proto, dev)

        if self.prev is None:
            # first frame of every clip (track_TF.py:88-93): the detections become the tracked set
            self.prev, self._bits = det, det_bits
            self.prev_n = list(counts)
            self.tracked = [[0] * k for k in counts]
            self._upload_meta(dev, None)
        else:
            prev = self.prev
            if D and Pn:
                ids = self._match_scores(det, det_bits, self._prev_bits, proto.shape[1] * proto.shape[2])[0].tolist()  # host read 2
                tmr.toc("match_scores")
            else:
                ids = [0] * D
            # greedy resolution (track_TF.py:132-156) per clip on host scalars -> one gather plan for all clips
            plan, self.prev_n, self.tracked = track_host.match_tf(self.prev_n, self.tracked, counts, ids, det_scores, self.max_instances)
            plan_dev = self._upload_meta(dev, plan if D else None)
            if D:
                # prev <- cat(prev, det)[plan] for every row tensor but the soft masks (see _TrackedRows); the masks' bit words ride
                # along instead: the keep rule of _pack_outputs counts pixels on them
                keys = tuple(k for k in _ROW_KEYS if k != "mask") + ("clip",)
                pbits = self._prev_bits if Pn else det_bits[:0]
                rows = ops.gather_rows2([prev[k] for k in keys] + [pbits], [det[k] for k in keys] + [det_bits], plan_dev, Pn)
                merged = _TrackedRows()
                for k, t in zip(keys, rows[:-1]):
                    merged[k] = t
                merged.defer_mask(prev["mask"], det["mask"], plan_dev, Pn, plan)
                self.prev, self._bits = merged, rows[-1]
            else:
                self._bits = self._prev_bits if Pn else None
            tmr.toc("tracker_update")
        self.prev_feat = (P4, T2S)
        self.t += 1
        out = self._pack_outputs(dev)
        tmr.toc("pack")
        return out

    def _update_dev(self, det, det_bits, counts, Pn, P4, T2S, proto, dev):
        """The tracker update of _step_tf with device_tracker: the resolution is a kernel on device inputs, the row counts it decides are
        copied to pinned memory behind it and read by _settle, and this step's gather and packing run at the capacity Pn + D (the plan's
        padding names row 0; pack_tracked walks the clips' new offsets, so a padding row is never packed).  Nothing here reads self.prev /
        prev_n through their properties once the resolution is enqueued: that would settle, i.e. wait."""
        tmr, D = self.timer, sum(counts)
        cnt = self._cnt_dev
        if self._prev is None:
            # first frame of every clip: the detections become the tracked set (counts are host integers already)
            self._prev, self._bits, self._prev_n = det, det_bits, list(counts)
            self._off_dev = F.pad(torch.cumsum(cnt, 0, dtype=torch.int32), (1, 0))
            self._tm_dev = torch.zeros(D, dtype=torch.int32, device=dev)
        elif D:
            prev = self._prev
            match = self._match_scores(det, det_bits, self._prev_bits, proto.shape[1] * proto.shape[2])[0] if Pn else None
            tmr.toc("match_scores")
            plan, new_off, new_tm = ops.track_resolve_tf(match, det["score"], cnt, self._off_dev, self._tm_dev if Pn else None, Pn, D, self.max_instances)
            slot = self._n_resolved % 2
            self._n_resolved += 1
            if self._off_pin[slot] is None:
                self._off_pin[slot] = torch.empty(self.B + 1, dtype=torch.int32).pin_memory()
            self._off_pin[slot].copy_(new_off, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            keys = tuple(k for k in _ROW_KEYS if k != "mask") + ("clip",)
            pbits = self._prev_bits if Pn else det_bits[:0]
            rows = ops.gather_rows2([prev[k] for k in keys] + [pbits], [det[k] for k in keys] + [det_bits], plan, Pn)
            merged = _TrackedRows()
            for k, t in zip(keys, rows[:-1]):
                merged[k] = t
            merged.defer_mask(prev["mask"], det["mask"], plan, Pn)
            self._prev, self._bits, self._tm_dev, self._off_dev = merged, rows[-1], new_tm, new_off
            self._unsettled = (self._off_pin[slot], ev)
        else:
            self._bits = self._prev_bits if Pn else None
        tmr.toc("tracker_update")
        self.prev_feat = (P4, T2S)
        self.t += 1
        prev = self._prev
        if prev is None or prev["box"].shape[0] == 0:
            out = torch.zeros(self.B, self.cfg.nms_top_k, DET_COLS, device=dev)
        else:
            out = ops.pack_tracked_bits(self._bits, prev["score"], self._tm_dev, self._off_dev, prev["box"], prev["class"], prev["mask_coeff"], self.B,
                                        self.cfg.nms_top_k, DET_COLS, 10, self.cfg.eval_conf_thresh)
        tmr.toc("pack")
        return out

    def _step_nontf(self, frames, first, next_frames):
        """One frame of every clip through Detect + Track (reference detection.py:98-137, track.py:56-179; STMask.py:323-325): the frame's own
        detections leave with their object ids; the tracker keeps BINARY masks (their bit words here) and replaces a matched object's row only while
        (mask_ious > 0.3).sum() < 2 (track.py:162).  All clips per launch; two host reads per step as the temporal-fusion path."""
        cfg, B = self.cfg, self.B
        dev = frames.device
        if first:
            self.prev, self.prev_n, self._bits = None, [0] * B, None
        fpn_outs, pred, _ = self._take_trunk(frames)
        self._prefetch_trunk(next_frames)
        proto = pred["proto"]
        mc = torch.tanh(pred["mask_coeff"])                               # STMask.py:324 (generate_mask applies tanh AGAIN on this path: reproduced)
        det, counts, det_scores = self._detections(pred, mc)
        D = sum(counts)
        if not cfg.train_track:
            det["track"] = F.normalize(det["mask_coeff"], dim=1)
        out = torch.zeros(B, cfg.nms_top_k, DET_COLS, device=dev)
        if D == 0:
            self._last = None
            self.t += 1
            return out
        det_mask, det_bits = ops.lincomb_sigmoid_crop_bits(proto, det["mask_coeff"], det["box"], det["clip"])
        Pn = sum(self.prev_n)
        if Pn:
            self._upload_meta(dev, None)
            match, miou = self._match_scores(det, det_bits, self._bits, proto.shape[1] * proto.shape[2])
            ids, n_over = torch.stack([match, (miou > 0.3).sum(1).to(torch.int32)]).tolist()   # host read 2: match ids + the update gate's counts
        else:
            ids, n_over = [0] * D, [0] * D
        plan, new_n, obj_ids = track_host.match_nontf(self.prev_n, counts, ids, det_scores, n_over)
        # output rows: the frame's detections with an object id (remove_false_inst, track.py:172-179), in detection order
        rows, dst_b, dst_j = track_host.output_rows(counts, obj_ids, cfg.remove_false_inst)
        meta = torch.tensor(plan + rows + dst_b + dst_j + [obj_ids[r] for r in rows], dtype=torch.int32).to(dev, non_blocking=True)
        nP, nR = len(plan), len(rows)
        plan_dev = meta[:nP]
        r_dev, b_dev, j_dev, id_dev = (meta[nP + k * nR:nP + (k + 1) * nR].long() for k in range(4))
        keys = ("box", "mask_coeff", "track", "class", "score", "clip")
        pbits = self._bits if Pn else det_bits[:0]
        a_rows = [self.prev[k] for k in keys] if Pn else [det[k][:0] for k in keys]
        merged = ops.gather_rows2(a_rows + [pbits], [det[k] for k in keys] + [det_bits], plan_dev, Pn)
        self.prev = dict(zip(keys, merged[:-1]))
        self._bits = merged[-1]
        self.prev_n = new_n
        if nR:
            out[b_dev, j_dev, 0:4] = det["box"][r_dev]
            out[b_dev, j_dev, 4] = det["score"][r_dev]
            out[b_dev, j_dev, 5] = det["class"][r_dev].float()
            out[b_dev, j_dev, 6] = id_dev.float()
            out[b_dev, j_dev, 7] = 1.0
            out[b_dev, j_dev, 8:8 + det["mask_coeff"].shape[1]] = det["mask_coeff"][r_dev]
        self._last = (det, det_mask, r_dev, b_dev, id_dev)
        self.t += 1
        return out

    def _upload_meta(self, dev, plan):
        """One host -> device copy per step: [clip row offsets (B + 1) | frames-since-last-match counters | gather plan] -> the plan on the
        device; sets _off_dev and _tm_dev.  (The non-TF tracker keeps no counters and sends its plan with its output rows: for it this is the
        offsets alone.)"""
        off = track_host.clip_offsets(self.prev_n)
        tm = [v for t in self.tracked for v in t]
        meta = torch.tensor(off + tm + (plan or []), dtype=torch.int32).to(dev, non_blocking=True)
        nb = len(off)
        self._off_dev, self._tm_dev = meta[:nb], meta[nb:nb + len(tm)]
        return meta[nb + len(tm):]

    def _pack_outputs(self, dev):
        """keep rule of track_TF.py:158-165 on device, scattered into [B, top_k, 40] without a host sync (two launches)."""
        cfg, B, prev = self.cfg, self.B, self.prev
        if prev is None or sum(self.prev_n) == 0:
            return torch.zeros(B, cfg.nms_top_k, DET_COLS, device=dev)
        return ops.pack_tracked_bits(self._bits, prev["score"], self._tm_dev, self._off_dev, prev["box"], prev["class"], prev["mask_coeff"], B,
                                     cfg.nms_top_k, DET_COLS, 10, cfg.eval_conf_thresh)

    def detections(self):
        """Reference-shaped per-clip detection dicts of the last step (host sync; for tests and users who want them)."""
        cfg, prev = self.cfg, self.prev
        outs = []
        if not self.tf:
            # the frame's own detections with their object ids; masks binary (track.py:88)
            if self._last is None:
                return [{} for _ in range(self.B)]
            det, det_mask, r_dev, b_dev, id_dev = self._last
            for b in range(self.B):
                sel = r_dev[b_dev == b]
                d = {k: det[k].index_select(0, sel) for k in ("box", "mask_coeff", "track", "class", "score")}
                d["mask"] = det_mask.index_select(0, sel).gt(0.5).float()
                d["box_ids"] = id_dev[b_dev == b]
                outs.append(d)
            return outs
        if prev is None:
            return [{} for _ in range(self.B)]
        dev = prev["box"].device
        tm = torch.tensor([v for t in self.tracked for v in t], device=dev)
        keep = (tm <= 10) & (prev["mask"].gt(0.5).sum([1, 2]) > 1) & (prev["score"] > cfg.eval_conf_thresh)
        off = track_host.clip_offsets(self.prev_n)
        for b in range(self.B):
            k = torch.nonzero(keep[off[b]:off[b + 1]]).view(-1)
            d = {key: prev[key][off[b]:off[b + 1]].index_select(0, k) for key in _ROW_KEYS}
            d["box_ids"] = k
            outs.append(d)
        return outs

    def tracked_rows(self):
        """The rows detections() would report for the last step, flat over all clips and without a host wait -- the input of the batched output
        stage (output_utils.OutputStageBatch): {"mask" [N,mh,mw] (soft; binary 0/1 on the non-TF path, as detections() hands them out), "box"
        [N,4], "score" [N], "class" [N], "frame" int32 [N] (the clip), "box_id" [N], "keep" bool [N]}, or None when there are no rows.  With
        temporal fusion the rows are the whole tracked set and "keep" is the rule detections() applies (track_TF.py:158-165); a kept row's
        box_id is what detections() reports: its index among its clip's tracked rows.  box and score are copies (the next step shifts the
        tracked set in place)."""
        if not self.tf:
            if self._last is None:
                return None
            det, det_mask, r_dev, b_dev, id_dev = self._last
            if r_dev.numel() == 0:
                return None
            return {"mask": det_mask.index_select(0, r_dev).gt(0.5).float(), "box": det["box"].index_select(0, r_dev),
                    "score": det["score"].index_select(0, r_dev), "class": det["class"].index_select(0, r_dev),
                    "frame": b_dev.to(torch.int32), "box_id": id_dev, "keep": torch.ones_like(r_dev, dtype=torch.bool)}
        prev = self._prev       # (not the property: with device_tracker an unsettled step's rows stand at their capacity, and this must not wait)
        if prev is None or (prev["box"].shape[0] if self._unsettled is not None else sum(self._prev_n)) == 0:
            return None
        mask, clip = prev["mask"], prev["clip"].to(torch.int32)
        keep = (self._tm_dev <= 10) & (mask.gt(0.5).sum([1, 2]) > 1) & (prev["score"] > self.cfg.eval_conf_thresh)
        if self._unsettled is not None:                     # padding rows past the new row count (known to the device alone) are never reported
            keep = keep & (torch.arange(keep.shape[0], device=keep.device, dtype=torch.int32) < self._off_dev[-1])
        box_id = torch.arange(clip.shape[0], device=clip.device, dtype=torch.int32) - self._off_dev.index_select(0, clip.long())
        return {"mask": mask, "box": prev["box"].clone(), "score": prev["score"].clone(), "class": prev["class"], "frame": clip, "box_id": box_id,
                "keep": keep}
