"""Validation during training: the reference's compute_validation_map (train.py:366-378) and validation (eval.py:503-573) -- switch the net to
eval, run the validation split, dump the results JSON, score it, go back to training -- without touching the net that trains.

``InferenceTwin`` is the eval net: ONE deepcopy of the live STMask, taken through fuse.optimize_for_inference once, with a record of where every
one of its tensors comes from in the live net (a plain copy, a convolution weight or bias with its BatchNorm folded in, a bottleneck's bias3).
``refresh()`` rewrites those tensors in place from the live net's current values in fuse._fold's arithmetic (s = gamma / sqrt(var + eps),
w' = w * s, b' = (b - mean) * s + beta; bit-equal to a fresh copy folded by torch) -- fold="device": csrc/fold.hip, 64 tensors a launch;
fold="torch": the same expressions as torch ops with out=, tensor by tensor, which also runs on the CPU and is the yardstick of the device form
-- and, on a GPU, builds the planar graph again from them (fuse.build_planar / attach_planar).  The packed planar weights and the captured HIP
graphs are rebuilt, not updated in place: the fp16 plane formats derive a per-layer power-of-two scale from the weights, whose reciprocal is a
kernel argument a captured graph freezes.  So every refresh opens a new ``generation``; a pipeline or VideoBatcher built on an older one is
stale, and the twin refuses to run it.

``validation()`` is the hook: refresh, serve ``dataset.videos()`` (datasets.YTVISValSet: frames read when asked for) through a VideoBatcher on
the twin into the results JSON, score it with eval_utils.calc_metrics when there is an annotation file.  The live net is never switched to
eval; its parameters, buffers, flags, the optimizer state and the random generators are as they were.

Not built: multi-GPU validation, iouType='bbox', compute_validation_loss, in-place update of the packed planar weights."""
import copy

import torch
import torch.nn as nn

from . import _lib, eval_utils, fuse, output_utils
from ._lib import FoldRow, StmError, c_p

FOLDS = ("device", "torch")
COPY, WEIGHT, BIAS, BIAS3 = "copy", "weight", "bias", "bias3"
# launches of the last refresh()'s parameter write: kernel launches of csrc/fold.hip, or torch operations of the torch form
COUNTERS = {"fold_launches": 0, "torch_ops": 0}


def _fold_pairs(net):
    """(conv name, bn name) of every BatchNorm fuse.fold_batchnorm folds, in its order, on a net that has not been folded."""
    pairs = []
    bb = net.backbone
    if isinstance(bb.bn1, nn.BatchNorm2d):
        pairs.append(("backbone.conv1", "backbone.bn1"))
    for li, layer in enumerate(bb.layers):
        for bi, blk in enumerate(layer):
            at = f"backbone.layers.{li}.{bi}"
            for cname, bname in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3")):
                if isinstance(getattr(blk, bname), nn.BatchNorm2d):
                    pairs.append((f"{at}.{cname}", f"{at}.{bname}"))
            if blk.downsample is not None and isinstance(blk.downsample[1], nn.BatchNorm2d):
                pairs.append((f"{at}.downsample.0", f"{at}.downsample.1"))
    return pairs


def _dense_f32(t):
    return t.dtype == torch.float32 and t.is_contiguous()


class _Source:
    """Where one tensor of the twin comes from: kind, dst (the twin's tensor), src (the live tensor or None), bn (the live BatchNorm or None)."""
    __slots__ = ("name", "kind", "dst", "src", "bn", "scale", "parts")

    def __init__(self, name, kind, dst, src=None, bn=None, parts=None):
        self.name, self.kind, self.dst, self.src, self.bn, self.parts = name, kind, dst, src, bn, parts
        self.scale = None      # torch form: the BatchNorm's scale buffer, shared by the weight and the bias row of one convolution


class InferenceTwin:
    """InferenceTwin(net, planes="fp16x2", fold="device"): see the module docstring.  net: an unfused STMask as STMask(cfg) builds it, in train or
    eval mode, on the CPU (fold="torch" only; no planar graph) or a GPU.  .net is the eval net, .generation counts the refreshes."""

    def __init__(self, net, planes="fp16x2", fold="device"):
        if fold not in FOLDS:
            raise ValueError(f"InferenceTwin: fold={fold!r}, expected 'device' or 'torch'")
        if getattr(net, "_planar", None) is not None or any(getattr(m, "fuse_relu", False) or hasattr(m, "bias3") for m in net.modules()):
            raise ValueError("InferenceTwin: the live net went through fuse.optimize_for_inference; the twin is made from an unfused net")
        self.live, self.planes, self.fold = net, planes, fold
        self.device = next(net.parameters()).device
        self.planar = self.device.type == "cuda"
        if fold == "device" and not self.planar:
            raise StmError("InferenceTwin: fold='device' is a HIP kernel for the MI355X and the net is on the CPU; use fold='torch' there")
        self._pairs = _fold_pairs(net)
        twin = copy.deepcopy(net)
        twin.eval()
        fuse.optimize_for_inference(twin, planar=self.planar, planes=planes)
        for p in twin.parameters():               # the eval net: no gradients (a deepcopy brings the live net's along)
            p.requires_grad_(False)
            p.grad = None
        self.net = twin
        self.generation = 0
        self.sources = []
        self.bind()

    # ---- the record of sources ------------------------------------------------------------------------------------------------------
    def bind(self):
        """Record, for every tensor of the twin's state_dict() and every non-persistent buffer it registered, where its value comes from in the
        live net; raises StmError naming a tensor that has no source (or whose source has another shape or dtype)."""
        live_mods = dict(self.live.named_modules())
        live_sd = self.live.state_dict(keep_vars=True)
        folded = {}
        for conv, bn in self._pairs:
            folded[conv + ".weight"] = (WEIGHT, conv, bn)
            folded[conv + ".bias"] = (BIAS, conv, bn)
        sources, scales = [], {}
        twin_sd = self.net.state_dict(keep_vars=True)
        for name, dst in twin_sd.items():
            if name in folded:
                kind, conv, bn = folded[name]
                src = live_sd.get(name)
                if kind == WEIGHT and src is None:
                    raise StmError(f"InferenceTwin: {name} has no source in the live net")
                row = _Source(name, kind, dst, src, live_mods[bn])
                if dst.dim() < 1 or dst.shape[0] != row.bn.weight.shape[0]:
                    raise StmError(f"InferenceTwin: {name} {tuple(dst.shape)} does not have the {row.bn.weight.shape[0]} channels of {bn}")
                row.scale = scales.setdefault(bn, torch.empty_like(row.bn.weight.detach()))
            elif name in live_sd:
                row = _Source(name, COPY, dst, live_sd[name])
            else:
                raise StmError(f"InferenceTwin: {name} of the optimised copy has no source in the live net")
            if row.src is not None and (row.src.shape != dst.shape or row.src.dtype != dst.dtype):
                raise StmError(f"InferenceTwin: {name} is {tuple(dst.shape)} {dst.dtype}, its source {tuple(row.src.shape)} {row.src.dtype}")
            sources.append(row)
        twin_mods = dict(self.net.named_modules())
        for name, dst in self.net.named_buffers():
            if name in twin_sd:
                continue
            owner, _, leaf = name.rpartition(".")
            blk = twin_mods.get(owner)
            if leaf != "bias3" or not isinstance(blk, fuse._FusedBottleneck):
                raise StmError(f"InferenceTwin: the buffer {name} of the optimised copy has no source in the live net")
            parts = [blk.conv3.bias] + ([blk.downsample[0].bias] if blk.downsample is not None else [])
            sources.append(_Source(name, BIAS3, dst, parts=parts))      # of the FOLDED values: written after the rows above
        self.sources = sources

    # ---- refresh --------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def write_parameters(self):
        """The parameter write of refresh() alone: every tensor of the twin from the live net's current values, in place."""
        COUNTERS["fold_launches"] = COUNTERS["torch_ops"] = 0
        if self.fold == "device":
            self._write_device()
        else:
            self._write_torch()
        for row in self.sources:
            if row.kind == BIAS3:
                if len(row.parts) == 2:
                    torch.add(row.parts[0], row.parts[1], out=row.dst)
                else:
                    row.dst.copy_(row.parts[0])
                COUNTERS["torch_ops"] += 1

    def _write_torch(self):
        done = set()
        for row in self.sources:
            if row.kind == COPY:
                row.dst.copy_(row.src)
                COUNTERS["torch_ops"] += 1
            elif row.kind in (WEIGHT, BIAS):
                bn, s = row.bn, row.scale
                if id(s) not in done:         # s = gamma / sqrt(var + eps), once a BatchNorm
                    torch.add(bn.running_var, bn.eps, out=s)
                    torch.sqrt(s, out=s)
                    torch.div(bn.weight, s, out=s)
                    done.add(id(s))
                    COUNTERS["torch_ops"] += 3
                if row.kind == WEIGHT:
                    torch.mul(row.src, s.view(-1, *([1] * (row.dst.dim() - 1))), out=row.dst)
                    COUNTERS["torch_ops"] += 1
                else:
                    if row.src is None:           # a convolution without bias: _fold's zeros_like(mean) - mean
                        row.dst.zero_()
                        row.dst.sub_(bn.running_mean)
                        COUNTERS["torch_ops"] += 1
                    else:
                        torch.sub(row.src, bn.running_mean, out=row.dst)
                    row.dst.mul_(s)
                    row.dst.add_(bn.bias)
                    COUNTERS["torch_ops"] += 3

    def _write_device(self):
        rows = []
        for row in self.sources:
            if row.kind == BIAS3:
                continue
            dst, src = row.dst, row.src
            if row.kind == COPY and not (_dense_f32(dst) and _dense_f32(src)):
                dst.copy_(src)                # a tensor that is not dense fp32 (an integer counter): a plain copy, nothing to fold
                COUNTERS["torch_ops"] += 1
                continue
            rows.append(fold_row(row.kind, dst, src, row.bn))
        with torch.cuda.device(self.device):
            COUNTERS["fold_launches"] += fold_rows(rows)

    def refresh(self):
        """Rewrite every tensor of the twin from the live net; on a GPU build the planar graph again and open a new generation."""
        self.write_parameters()
        if self.planar:
            self.net._planar_bf16x3 = None            # the range fallback's graph (pipeline.py) was packed from the old weights
            fuse.attach_planar(self.net, fuse.build_planar(self.net, self.planes))
        self.generation += 1
        return self

    # ---- serving --------------------------------------------------------------------------------------------------------------------------
    def batcher(self, n_slots, score_threshold=None, **kw):
        """A serve.VideoBatcher on the current generation, batched_output=True by default; with batched output the output stage drops rows at
        score_threshold (default: cfg.eval_conf_thresh, the reference's validation)."""
        from .serve import VideoBatcher
        kw.setdefault("batched_output", True)
        if kw["batched_output"] and kw.get("output_stage") is None:
            thr = self.net.cfg.eval_conf_thresh if score_threshold is None else score_threshold
            classes = kw.get("classes") or ["class_%d" % i for i in range(1, self.net.cfg.num_classes)]
            kw["output_stage"] = output_utils.OutputStageBatch(classes, score_threshold=thr)
        vb = VideoBatcher(self.net, n_slots, **kw)
        vb.twin_generation = self.generation
        return vb

    def run(self, batcher, videos, out_file=None, **kw):
        """batcher.run(videos, out_file) after the check that it was built on this generation."""
        built = getattr(batcher, "twin_generation", None)
        if built is not None and built != self.generation:
            raise StmError(f"InferenceTwin: this batcher was built on generation {built}, the twin is at {self.generation}: its packed weights "
                           "and captured graphs are those of older parameters; take a new one from twin.batcher()")
        return batcher.run(videos, out_file=out_file, **kw)


def fold_row(kind, dst, src, bn=None):
    """One _lib.FoldRow (csrc/fold.h stm_fold_row) from tensors; checks what the kernel relies on."""
    code = {COPY: _lib.FOLD_COPY, WEIGHT: _lib.FOLD_WEIGHT, BIAS: _lib.FOLD_BIAS}[kind]
    for what, t in (("dst", dst), ("src", src)):
        if t is not None and not (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()):
            raise StmError(f"fold_row: {what} must be a dense float32 GPU tensor, got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    if src is not None and src.numel() != dst.numel():
        raise StmError(f"fold_row: dst has {dst.numel()} elements, src {src.numel()}")
    r = FoldRow()
    r.dst, r.src, r.numel, r.kind, r.inner = dst.data_ptr(), (src.data_ptr() if src is not None else None), dst.numel(), code, 1
    if kind != COPY:
        ch = bn.weight.numel()
        for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
            if not (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == ch):
                raise StmError("fold_row: the BatchNorm's four tensors must be contiguous float32 GPU tensors of one length")
        if ch == 0 or dst.numel() % ch:
            raise StmError(f"fold_row: {dst.numel()} elements do not make {ch} channels")
        r.inner, r.eps = dst.numel() // ch, bn.eps
        r.gamma, r.var = bn.weight.data_ptr(), bn.running_var.data_ptr()
        if kind == BIAS:
            r.beta, r.mean = bn.bias.data_ptr(), bn.running_mean.data_ptr()
    return r


def fold_rows(rows, stream=None):
    """stm_fold_rows_f32 over any number of rows, _lib.FOLD_MAX_ROWS a call -> the number of calls (launches, when the rows share one eps)."""
    calls = 0
    stream = c_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    for k in range(0, len(rows), _lib.FOLD_MAX_ROWS):
        part = rows[k:k + _lib.FOLD_MAX_ROWS]
        _lib.private_call("stm_fold_rows_f32", (FoldRow * len(part))(*part), len(part), stream)
        calls += 1
    return calls


def validation(twin, dataset, out_json, ann_file=None, metrics_file=None, n_slots=8, scorer=None, batcher=None, decode="host", decode_split=None):
    """The round trip: twin.refresh(); the split through a VideoBatcher on the twin into out_json (results2json_videoseg's file, rows under
    cfg.eval_conf_thresh dropped as in the reference's validation); with ann_file, (scorer or eval_utils.calc_metrics)(ann_file, out_json,
    output_file=metrics_file) -- the two branches of eval.py:566-573.  -> the metrics, or None when nothing was scored.  batcher (anything with
    run(videos, out_file=...)) and scorer are injectable.  Nothing of the live net, the optimizer or the random generators changes.
    decode="device": the dataset is a YTVISValSet(decode="device"), whose frames are still JPEG bytes, and the batcher made here decodes them on
    the device (prep=jpeg.compressed_prep(split=decode_split), decode_split defaulting to the dataset's); a batcher handed in must bring such a
    prep itself."""
    if decode not in ("host", "device"):
        raise ValueError(f"validation: decode={decode!r}")
    if getattr(dataset, "decode", decode) != decode:
        raise StmError(f"validation: decode={decode!r}, the dataset was made with decode={dataset.decode!r}")
    twin.refresh()
    if batcher is not None:
        vb = batcher
    elif decode == "device":
        from . import jpeg
        vb = twin.batcher(n_slots, prep=jpeg.compressed_prep(split=decode_split if decode_split is not None else getattr(dataset, "decode_split", None)))
    else:
        vb = twin.batcher(n_slots)
    twin.run(vb, dataset.videos(), out_file=out_json)
    if ann_file is None:
        return None
    return (scorer or eval_utils.calc_metrics)(ann_file, out_json, output_file=metrics_file)


def result_paths(checkpoint_path):
    """(out_json, metrics_file) of a checkpoint: its path with .pth replaced by .json and .txt (train.py:369, eval.py:573)."""
    stem = checkpoint_path[:-len(".pth")] if checkpoint_path.endswith(".pth") else checkpoint_path
    return stem + ".json", stem + ".txt"
