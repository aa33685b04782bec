"""Shared driver of the long-clip tracker tests (test_gpu_long_clips.py on the GPU, test_host_model_cpu.py under the CPU oracle): run a clip of a
model_full_tf* golden (gen_golden.py gen_model_full_tf) through BatchedClipPipeline beside a second clip and compare clip 0 with the reference,
frame by frame: the tracker's whole state, the keep rule's decisions, the reported set from detections() and from the packed step() output."""
import numpy as np
import torch

from stmask_amd import synthetic
from stmask_amd.dist import unpack_detections

COMPANION_SEED = 2


def golden_clips(g, zero_companion=()):
    """[2, T, 3, H, W]: clip 0 = the golden's frames (frame_src: indices into synthetic_clip(..., seed=clip_seed), -1 = all zeros), clip 1 = the same
    frame indices of another seed, all-zero on the frames listed in zero_companion (where clip 0 is all-zero too, a whole step detects nothing)."""
    h, w = [int(v) for v in g["frames_hw"]]
    src = [int(v) for v in g["frame_src"]]
    out = []
    for b, seed in enumerate((int(g["clip_seed"]), COMPANION_SEED)):
        clip = synthetic.synthetic_clip(max(src) + 1, h, w, seed=seed)
        zero = [s < 0 for s in src] if b == 0 else [t in zero_companion for t in range(len(src))]
        out.append(torch.stack([torch.zeros_like(clip[0]) if z else clip[max(s, 0) if b == 0 else t] for t, (s, z) in enumerate(zip(src, zero))]))
    return torch.stack(out)


def _bit_counts(bits):
    """Pixels set per row of a mask bit table: int64 words [n, ceil(h*w/64)] (the kernels), or the bool masks the CPU oracle stands in with."""
    b = bits.cpu()
    if b.dtype == torch.bool:
        return b.sum(1)
    return torch.from_numpy(np.unpackbits(b.contiguous().numpy().view(np.uint8), axis=1).sum(1).astype(np.int64))


def _excused(g, t):
    return set(int(v) for v in g[f"t{t}_excused_rows"].tolist())


def rules_decided(g):
    """From the golden alone: which keep conditions (1: age <= 10, 2: > 1 mask pixel, 3: score > eval_conf_thresh) were the ONLY failing one for some
    non-excused row of some frame, and how many non-excused rows were matched again after >= 5 frames without a match."""
    T = int(g["n_frames"])
    decided, rematched = set(), 0
    for t in range(T):
        ex = _excused(g, t)
        for c in (1, 2, 3):
            if any(int(i) not in ex for i in g[f"t{t}_only_cond{c}"].tolist()):
                decided.add(c)
        rematched += sum(int(i) not in ex for i in g[f"t{t}_rematched"].tolist())
    return decided, rematched


def _mask_delta(got, ref):
    """soft_mask_delta of test_gpu_parity: values where both sides are inside their crop, and the count of pixels where only one side is."""
    both = (got != 0) & (ref != 0)
    d = (got - ref) * both
    n = both.sum(dim=(1, 2)).clamp(min=1)
    return (d.pow(2).sum(dim=(1, 2)) / n).sqrt(), d.abs().amax(dim=(1, 2)), ((got != 0) ^ (ref != 0)).sum(dim=(1, 2))


def _check_reported(tag, got, g, t, ex, tol):
    ids = [int(v) for v in got["box_ids"].cpu().tolist()]
    ref_ids = [int(v) for v in g[f"t{t}_box_ids"].tolist()]
    assert [i for i in ids if i not in ex] == [i for i in ref_ids if i not in ex], (tag, t, ids, ref_ids)
    pos = {i: k for k, i in enumerate(ids)}
    keep = [k for k, i in enumerate(ref_ids) if i not in ex]
    if not keep:
        return 0.0
    mine = torch.tensor([pos[ref_ids[k]] for k in keep])
    keep = torch.tensor(keep)
    assert got["class"].cpu()[mine].tolist() == g[f"t{t}_class"][keep].tolist(), (tag, t)
    d = max((got["box"].cpu()[mine] - g[f"t{t}_box"][keep]).abs().max().item(),
            (got["score"].cpu()[mine] - g[f"t{t}_score"][keep]).abs().max().item())
    assert d < tol, (tag, t, d)
    return d


def run_long_clip(tag, pipe, g, clips, tol=5e-6, tol_coeff=1e-5, mask_rms=1e-4, mask_abs=2e-4, next_depth=0, zero_companion=()):
    """Drive pipe over clips [2, T, ...] or a list of T frame batches [2, ...] (already on the pipeline's device and memory format) and compare clip 0
    with the golden g.  next_depth > 0: hand step() the next next_depth frames as the benchmark's Runner does.  tol: boxes and scores; tol_coeff: the
    float64 sum and sum |.| of a row's 32 mask coefficients, relative to sum |.|.  Returns a per-frame report."""
    T = int(g["n_frames"])
    mask_frames = set(int(v) for v in g["mask_frames"].tolist())
    n_masks = int(g["n_masks"])
    frames = list(clips) if isinstance(clips, (list, tuple)) else [clips[:, t] for t in range(T)]
    rep = {}
    for t in range(T):
        nxt = [frames[t + k] for k in range(1, next_depth + 1) if t + k < T] if next_depth else None
        n1_before, tm1_before = pipe.prev_n[1], list(pipe.tracked[1])
        packed = pipe.step(frames[t], is_first=(t == 0), next_frames=nxt or None)
        dets = pipe.detections()
        det = dets[0]
        for b in range(2):
            # both clips: the packed rows (kernel keep rule on the uploaded counters and the masks' bit words) are the rows detections() keeps (the
            # keep rule in torch on the soft masks) -- a stale or misrouted bit word or counter breaks this where the masks or ages have changed
            un = unpack_detections(packed[b].cpu())
            ids_b = dets[b]["box_ids"].cpu() if dets[b] else torch.zeros(0, dtype=torch.int64)
            assert torch.equal(un["box_ids"], ids_b[:packed.shape[1]]), (tag, t, b)
            if len(ids_b):
                assert torch.equal(un["class"], dets[b]["class"].cpu()) and torch.equal(un["box"], dets[b]["box"].cpu()), (tag, t, b)
        rows = sum(pipe.prev_n)
        if rows:
            # the bit words the packed output's keep rule counts are those of the tracked set's CURRENT soft masks, row for row: after a match (the
            # gathered words), after a frame without any detection (CandidateShift's words) and after a per-clip drop
            assert torch.equal(_bit_counts(pipe._bits)[:rows], (pipe.prev["mask"][:rows] > 0.5).sum(dim=(1, 2)).cpu()), (tag, t)
        if t in zero_companion:
            # the companion detected nothing either: the step had no detection at all, its tracked rows only aged
            assert pipe.prev_n[1] == n1_before > 0 and pipe.tracked[1] == [v + 1 for v in tm1_before], (tag, t)
        ex = _excused(g, t)
        assert len(ex) <= max(2, pipe.prev_n[0] // 50) and not bool(g[f"t{t}_count_fragile"]), (tag, t, sorted(ex))
        # -- the tracker's state of clip 0: rows [0, prev_n[0]) (row = instance id)
        n = pipe.prev_n[0]
        ref_n = g[f"t{t}_state_box"].shape[0]
        assert n == ref_n, (tag, t, n, ref_n)
        r = dict(state_rows=n, reported=len(g[f"t{t}_box_ids"]), excused=len(ex))
        if n:
            ok = torch.tensor([i not in ex for i in range(n)])
            st = {k: pipe.prev[k][:n].cpu() for k in ("box", "score", "class", "mask")}
            assert st["class"][ok].tolist() == g[f"t{t}_state_class"][ok].tolist(), (tag, t)
            tm_ref = [int(v) for v in g[f"t{t}_state_tracked_mask"].tolist()]
            assert [v for i, v in enumerate(pipe.tracked[0]) if i not in ex] == [v for i, v in enumerate(tm_ref) if i not in ex], (tag, t)
            sb = (st["box"] - g[f"t{t}_state_box"])[ok].abs().max().item()
            ss = (st["score"] - g[f"t{t}_state_score"])[ok].abs().max().item()
            assert sb < tol and ss < tol, (tag, t, sb, ss)
            ms, ref_ms = st["mask"].double(), g[f"t{t}_state_mask_sums"]
            area = ref_ms[:, 0].clamp(min=1.0)
            cnt = (ms > 0.5).double().sum(dim=(1, 2))
            d_sum = ((ms.sum(dim=(1, 2)) - ref_ms[:, 0]).abs() / area)[ok].max().item()
            d_cnt = (cnt - ref_ms[:, 2]).abs()[ok].max().item()
            # a crop edge may move by one pixel row / column when a box moves by 1e-6: the sums get the perimeter's worth of slack -- but the keep
            # rule's pixel condition (> 1 pixel over 0.5, track_TF.py:162) must come out as the reference's on every non-excused row
            assert d_sum < 2e-2 and d_cnt <= 2 * (ms.shape[1] + ms.shape[2]), (tag, t, d_sum, d_cnt)
            assert torch.equal((cnt > 1)[ok], (ref_ms[:, 2] > 1)[ok]), (tag, t)
            # the 32 mask coefficients of every row (CandidateShift adds TemporalNet's shift to them frame after frame), as float64 (sum, sum |.|)
            # relative to the row's sum |.| (it grows on rows that stay unmatched)
            cs = pipe.prev["mask_coeff"][:n].cpu().double()
            ref_cs = g[f"t{t}_state_mask_coeff_sums"]
            d_coeff = ((torch.stack([cs.sum(1), cs.abs().sum(1)], 1) - ref_cs).abs().amax(1) / ref_cs[:, 1].clamp(min=1.0))[ok].max().item()
            assert d_coeff < tol_coeff, (tag, t, d_coeff)
            r.update(state_box=sb, state_score=ss, mask_sum_rel=d_sum, mask_count=d_cnt, state_coeff_sums=d_coeff)
        # -- the reported set: detections() (keep rule in torch on the soft masks) and the packed output (keep_flags_bits + pack_tracked kernels on
        # the uploaded counters and the masks' bit words)
        r["box"] = _check_reported(tag, det, g, t, ex, tol) if n else 0.0
        if not n:
            assert (packed[0, :, 7] > 0).sum().item() == 0 and len(g[f"t{t}_box_ids"]) == 0, (tag, t)
        else:
            assert len(g[f"t{t}_box_ids"]) <= packed.shape[1], (tag, t)          # (the packed format holds nms_top_k rows per clip)
            r["packed_box"] = _check_reported(tag + "/packed", unpack_detections(packed[0].cpu()), g, t, ex, tol)
        if t in mask_frames and len(g[f"t{t}_box_ids"]):
            ids = [int(v) for v in det["box_ids"].cpu().tolist()]
            sel = [(ids.index(int(i)), k) for k, i in enumerate(g[f"t{t}_box_ids"][:n_masks].tolist()) if int(i) not in ex]
            got_m = det["mask"].cpu()[torch.tensor([a for a, _ in sel])]
            rms, mx, edge = _mask_delta(got_m, g[f"t{t}_mask"][torch.tensor([b for _, b in sel])])
            assert rms.max().item() < mask_rms and mx.max().item() < mask_abs, (tag, t, rms.max().item(), mx.max().item())
            r.update(mask_rms=rms.max().item(), mask_abs=mx.max().item(), crop_edge_pixels=int(edge.max()))
        rep[f"t{t}"] = r
    return rep
