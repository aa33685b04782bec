"""Serving a queue of videos through the batched pipeline (continuous batching).

An evaluation split (YouTube-VIS, OVIS) is a queue of videos of different lengths and source sizes; the reference runs it one video at a time
and resets its tracker per video (track_TF.py:52-54,86-93).  ``VideoBatcher`` keeps ``n_slots`` videos in flight in one
``BatchedClipPipeline``: slot b holds one video, advances it one frame per step, and when that video ends the next queued video starts in the
same slot on the next step (``is_first[b] = True``; the other slots keep their tracker state).  With the queue empty a slot is idle
(``active[b] = False``).  Every frame's tracked detections go through the reference's output stage with that video's own ``img_meta``
(``output_utils.postprocess_ytbvis`` -> ``eval_utils.bbox2result_with_id``), and a finished video's frames become its YouTube-VIS records.

The whole schedule is known before the first step, so the batches of the next ``pipe.prefetch_depth`` steps are pre-processed ahead and handed
to the pipeline as ``next_frames`` (the same tensor objects the later steps pass as ``frames``): their trunks run beside the current step.

``VideoBatcher(..., batched_output=True)`` replaces the per-slot output stage by one batched device stage per step
(``pipeline.tracked_rows()`` -> ``output_utils.OutputStageBatch``): step s is submitted, step s + 1 runs, then step s's records are read, so the
host never waits for the step it has just enqueued.  The records are the same.

``run(..., on_frame=f)`` also draws every busy slot's tracked instances onto that slot's own source frame on the device (display.render_batch,
source mode: one launch per step) and calls f(video_id, frame_id, frame_u8) per slot; without it nothing is drawn.
"""
from collections import deque

import torch

from . import display, eval_utils, output_utils, preprocess


def schedule(lengths, n_slots):
    """FIFO slot assignment -> one row per step: per slot (video index, frame index) or None (idle).  A slot whose video has ended takes the
    next queued video on the next step; slots are served in index order.  The schedule ends when every slot is idle."""
    if n_slots < 1:
        raise ValueError("schedule: n_slots must be >= 1")
    if any(int(t) < 1 for t in lengths):
        raise ValueError("schedule: every video needs at least one frame")
    queue, cur, steps = deque(range(len(lengths))), [None] * n_slots, []
    while True:
        for b in range(n_slots):
            c = cur[b]
            if c is not None and c[1] + 1 < lengths[c[0]]:
                cur[b] = (c[0], c[1] + 1)
            else:
                cur[b] = (queue.popleft(), 0) if queue else None
        if all(c is None for c in cur):
            return steps
        steps.append(list(cur))


def device_prep(frames, frame_ids, size=(640, 360), channels_last=True):
    """Default pre-processing of one step: frames = per slot a uint8 [H, W, 3] frame (on the GPU, or pinned host memory: copied with
    non_blocking) or None for an idle slot.  Each run of consecutive busy slots is ONE stm_preprocess_u8_multi_f32 launch (per 64 frames) into
    its rows of the batch; idle rows are zero.  -> (batch [B, 3, 384, 640], per slot img_meta or None)."""
    busy = [f for f in frames if f is not None]
    dev = busy[0].device if busy and busy[0].is_cuda else torch.device("cuda")
    w, h = size
    batch = torch.empty(len(frames), 3, -(-h // 32) * 32, -(-w // 32) * 32, device=dev)
    metas = [None] * len(frames)
    b = 0
    while b < len(frames):
        e = b
        while e < len(frames) and (frames[e] is None) == (frames[b] is None):
            e += 1
        if frames[b] is None:
            batch[b:e].zero_()
        else:
            fs = [f if f.is_cuda else f.to(dev, non_blocking=True) for f in frames[b:e]]
            _, metas[b:e] = preprocess.preprocess_eval_frames_multi(fs, frame_ids[b:e], out=batch[b:e], size=size)
        b = e
    if channels_last:
        batch = batch.contiguous(memory_format=torch.channels_last)   # the layout of the optimized inference graph's trunk
    return batch, metas


class VideoBatcher:
    """run(videos) -> YouTube-VIS records of a queue of videos served ``n_slots`` at a time (module docstring).

    videos: sequence of (video_id, frames_u8) with frames_u8 uint8 [T_i, H_i, W_i, 3] on the GPU or in pinned host memory (T_i >= 1; sizes may
    differ between videos).  prep(frames, frame_ids) -> (batch, metas) pre-processes one step (default: device_prep); pipeline: the
    BatchedClipPipeline to drive (default: a new one on `net`) -- both injectable, so the scheduling can be exercised without a GPU; so is
    output_stage (submit(rows, metas) -> ticket, collect(ticket) -> per-slot records), which batched_output=True uses."""

    def __init__(self, net, n_slots, use_graph=True, lookahead=None, prep=None, pipeline=None, classes=None, batched_output=False,
                 output_stage=None):
        if pipeline is None:
            from .pipeline import BatchedClipPipeline
            pipeline = BatchedClipPipeline(net, n_slots)
        self.net, self.B, self.pipe = net, n_slots, pipeline
        self.pipe.use_graph = use_graph
        self.lookahead = lookahead
        self.prep = prep if prep is not None else device_prep
        self.classes = classes if classes is not None else ["class_%d" % i for i in range(1, net.cfg.num_classes)]
        # batched_output: one output stage per step for all busy slots (output_utils.OutputStageBatch on pipeline.tracked_rows(): a fixed number
        # of launches and one device -> host copy, read one step late) instead of postprocess_ytbvis per slot; the records are the same
        self.batched_output = bool(batched_output)
        self.output_stage = output_stage
        if self.batched_output and self.output_stage is None:
            self.output_stage = output_utils.OutputStageBatch(self.classes)
        self.steps = 0            # steps of the last run
        self.busy_slot_steps = 0  # active (slot, step) pairs of the last run

    def occupancy(self):
        """Active slot-steps / all slot-steps of the last run."""
        return self.busy_slot_steps / max(1, self.steps * self.B)

    @torch.no_grad()
    def run(self, videos, out_file=None, on_frame=None):
        """-> the YouTube-VIS records (or results2json_videoseg's output when out_file is given).  on_frame(video_id, frame_id, frame_u8):
        called per busy slot and step with its frame annotated on the device (uint8 [H, W, 3] in the frame's own channel order).  Not built:
        on_frame over videos whose frames are jpeg.CompressedFrames (prep=jpeg.compressed_prep): the drawing reads the source frame's pixels,
        which such a video does not hold; serve those without on_frame."""
        videos = list(videos)
        plan = schedule([int(v[1].shape[0]) for v in videos], self.B)
        depth = self.pipe.prefetch_depth if self.lookahead is None else int(self.lookahead)
        ready = deque()                                    # (batch, metas) of the next steps, in step order

        def prepare(s):
            row = plan[s]
            frames = [None if c is None else videos[c[0]][1][c[1]] for c in row]
            ids = [None if c is None else c[1] for c in row]
            return self.prep(frames, ids)

        frame_results = [[] for _ in videos]
        self.steps, self.busy_slot_steps = len(plan), 0
        pending = None                                     # batched output: (ticket, plan row) of the step whose records are still on the device

        def collect(ticket, row):
            for c, rec in zip(row, self.output_stage.collect(ticket)):
                if c is not None:
                    frame_results[c[0]].append(rec)
        for s, row in enumerate(plan):
            while len(ready) < 1 + depth and s + len(ready) < len(plan):
                ready.append(prepare(s + len(ready)))
            batch, metas = ready.popleft()
            is_first = [c is not None and c[1] == 0 for c in row]
            active = [c is not None for c in row]
            nxt = [r[0] for r in list(ready)[:depth]] if depth > 0 else None
            self.pipe.step(batch, is_first=is_first, next_frames=nxt or None, active=active)
            if self.batched_output:
                # this step's output stage is enqueued behind its kernels; the previous step's records are read while both run
                step_metas = [None if c is None else dict(metas[b], video_id=videos[c[0]][0], frame_id=c[1]) for b, c in enumerate(row)]
                ticket = self.output_stage.submit(self.pipe.tracked_rows(), step_metas)
                if pending is not None:
                    collect(*pending)
                pending = (ticket, row)
            dets = self.pipe.detections() if on_frame is not None or not self.batched_output else None
            if on_frame is not None:
                busy = [b for b, c in enumerate(row) if c is not None]
                dev = batch.device
                srcs = [videos[row[b][0]][1][row[b][1]] for b in busy]
                srcs = [f if f.device == dev else f.to(dev, non_blocking=True) for f in srcs]
                drawn = display.render_batch([dets[b] for b in busy], srcs, [metas[b] for b in busy], mode="source")
                for b, img in zip(busy, drawn):
                    on_frame(videos[row[b][0]][0], row[b][1], img)
            for b, c in enumerate(row):
                if c is None:
                    continue
                self.busy_slot_steps += 1
                if self.batched_output:
                    continue
                vid = videos[c[0]][0]
                meta = dict(metas[b], video_id=vid, frame_id=c[1])
                if dets[b] and dets[b]["box"].shape[0]:
                    post = output_utils.postprocess_ytbvis({"detection": dets[b]}, meta)
                    frame_results[c[0]].append(eval_utils.bbox2result_with_id(post, meta, self.classes))
                else:
                    frame_results[c[0]].append({"video_id": vid, "frame_id": c[1]})     # (what bbox2result_with_id gives an empty frame)
        if pending is not None:
            collect(*pending)                              # the last step
        order = sorted(range(len(videos)), key=lambda i: videos[i][0])
        flat = [r for i in order for r in frame_results[i]]   # per video in frame order, videos by video_id (results2json_videoseg's input order)
        return eval_utils.video_records(flat) if out_file is None else eval_utils.results2json_videoseg(flat, out_file)
