"""Trunk scheduling of the batched clip pipeline: forward_single for the frames of a step, eager or replayed from a ring of captured HIP
graphs, with the trunks of the next frames running ahead on side streams.

The trunk does not depend on the tracker (forward_single has no cross-frame dependence), so nothing here reads tracker state:
``TrunkRunner`` is the base of ``pipeline.BatchedClipPipeline``, which asks it for the trunk of a frame (_take_trunk) and tells it
which frames come next (_prefetch_trunk).
"""
import os
import sys
import time

import torch

from . import ops, planar

_SIDE_STREAMS = {}


def concurrent_side_streams(dev, n=2):
    """n streams that really run BESIDE the current stream and beside each other.  HIP maps streams onto a few hardware queues; two streams that land on
    one queue run their work one after the other, silently -- measured: the same pipeline gives 780 frames/s single-stream with two trunk graphs in
    flight, 560 when its side streams happen to share a queue (after another pipeline in the same process had used up some streams of torch's pool) and
    440 when one of them shares the main stream's queue; GPU_MAX_HW_QUEUES only moves the collisions.  So the streams are picked by test, once per
    process and main stream: a 0.5-ms spin kernel on the main stream, on the streams chosen so far and on the candidate -- the candidate is taken when
    all of them finish in the time of one."""
    dev = torch.device(dev)
    main = torch.cuda.current_stream(dev)
    key = (dev.index, main.cuda_stream)
    have = _SIDE_STREAMS.get(key, [])
    if len(have) >= n:
        return have[:n]                              # (the list only grows: the first trunk_stream_count() are the trunk streams, the one after them serves the detection gather)
    cands = [torch.cuda.Stream(device=dev) for _ in range(16)]
    chosen = list(have)
    spin = getattr(torch.cuda, "_sleep", None)
    if spin is not None and not torch.cuda.is_current_stream_capturing():
        cycles = 1_000_000

        def run(streams):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for s_ in streams:
                with torch.cuda.stream(s_):
                    spin(cycles)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        run([main])
        base = min(run([main]) for _ in range(3))
        for c in cands:
            if len(chosen) == n:
                break
            if min(run([main] + chosen + [c]) for _ in range(2)) < 1.4 * base:
                chosen.append(c)
    for c in cands:                                  # (no spin kernel, or fewer independent queues than asked for: any streams will do -- results never depend on it)
        if len(chosen) == n:
            break
        if c not in chosen:
            chosen.append(c)
    _SIDE_STREAMS[key] = chosen
    return chosen[:n]


def trunk_stream_count():
    """How many of concurrent_side_streams()'s streams the pipelines rotate their prefetched trunks over (dist.DetectionGatherer takes the next one)."""
    return max(2, TrunkRunner.PREFETCH_DEPTH)


class TrunkRunner:
    """The trunk of one batch of clips: eager, or from round-robin graph slots; up to prefetch_depth frames ahead on side streams."""

    # Outputs of frame t-1 (previous-frame features of the temporal fusion) and t are live while t+1 .. t+D are produced; a prefetched trunk that is
    # dropped (the caller changed its mind about the next frames) still used up its slot: 2 D + 2 slots cover D prefetched frames with D drops (the
    # slot of frame f is replayed again by the (2 D + 2)-th trunk after it; at most 2 D + 1 start before step f + 1 has read its features).
    # D = trunks in flight ahead of the current frame under graph replay (eager trunks: 1).  Single stream: depth 1 543 frames/s, 2 777, 3 878, 4 793; 8 clips: 1 401 /
    # 1 491 / 1 488 / 1 454 (profiles/r05_trunk_depth2_ab.txt)
    PREFETCH_DEPTH = int(os.environ.get("STM_PREFETCH_DEPTH", "3"))
    N_GRAPH_SLOTS = 2 * PREFETCH_DEPTH + 2
    # Large batches (round 6): a 32-clip trunk fills the GPU by itself, but not at its two ends (the stem and layer1 ramp up, the small FPN levels, P6 / P7 and the head's
    # last launches run on few workgroups) -- two replayed trunks in flight overlap those: 1 599 (eager, one frame ahead) -> 1 587-1 593 (graphs, depth 1) -> 1 630-1 633
    # (depth 2) -> 1 627-1 628 (depth 3) frames/s at 32 clips, same box, alternating.  Above LARGE_BATCH clips the depth is capped at 2 (a slot's private pool is ~10 GB there).
    LARGE_BATCH = 8

    def __init__(self, net, n_clips, timer):
        self.net, self.cfg, self.B = net, net.cfg, n_clips
        self.tf = bool(self.cfg.temporal_fusion_module)
        self.timer = timer          # a pipeline._StageTimer: while it is on, trunks run eagerly and nothing runs ahead
        self._pending = []          # FIFO of (frames, (fpn_outs, pred), event): trunks of the NEXT frame(s), running on the side stream(s)
        self._sides = []            # side streams of the prefetched trunks (two under graph replay: see _prefetch_trunk)
        self._side_next = 0
        self.prefetch_early = True   # start the next trunk at the beginning of step() (measured best at every batch size: +0.5 % at 32 clips, +5.7 % at 8, +13 % at 1);
                                     # False: after the TF convolutions are enqueued (the two big kernel groups then never share the GPU: clean per-kernel timings)
        self.use_graph = False       # replay the trunk (forward_single) from captured HIP graphs: see _trunk_run
        self._graph_sparse = None    # sparse-head setting (threshold, capacity) the slots were captured with: baked into the graphs
        self._sparse_now = None
        self._graph_planes = None    # plane format of the net's inference graph when the slots were captured (a net may serve several pipelines: _trunk_run)
        self._reset_graphs()
        # Sparse head (planar.PlanarGraph._sparse_head, csrc/head_sparse.hip): the bbox / mask / track branches of the shared head run only at
        # the positions with a prior that passes eval_conf_thresh -- the rows the detection stage reads (generate_candidate, TF_utils.py:54-82).
        # Results are the dense head's, bit for bit, at every row that is read.  STM_SPARSE_HEAD=0 keeps the dense head (A/B runs).  The
        # setting (head form, eval_conf_thresh, capacity) is baked into a captured trunk graph: when it changes, the graphs are captured again.
        self.sparse_head = os.environ.get("STM_SPARSE_HEAD", "1") != "0"
        # ... with its output layers at the centre pixel of each position's 5 x 5 patch map only (one-pixel window launches: the other 24 pixels
        # are never read).  STM_HEAD_CENTER=0 runs them over the whole maps (A/B runs); part of the setting baked into the graphs
        self.head_center = planar.head_center_default()
        # ... and its mask / track branches only at the positions with a kept prior of their own: about half the listed positions are there as
        # the centerness partner of a kept prior, and centerness comes out of the bbox branch.  STM_HEAD_SPLIT=0: all three branches at every
        # listed position (A/B runs); part of the setting baked into the graphs
        self.head_split = planar.head_split_default()
        # ... and its patch towers over each entry's own kernel footprint: the list holds (pixel, kernel shape) entries, and shape k's output layers
        # read kh x kw pixels of tower 2.  STM_HEAD_SHAPES=0: the towers over the whole maps of every listed pixel (A/B runs); part of the setting
        self.head_shapes = planar.head_shapes_default()
        # batches from which it is on: a single-stream step is a chain of launches bound by their latency, and the sparse head has 22 more of them
        # (frames/s dense / sparse at 1 clip 812-817 / 713-733, 2 clips 1 073-1 075 / 1 058-1 064, 4 clips 1 301-1 305 / 1 321-1 324, 8 clips
        # 1 435 / 1 543: DESIGN.md section 6).  STM_SPARSE_MIN_CLIPS for A/B runs
        self.sparse_min_clips = int(os.environ.get("STM_SPARSE_MIN_CLIPS", "4"))
        self.sparse_capacity = None  # positions per step the patch launches are sized for (None: PlanarGraph.sparse_capacity; tests set a small one)

    def _reset_graphs(self):
        """No slot captured, eager warm-up ahead: the state before the first capture.  (The caller has emptied _pending and synchronised if trunks
        may still be running on the old slots.)"""
        self._graphs = []            # round-robin slots: (static input, graph, outputs)
        self._graph_ws = []          # per slot: the workspaces its captured graph writes into (kept alive here)
        self._graph_next = 0
        self._graph_warm = 0
        self.graph_active = False

    @property
    def prefetch_depth(self):
        return self.PREFETCH_DEPTH if self.B <= self.LARGE_BATCH else min(self.PREFETCH_DEPTH, 2)

    @property
    def n_graph_slots(self):
        return 2 * self.prefetch_depth + 2

    def _sparse_setting(self, pg):
        """What PlanarGraph.run gets as `sparse` for this pipeline's trunks: Detect_TF with cross-class Fast NMS is the consumer whose reads are known
        to be the kept rows only (ops.detect_cc + ops.gather_detections); every other path keeps the dense head."""
        if not (self.sparse_head and self.B >= self.sparse_min_clips and self.tf and pg is not None and pg.sparse_supported()):
            return None
        if not getattr(self.net.Detect_TF, "use_cross_class_nms", True):
            return None
        return planar.SparseHead(thresh=float(self.cfg.eval_conf_thresh), capacity=self.sparse_capacity, center=self.head_center, split=self.head_split,
                                 # (a capacity given by the caller counts POSITIONS and keeps the list of positions; the segments of entries are sized by the default rule)
                                 shapes=self.head_shapes and self.sparse_capacity is None)

    def _trunk(self, frames):
        pg = getattr(self.net, "_planar", None)
        if pg is None:
            return self._trunk_run(frames)
        self._sparse_now = self._sparse_setting(pg)
        before, pg.sparse = pg.sparse, self._sparse_now
        try:
            return self._trunk_run(frames)
        finally:
            pg.sparse = before

    def _trunk_run(self, frames):
        """forward_single(frames).  With use_graph the ~110 launches of the trunk (every one a Python -> ctypes call: ~25 us of
        host time each, i.e. more than the GPU needs for them at 1-8 clips) are captured once per slot into a HIP graph and
        replayed: one copy of the frames into the slot's static input + one graph launch per step.  Slots in round-robin,
        because a step still reads the previous frame's P4 / T2S while the next frames' trunks are already running on the side
        streams; a slot's outputs stay valid until it is replayed again, N_GRAPH_SLOTS trunks later.  Every slot has its own memory pool
        and its own workspaces: replays may run CONCURRENTLY on different side streams (a single-frame trunk is a chain of ~155 dependent
        small launches -- 1.57 ms of GPU-side launch latency for half that in work; two chains overlap almost completely:
        profiles/r05_two_trunks_probe.txt)."""
        net = self.net
        if not (self.use_graph and getattr(net, "_planar", None) is not None and not self.timer.on and ops._conv_timing is None
                and ops._im2col_timing is None):
            return net.forward_single(frames)
        planes = getattr(net, "_planar_planes", None)
        if self._graphs and (self._graph_planes != planes or self._graph_sparse != self._sparse_now):
            # another pipeline on the same net fell back to bf16x3 planes (BatchedClipPipeline._fall_back swaps the net's inference graph): this
            # pipeline's captured trunks still replay the fp16 graph they were captured from -- drop them (with their private pools) and capture
            # again on the net's current graph
            self._pending = []
            torch.cuda.synchronize()
            self._reset_graphs()
        if self._graph_warm < 2:
            # eager first: packs the weights, sizes the workspaces, fills the prior cache, reserves the kernels' LDS
            self._graph_warm += 1
            return net.forward_single(frames)
        if len(self._graphs) < self.n_graph_slots:
            reserved0 = torch.cuda.memory_reserved(frames.device)
            static_in = frames.clone(memory_format=torch.preserve_format)
            graph = torch.cuda.CUDAGraph()
            ws = {}
            self._graph_ws.append(ws)
            cur = torch.cuda.current_stream()
            cap = torch.cuda.Stream(device=frames.device)
            cap.wait_stream(cur)
            # scratch buffers whose addresses the graph bakes in are owned by this pipeline (ops.workspace_scope), not by the
            # capture stream's slot of the global cache
            with ops.workspace_scope(ws):
                with torch.cuda.stream(cap):
                    net.forward_single(static_in)             # once more on the capture stream: sizes this scope's workspaces
                with torch.cuda.graph(graph, stream=cap):
                    out = net.forward_single(static_in)
            cur.wait_stream(cap)
            if not self._graphs:
                # every slot keeps a private pool the size of a trunk's activations (~8 GB at 32 clips of 384x640): before the ring is built, make sure
                # the other 2 D + 1 slots fit beside what the process holds -- else this pipeline keeps the eager trunk (one frame of look-ahead)
                slot_bytes = max(torch.cuda.memory_reserved(frames.device) - reserved0, 0)
                free = torch.cuda.mem_get_info(frames.device)[0] + torch.cuda.memory_reserved(frames.device) - torch.cuda.memory_allocated(frames.device)
                if (self.n_graph_slots - 1) * slot_bytes > 0.9 * free:
                    sys.stderr.write(f"stmask_amd: {self.n_graph_slots} trunk-graph slots of {slot_bytes / 1e9:.1f} GB do not fit in {free / 1e9:.1f} GB of free HBM: "
                                     "this pipeline keeps the eager trunk\n")
                    del graph, out, static_in
                    self._graph_ws.pop()
                    self.use_graph = False
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    return net.forward_single(frames)
            self._graphs.append((static_in, graph, out))
            self._graph_planes = planes
            self._graph_sparse = self._sparse_now
            self.graph_active = True
        static_in, graph, out = self._graphs[self._graph_next]
        self._graph_next = (self._graph_next + 1) % self.n_graph_slots
        if static_in.shape != frames.shape:
            raise ops.StmError("BatchedClipPipeline: the frame batch changed shape under a captured trunk graph")
        static_in.copy_(frames)
        graph.replay()
        return out

    def _prefetch_trunk(self, next_frames):
        """Enqueue the trunk(s) of the next frame(s) on side streams.  The trunk does not depend on the tracker, and the rest
        of this step is ~200 tiny launches around two host reads (latency-bound: the GPU idles 10-17 % of the step without
        this).  next_frames: the frames of the next call, or a list [next, the one after, ...] -- under graph replay up to PREFETCH_DEPTH of
        them are started (those not in flight yet), rotating over as many side streams, so that the trunk graphs run beside each other and
        beside this step's tracker tail; eager trunks (large batches fill the GPU by themselves) keep one frame of look-ahead.  A side stream
        waits for everything enqueued on the main stream so far."""
        if next_frames is None or self.timer.on:
            return
        nxt = list(next_frames) if isinstance(next_frames, (list, tuple)) else [next_frames]
        depth = self.prefetch_depth if (self.use_graph and self.graph_active) else 1
        main = torch.cuda.current_stream()
        for f in nxt[:depth]:
            if f is None or any(p[0] is f for p in self._pending):
                continue
            if not self._sides:
                self._sides = concurrent_side_streams(f.device, trunk_stream_count())
            side = self._sides[self._side_next]
            self._side_next = (self._side_next + 1) % len(self._sides)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                out = self._trunk(f)
                ev = torch.cuda.Event()
                ev.record()
            self._pending.append((f, out, ev))

    def _take_trunk(self, frames):
        """(fpn_outs, pred) of `frames`: the trunk started for them on a side stream by an earlier step, or a fresh one.  Third value: a
        prefetched trunk of OTHER frames was dropped."""
        net = self.net
        dropped = False
        while self._pending and self._pending[0][0] is not frames:
            torch.cuda.current_stream().wait_event(self._pending.pop(0)[2])   # a trunk nobody asked for: let it finish, drop it
            dropped = True
        if self._pending:
            _, (fpn_outs, pred), ev = self._pending.pop(0)
            torch.cuda.current_stream().wait_event(ev)
            if not self.graph_active:                            # (graph outputs live in the graphs' own pools)
                for t_ in list(pred.values()) + list(fpn_outs):  # allocated on the side stream, consumed on this one
                    if torch.is_tensor(t_):
                        t_.record_stream(torch.cuda.current_stream())
                t2s_ = pred["T2S_feat"][net.correlation_selected_layer] if isinstance(pred.get("T2S_feat"), (list, tuple)) and self.tf else None
                if torch.is_tensor(t2s_):
                    t2s_.record_stream(torch.cuda.current_stream())
        else:
            fpn_outs, pred = self._trunk(frames)
        return fpn_outs, pred, dropped
