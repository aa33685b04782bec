"""What the Python half of the planar launch path (stmask_amd/planar.py, the planar wrappers of stmask_amd/ops.py) sends across the C boundary,
recorded on CPU tensors: no kernel runs, every entry point is replaced by a function that writes one canonical line per call.

    trace = run_case(name)          # list of lines
    tests/golden/planar_trace.json.gz  # {case: lines} as the commit BEFORE PlanarConv.__call__ became steps recorded them
                                    # (scripts/make_planar_trace_golden.py, scripts/planar_trace_golden_parent.md)

The module uses only names of stmask_amd that exist in that parent commit too: ops.call / planar.call, ops.conv_set_pixel_gate and the stubs
ops._dev, ops._stream, ops.planar_range_flag, torch.cuda.current_device / current_stream / is_current_stream_capturing -- all patched for the
duration of one trace and restored after it.  (One exception, by getattr: the rule table asks PlanarConv._pick_kernel where the class has it and
restates the parent's expression where it does not.)

A line: the entry name, then every argument.  Integers as they are, floats by repr; a struct as Name{field=value,...} and a ctypes array as
[...], both WITHOUT their zero fields / trailing zeros (a field that is not written is 0); a pointer as @label:bytes+offset -- the storage it
points into (label = index of its first appearance in the trace), that storage's size and the byte offset -- or `null`.  The recorder keeps every
storage it has labelled alive until the trace ends, so an address is never reused and a label is an identity: a launch that reads the wrong
buffer changes its line.  A pointer into no live tensor is an error of the trace.  Launch arguments do not depend on tensor values (nothing
computes them), so inputs are torch.empty and thresholds arbitrary."""
import bisect
import contextlib
import ctypes
import gc

import torch

from stmask_amd import _lib, fuse, ops, planar
from stmask_amd._lib import StmError, c_p
from stmask_amd.config import get_cfg
from stmask_amd.model import STMask
from stmask_amd.planar import PlanarConv
from stmask_amd import synthetic


class TraceError(AssertionError):
    pass


class Recorder:
    def __init__(self, record=True):
        self.record = record          # False: count the calls only (host-cost timing: scripts/make_planar_trace_golden.py --time)
        self.lines, self.n_calls = [], 0
        self.bases, self.spans = [], {}      # sorted storage addresses; address -> (bytes, storage kept alive)
        self.labels = {}

    # ---- pointers -------------------------------------------------------------------------------------------------------------------
    def _find(self, ptr):
        i = bisect.bisect_right(self.bases, ptr) - 1
        if i >= 0:
            base = self.bases[i]
            if ptr < base + max(self.spans[base][0], 1):
                return base
        return None

    def _scan(self, objs):
        for o in objs:
            if type(o) is torch.Tensor or type(o) is torch.nn.Parameter:
                try:
                    st = o.untyped_storage()
                    base, n = st.data_ptr(), st.nbytes()
                except Exception:      # (tensors without storage)
                    continue
                if base and base not in self.spans:
                    self.spans[base] = (n, st)
                    bisect.insort(self.bases, base)

    def pointer(self, ptr):
        if not ptr:
            return "null"
        base = self._find(ptr)
        for gen in (0, 1, 2):           # a tensor made since the last look is among the young objects, as a rule
            if base is not None:
                break
            self._scan(gc.get_objects(generation=gen))
            base = self._find(ptr)
        if base is None:
            raise TraceError(f"pointer {ptr:#x} of call {self.n_calls} points into no live tensor")
        label = self.labels.setdefault(base, len(self.labels))
        return f"@{label}:{self.spans[base][0]}+{ptr - base}"

    # ---- values ---------------------------------------------------------------------------------------------------------------------
    def _array(self, a):
        if issubclass(a._type_, ctypes.Structure):
            return "[" + ",".join(self._struct(s) for s in a) + "]"
        if a._type_ is ctypes.c_void_p:
            return "[" + ",".join(self.pointer(v) for v in a) + "]"
        vals = [repr(v) for v in a]
        while vals and vals[-1] in ("0", "0.0"):
            vals.pop()
        return "[" + ",".join(vals) + "]"

    def _struct(self, s):
        out = []
        for name, _ in s._fields_:
            v = getattr(s, name)
            txt = self._array(v) if isinstance(v, ctypes.Array) else repr(v)
            if txt not in ("0", "0.0", "[]"):
                out.append(f"{name}={txt}")
        return type(s).__name__ + "{" + ",".join(out) + "}"

    def _arg(self, kind, v):
        if kind != "p":
            return repr(float(v)) if kind in "fd" else str(int(v))
        if v is None:
            return "null"
        if isinstance(v, ctypes.Array):
            return self._array(v)
        if isinstance(v, ctypes.c_void_p):
            return self.pointer(v.value)
        if isinstance(v, int):
            return self.pointer(v)
        obj = getattr(v, "_obj", None)          # ctypes.byref(struct)
        if isinstance(obj, ctypes.Structure):
            return self._struct(obj)
        raise TraceError(f"argument {v!r} of call {self.n_calls}")

    # ---- the two functions that stand in for the library --------------------------------------------------------------------------
    def call(self, name, *args):
        self.n_calls += 1
        if not self.record:
            return
        kinds = _lib.all_signatures()[name][1]
        if len(args) != len(kinds):
            raise StmError(f"{name} takes {len(kinds)} arguments, got {len(args)}")
        self.lines.append(name + " " + " ".join(self._arg(k, v) for k, v in zip(kinds, args)))

    def set_pixel_gate(self, ctl, index):
        self.n_calls += 1
        if self.record:
            self.lines.append(f"conv_set_pixel_gate {self.pointer(ctl.data_ptr())} [{int(index)}]")


class _Stream:
    cuda_stream = 0

    def wait_stream(self, other):
        pass


@contextlib.contextmanager
def tracing(rec, kxr_rule=None, **constants):
    """The library replaced by `rec`, the six stubs in place, and planar's module constants `constants` set -- all restored on the way out.
    kxr_rule: the pixel count PlanarConv.kxr_rule_pixels answers with (0 brings the kx-reuse kernel to the small frames of the cases).
    Scratch buffers come from a store of the trace's own (ops.workspace_scope), so that no case sees what another one grew."""
    patches = [(ops, "call", rec.call), (planar, "call", rec.call), (ops, "conv_set_pixel_gate", rec.set_pixel_gate),
               (ops, "_dev", lambda *ts: None), (ops, "_stream", lambda: c_p(0)), (ops, "planar_range_flag", lambda: None),
               (torch.cuda, "current_device", lambda: 0), (torch.cuda, "current_stream", lambda *a: _Stream()),
               (torch.cuda, "is_current_stream_capturing", lambda: False)] + [(planar, k, v) for k, v in constants.items()]
    if kxr_rule is not None:
        patches.append((PlanarConv, "kxr_rule_pixels", lambda self: kxr_rule))
    saved = [(mod, name, getattr(mod, name)) for mod, name, _ in patches]
    fmt = (planar.FMT, planar.BACKBONE_FMT)
    for mod, name, new in patches:
        setattr(mod, name, new)
    try:
        with ops.workspace_scope({}), torch.no_grad():
            yield rec
    finally:
        for mod, name, old in saved:
            setattr(mod, name, old)
        planar.FMT, planar.BACKBONE_FMT = fmt


def attempt(rec, fn):
    """fn(); an error the layer raises becomes a line: type and message."""
    try:
        fn()
    except StmError as e:
        rec.lines.append(f"raise {type(e).__name__}: {e}")


# ---- nets ------------------------------------------------------------------------------------------------------------------------------------
R50, ADA, ALI, R101 = ("STMask_plus_resnet50_config", "STMask_plus_resnet50_ada_config", "STMask_plus_resnet50_ali_config",
                       "STMask_plus_base_config")
FRAMES = (2, 3, 96, 160)


def build_net(cfg_name, planes):
    """The folded net with its planar graph in the plane format `planes`, built anew for every case: weights are packed when a layer first runs,
    so a case's trace holds its packing calls whichever cases ran before it.  (Built under the tracing stubs: building sends nothing across the
    boundary, but it asks the library which layers its kernels take.)"""
    net = STMask(get_cfg(cfg_name))
    net.eval()
    synthetic.fill_state_dict(net, seed=0)
    with tracing(Recorder()):
        fuse.optimize_for_inference(net, planar=True, planes=planes)
    return net


def forward_case(cfg_name, planes, sparse=None, net=None, **constants):
    """net: one built before (host-cost timing: a pass then packs nothing after the first)."""
    def run(rec, net=net):
        net = net or build_net(cfg_name, planes)
        with tracing(rec, **constants):
            planar.set_format(0 if planes == "bf16x3" else 1, backbone_fmt=2 if planes == "fp16x1" else None)
            pg = net._planar
            pg.sparse = sparse
            try:
                attempt(rec, lambda: net.forward_single(torch.empty(*FRAMES)))
            finally:
                pg.sparse = None
    return run


def temporal_case(n, **constants):
    def run(rec):
        tn = build_net(R50, "fp16x2")._planar_temporal
        with tracing(rec, **constants):
            planar.set_format(1)
            xp = torch.empty(2, tn.cpad // 32, n * 49, 32, dtype=torch.float16)
            attempt(rec, lambda: tn.forward_planes(xp, n))
    return run


# ---- direct calls ------------------------------------------------------------------------------------------------------------------------------
def conv(O, C, k=3, stride=1, padding=None, fmt=1, seed=0, bias=True, **kw):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(O, C, k, k, generator=g) * 0.05
    return PlanarConv(w, torch.randn(O, generator=g) if bias else None, stride, k // 2 if padding is None else padding, fmt=fmt, **kw)


def planes(S, N, fmt=1, P=None):
    NP, dt = ops.plane_layout(fmt)
    return torch.empty(NP if P is None else P, S, N, 32, dtype=dt)


def _ctl():
    return torch.empty(64, dtype=torch.int32)


def direct(fn):
    def run(rec):
        with tracing(rec):
            planar.set_format(1)
            attempt(rec, fn)
    return run


def _kxr_side(kxr, delta, groups=1):
    """A layer the kx-reuse kernel takes, at one pixel below (delta = 1) or at (0) its threshold, with the override `kxr`."""
    def fn():
        c = conv(16 * groups, 64, groups=groups, group_cout=[16] * groups if groups > 1 else None)
        assert c.kxr
        M = 2 * 12 * 20
        c.kxr_min_pixels = M + delta
        c(planes(2 * groups, M), ("img", 2, 12, 20), out="f32", kxr=kxr)
    return fn


def _windows9(h=7, w=7):
    wins = [win for _, win in planar.border_windows(h, w)]
    packed = [torch.empty(_lib.lib().stm_conv_packed_weight_bytes_tiled(128, 64, kh, kw, 2, 128), dtype=torch.uint8) for kh, kw, *_ in wins]
    return wins, packed


def _segments(bad=None, groups=1):
    """PlanarConv.window_segments as the sparse head's shapes form calls it: three segments of 9 x 9 patches -> windows of the 7 x 7 maps."""
    def fn():
        c = conv(128 * groups, 64, padding=0, groups=groups, stride=2 if bad == "stride" else 1)
        B, S0, S1 = 6, 9, 7
        w1 = [(5, 5, 1, 1), (7, 5, 0, 1), (5, 7, 1, 0)]
        xp = planes(4, B * S0 * S0 + (0 if bad != "fit" else -1))
        out = planes(8, B * S1 * S1 - (1 if bad == "out" else 0))
        c.window_segments(xp, B, S0, S0, w1, out, S1, (_ctl(), 19), x_ch_off=64 - 32 * groups, out_slab_off=4 - 2 * groups)
    return fn


def _direct_cases():
    img = ("img", 2, 12, 20)
    M = 2 * 12 * 20
    d = {}
    d["plain_planes"] = lambda: conv(64, 64)(planes(2, M), img)
    d["plain_f32_bf16x3"] = lambda: conv(64, 64, fmt=0)(planes(2, M, fmt=0), img, out="f32")
    d["plain_fp16x1_to_fp16x2"] = lambda: conv(64, 64, fmt=2, out_fmt=1)(planes(2, M, fmt=2), img, out="both")
    d["stride2"] = lambda: conv(128, 64, stride=2)(planes(2, M), img, out="both")
    d["levels"] = lambda: conv(256, 64)(planes(2, 2 * (12 * 20 + 6 * 10 + 3 * 5)), ("levels", 2, [(12, 20), (6, 10), (3, 5)]), out="f32")
    # the second source: 64 channels at the output's size + 32 channels of 12 x 20 images read at stride 2
    d["x2"] = lambda: conv(64, 96, k=1)(planes(2, 2 * 6 * 10), ("img", 2, 6, 10), x2=(planes(1, M), 12, 20, 2))
    d["x2_residual_both"] = lambda: conv(64, 96, k=1)(planes(2, 2 * 6 * 10), ("img", 2, 6, 10), out="both", x2=(planes(1, M), 12, 20, 2),
                                                      residual=torch.empty(2 * 6 * 10, 64))
    d["residual_f32"] = lambda: conv(64, 64)(planes(2, M), img, residual=torch.empty(M, 64))
    d["residual_planes"] = lambda: conv(64, 64)(planes(2, M), img, out="f32", residual=planes(2, M))
    d["out_both_given"] = lambda: conv(64, 64)(planes(2, M), img, out="both", out_planes=planes(6, M + 100), out_f32=torch.empty(M + 100, 192),
                                               out_off=100, out_ch_off=64, out_slab_off=3)
    d["out_planes_given"] = lambda: conv(64, 64)(planes(2, M), img, out_planes=planes(2, 2 * M), out_off=M)
    d["x_off_x_ch_off"] = lambda: conv(64, 64)(planes(5, M + 77), img, out="f32", x_off=77, x_ch_off=96)
    d["window_general"] = lambda: conv(64, 64, padding=0)(planes(2, 4 * 81), ("img", 4, 9, 9), out_planes=planes(2, 4 * 49),
                                                           window=(1, 2, 5, 4, -1, -2, 7, 7))
    d["window_general_f32"] = lambda: conv(64, 64, padding=0)(planes(2, 4 * 81), ("img", 4, 9, 9), out="f32", out_f32=torch.empty(4 * 49, 64),
                                                               window=(0, 0, 7, 7, 0, 0, 7, 7), gate=(_ctl(), 3))
    d["window_one_pixel_kxr"] = lambda: conv(16, 64)(planes(2, 4 * 25), ("img", 4, 5, 5), out="f32", out_f32=torch.empty(4, 16),
                                                      window=(0, 0, 1, 1, -1, -1, 1, 1), gate=(_ctl(), 7), kxr=True)
    d["window_one_pixel_general"] = lambda: conv(128, 64)(planes(4, 4 * 25), ("img", 4, 5, 5), out="f32", out_f32=torch.empty(4, 128), x_ch_off=64,
                                                           window=(0, 0, 1, 1, -1, -1, 1, 1), gate=(_ctl(), 15), kxr=False)
    d["gate"] = lambda: conv(64, 64)(planes(2, M), img, gate=(_ctl(), 5))
    d["gate_splitk_off"] = lambda: conv(64, 64)(planes(2, M), img, gate=(_ctl(), 5), splitk=False)
    d["splitk_off"] = lambda: conv(64, 64)(planes(2, M), img, splitk=False)
    d["gate_kxr"] = lambda: conv(16, 64)(planes(2, M), img, out="f32", gate=(_ctl(), 4), kxr=True)
    for kxr in (None, True, False):
        for delta in (0, 1):
            d[f"kxr_{kxr}_{'at' if delta == 0 else 'below'}"] = _kxr_side(kxr, delta)
    d["kxr_grouped_at"] = _kxr_side(None, 0, groups=2)
    d["kxr_residual"] = lambda: conv(16, 64)(planes(2, M), img, out="f32", kxr=True, residual=torch.empty(M, 16))
    d["kxr_twice"] = lambda: [c(planes(2, M), img, out="f32", kxr=True) for c in [conv(16, 64)] * 2]       # packs once
    d["tile_64"] = lambda: conv(256, 64, tile_n=64)(planes(2, M), img)
    d["tile_128"] = lambda: conv(256, 64, tile_n=128)(planes(2, M), img)
    d["tile_both"] = lambda: [c(planes(9, m), ("img", 2, h, 20)) for c in [conv(256, 288)] for h, m in ((12, M), (1400, 56000), (12, M))]
    d["grouped_group_cout"] = lambda: conv(192, 64, groups=3, tile_n=64, group_cout=[41, 5, 32])(planes(8, M), img, out="f32", x_ch_off=64)
    d["grouped_levels_wscale"] = lambda: _wscaled(conv(128, 64, groups=2))(planes(4, 2 * 300), ("levels", 2, [(12, 20), (6, 10)]), out="f32")
    d["window_segments"] = _segments()
    d["window_segments_grouped"] = _segments(groups=2)
    d["ops_conv2d_planar"] = lambda: ops.conv2d_planar(planes(2, M, fmt=0), torch.empty(1000, dtype=torch.uint8), (96, 64, 3, 3), (2, 12, 20),
                                                       torch.empty(96), padding=1, relu=True, out="both")
    d["ops_conv2d_planar_fp16"] = lambda: ops.conv2d_planar(planes(2, M), torch.empty(1000, dtype=torch.uint8), (96, 64, 3, 3), (2, 12, 20), None,
                                                            residual=torch.empty(2 * 6 * 10, 96), stride=2, padding=1, out="f32", tile_n=64, fmt=1,
                                                            out_scale=0.25)
    d["ops_conv2d_planar_residual_planes"] = lambda: ops.conv2d_planar(planes(2, M), torch.empty(1000, dtype=torch.uint8), (96, 64, 1, 1), (2, 12, 20),
                                                                       residual=planes(3, M), fmt=1)

    def windows(out):
        def fn():
            wins, packed = _windows9()
            n = 5
            if out == "pool":
                ops.conv2d_planar_windows_pool(planes(2, n * 49 + 3), packed, wins, torch.empty(128), n, 7, 7, 64, 128, 7, 7, 0.5, torch.empty(8, 128, dtype=torch.int64))
            else:
                ops.conv2d_planar_windows(planes(2, n * 49), packed, wins, None if out == "f32" else torch.empty(128), n, 7, 7, 64, 128, 7, 7, 0.5,
                                          relu=out != "f32", out_f32=torch.empty(n * 49, 128) if out != "planes" else None,
                                          out_planes=planes(4, n * 49) if out != "f32" else None)
        return fn

    for out in ("planes", "f32", "both", "pool"):
        d["ops_windows_" + out] = windows(out)
    # ---- every StmError of these functions, one case each (raise sites no case reaches: UNREACHED below)
    e = {}
    e["planes_dtype"] = lambda: conv(64, 64)(planes(2, M, fmt=0), img)
    e["planes_strided"] = lambda: conv(64, 64)(planes(2, M + 1)[:, :, 1:], img)
    e["channels"] = lambda: conv(64, 64)(planes(2, M), img, x_ch_off=32)
    e["x_ch_off_odd"] = lambda: conv(64, 64)(planes(3, M), img, x_ch_off=16)
    e["levels_not_whole"] = lambda: conv(64, 64)(planes(2, M + 1), ("levels", 2, [(12, 20)]))
    e["window_residual"] = lambda: conv(64, 64)(planes(2, M), img, out_planes=planes(2, M), window=(0, 0, 12, 20, 1, 1, 12, 20), residual=planes(2, M))
    e["input_past_buffer"] = lambda: conv(64, 64)(planes(2, M), img, x_off=1)
    e["window_no_output"] = lambda: conv(64, 64)(planes(2, M), img, window=(0, 0, 12, 20, 1, 1, 12, 20))
    e["window_no_f32_output"] = lambda: conv(64, 64)(planes(2, M), img, out="both", out_planes=planes(2, M), window=(0, 0, 12, 20, 1, 1, 12, 20))
    e["out_slab_past"] = lambda: conv(64, 64)(planes(2, M), img, out_planes=planes(3, M), out_slab_off=2)
    e["residual_one_plane"] = lambda: conv(64, 64)(planes(2, M), img, residual=planes(2, M, P=1))
    e["gate_second_source"] = lambda: conv(64, 96, k=1)(planes(2, 120), ("img", 2, 6, 10), x2=(planes(1, M), 12, 20, 2), gate=(_ctl(), 0))
    e["second_source_levels"] = lambda: conv(64, 96, k=1)(planes(2, 120), ("levels", 2, [(6, 10)]), x2=(planes(1, M), 12, 20, 2))
    e["second_source_dtype"] = lambda: conv(64, 96, k=1)(planes(2, 120), ("img", 2, 6, 10), x2=(planes(1, M, fmt=0), 12, 20, 2))
    e["pack_channels"] = lambda: conv(64, 48, k=1)(planes(2, M), img)
    e["segments_stride"] = _segments("stride")
    e["segments_fit"] = _segments("fit")
    e["segments_out"] = _segments("out")
    e["ops_conv2d_planar_planes"] = lambda: ops.conv2d_planar(planes(2, M, fmt=0), torch.empty(8, dtype=torch.uint8), (96, 64, 3, 3), (2, 12, 20), fmt=1)
    e["ops_conv2d_planar_size"] = lambda: ops.conv2d_planar(planes(2, M), torch.empty(8, dtype=torch.uint8), (96, 96, 3, 3), (2, 12, 20), fmt=1)
    e["ops_conv2d_planar_residual_planes"] = lambda: ops.conv2d_planar(planes(2, M), torch.empty(8, dtype=torch.uint8), (96, 64, 1, 1), (2, 12, 20),
                                                                       residual=planes(2, M), fmt=1)
    e["ops_conv2d_planar_residual_f32"] = lambda: ops.conv2d_planar(planes(2, M), torch.empty(8, dtype=torch.uint8), (96, 64, 1, 1), (2, 12, 20),
                                                                    residual=torch.empty(M, 64), fmt=1)
    e["ops_windows_no_output"] = lambda: ops.conv2d_planar_windows(planes(2, 49), [], [(3, 3, 1, 1, 7, 7, 0, 0)], None, 1, 7, 7, 64, 128, 7, 7, 1.0)
    e["ops_windows_pool_dtype"] = lambda: ops.conv2d_planar_windows_pool(planes(2, 49), [], [(3, 3, 1, 1, 7, 7, 0, 0)], None, 1, 7, 7, 64, 128, 7, 7, 1.0,
                                                                         torch.empty(1, 128, dtype=torch.int32))
    e["set_format"] = lambda: planar.set_format(3)
    e["set_format_backbone"] = lambda: planar.set_format(0, backbone_fmt=2)
    d.update({"error_" + k: v for k, v in e.items()})
    return {"direct_" + k: direct(v) for k, v in d.items()}


def _wscaled(c):
    c.wscale = 4096.0
    return c


# StmError sites of planar.py and of the planar wrappers of ops.py that no case reaches:
UNREACHED = (
    "PlanarGraph._sparse_head (shapes form): 'an output layer's kernel does not fit the patch maps' -- no STMask config has such a head",
    "ops.head_seg_capacity: 'a segment of N entries' -- a capacity of 2^28 entries",
    "ops.head_candidates / head_patch_gather / head_patch_mask / head_assemble_sparse: their shape checks -- the sparse head sizes every tensor itself",
    "ops.head_assemble: 'inputs must be contiguous fp32 matrices' -- likewise",
    "ops.plane_layout: 'unknown planar format' -- set_format refuses the format first",
    "ops.conv_pack_weights_kxr: the library's refusal -- PlanarConv asks conv_kxr_supported before",
    "ops.bottleneck_chain, ops.split_planes, ops.temporal_pool_fc: shape checks -- their callers in planar.py build the shapes they check",
)


# ---- the rule table: tile and kernel choice at the workload's sizes, which CPU tensors cannot hold -----------------------------------------------
def layer_pixels(net, B, H, W):
    """(name, layer, output pixels M, full-size output, residual) of every PlanarConv of the net's graph for B frames of H x W, in launch order."""
    bb, pg = net._planar_backbone, net._planar
    hw = lambda h, w, k, s, p: ops.conv_out_hw(h, w, k, k, s, s, p, p, 1, 1)
    H, W = hw(*hw(H, W, 7, 2, 3), 3, 2, 1)                 # stem convolution, max-pool
    rows, stages = [], []
    for si, blks in enumerate(bb.blocks):
        for bi, e in enumerate(blks):
            sh, sw = e["stride"]
            Ho, Wo = (H - 1) // sh + 1, (W - 1) // sw + 1
            same = (Ho, Wo) == (H, W)
            rows.append((f"layers.{si}.{bi}.c1", e["c1"], B * H * W, True, False))
            for key, full, res in (("c2", same, False), ("om", same, False), ("dcn_conv", True, False), ("ds", same, False), ("c3", True, True),
                                   ("c3ds", True, False)):
                if key in e:
                    rows.append((f"layers.{si}.{bi}.{key}", e[key], B * Ho * Wo, full, res))
            H, W = Ho, Wo
        stages.append((H, W))
    sizes = [stages[i] for i in net.backbone_selected]
    n = pg.n_lat
    for i in range(n):
        h, w = sizes[n - 1 - i]
        rows.append((f"fpn_lat.{i}", pg.fpn_lat[i], B * h * w, True, i > 0))
        rows.append((f"fpn_pred.{i}", pg.fpn_pred[i], B * h * w, True, False))
    for i, dn in enumerate(pg.fpn_down):
        h, w = sizes[-1]
        sizes.append(ops.conv_out_hw(h, w, dn.kh, dn.kw, dn.sh, dn.sw, dn.ph, dn.pw, 1, 1))
        rows.append((f"fpn_down.{i}", dn, B * sizes[-1][0] * sizes[-1][1], sizes[-1] == (h, w), False))
    h, w = sizes[net.proto_src]
    for i, layer in enumerate(pg.proto):
        if isinstance(layer, PlanarConv):
            rows.append((f"proto.{i}", layer, B * h * w, True, False))
        else:
            h, w = h * int(layer.kwargs["scale_factor"]), w * int(layer.kwargs["scale_factor"])
    ntot = B * sum(h * w for h, w in sizes)
    head = [("up", pg.up), ("tower1", pg.tower1), ("tower2", pg.tower2)]
    for k, f in enumerate(pg.finals):
        head += [(f"finals.{k}.{name}", getattr(f, name)) for name in ("small", "trk", "fconv", "adconv") if getattr(f, name) is not None]
    rows += [(name, layer, ntot, True, False) for name, layer in head]
    return rows


def rule_table(rec):
    for cfg_name in (R50, R101):
        net = build_net(cfg_name, "fp16x2")
        for clips in (1, 4, 8, 32):
            seen = set()
            for name, c, M, full, res in layer_pixels(net, clips, 384, 640):
                pick = getattr(c, "_pick_kernel", None)
                if pick is not None:
                    tile = pick(M, full, None, res, None)
                else:       # the parent's expression, PlanarConv.__call__ before the steps
                    use_kxr = c.kxr and not res and full and M >= (c.kxr_min_pixels if c.kxr_min_pixels is not None else c.kxr_rule_pixels())
                    tile = 0 if use_kxr else c.pick_tile(M)
                row = f"C={c.C} O={c.O} k={c.kh}x{c.kw} s={c.sh} groups={c.groups} M={M} full={int(full)} residual={int(res)} pick_tile={c.pick_tile(M)} kernel={tile}"
                if row not in seen:           # (the repeated blocks of a stage: the first one's name stands for all)
                    seen.add(row)
                    rec.lines.append(f"rule {cfg_name} clips={clips} {name} {row}")


# ---- the case list -------------------------------------------------------------------------------------------------------------------------------
THR = 0.3
SPARSE = {"pos": (THR, None), "cap": (THR, 256, False), "center": (THR, 256, True, False), "split": (THR, 256, True, True, False),
          "shapes": (THR, 256, True, True, True)}
CASES = {"forward_r50_fp16x2_dense": forward_case(R50, "fp16x2")}
CASES.update({f"forward_r50_fp16x2_sparse_{k}": forward_case(R50, "fp16x2", sparse=v) for k, v in SPARSE.items()})
# ... and with the kx-reuse kernel and the fused deformable convolution, which the frames of the cases are too small for under the measured rules
CASES["forward_r50_fp16x2_dense_kxr_fused"] = forward_case(R50, "fp16x2", kxr_rule=0, DCN_FUSED_MIN_TILES=1)
CASES.update({f"forward_r50_fp16x2_sparse_{k}_kxr": forward_case(R50, "fp16x2", sparse=SPARSE[k], kxr_rule=0) for k in ("center", "shapes")})
CASES.update({"forward_r50_bf16x3_dense": forward_case(R50, "bf16x3"), "forward_r50_fp16x1_dense": forward_case(R50, "fp16x1")})
for _name, _cfg in (("ada", ADA), ("ali", ALI)):
    CASES[f"forward_{_name}_default"] = forward_case(_cfg, "fp16x2")
    CASES[f"forward_{_name}_fused_min_tiles_1"] = forward_case(_cfg, "fp16x2", DCN_FUSED_MIN_TILES=1)
    CASES[f"forward_{_name}_fcb_module"] = forward_case(_cfg, "fp16x2", FCB_PLANAR=False)
CASES.update({"temporal_n8": temporal_case(8), "temporal_n335_pool": temporal_case(335, TN_POOL=True),
              "temporal_n335_no_pool": temporal_case(335, TN_POOL=False)})
CASES.update(_direct_cases())
CASES["rule_table"] = rule_table


def run_case(name, record=True):
    rec = Recorder(record)
    CASES[name](rec)
    return rec.lines if record else rec.n_calls
