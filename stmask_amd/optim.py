"""GuardedSGD: the reference's optim.SGD(lr, momentum, weight_decay) (train.py:181) as one fused pass of csrc/optim.hip per 64 tensors, with the
reference's `if torch.isfinite(loss).item(): optimizer.step()` (train.py:314-316) moved into the kernel: every workgroup reads the loss (and, with
guard="grads", a flag a first pass over the gradients sets) and leaves parameters and momentum untouched when it is not finite.  step() never waits
for the device; counters() is the one host read.  Per element, in IEEE fp32, unfused:  g' = g + wd * p;  m = mu * m + g';  p = p - lr * m, with
momentum buffers that start as zeros (mu * 0 + g' == g': torch's first step, also when the guard skipped the first steps).  There is no CPU
fallback: step() on CPU parameters raises StmError."""
import ctypes

import torch

from . import _lib
from ._lib import StmError, c_p

MAX_TENSORS = _lib.DP_MAX_TENSORS    # csrc/optim.h STM_OPTIM_MAX_TENSORS: tensors per launch (the table travels in the kernel arguments)
CHUNK = _lib.DP_CHUNK                # csrc/optim.h STM_OPTIM_CHUNK: elements per workgroup
GUARDS = ("loss", "grads", None)


def _dense(t):
    """Every element of the storage span is an element of t exactly once (contiguous in some dimension order)."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda x: x[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def _layout(t):
    """The strides that place elements (a dimension of size 1 has none)."""
    return tuple(st for s, st in zip(t.shape, t.stride()) if s != 1)


def _raw_stream():
    return c_p(torch.cuda.current_stream().cuda_stream)


class GuardedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, guard="loss"):
        if guard not in GUARDS:
            raise ValueError(f"GuardedSGD: guard={guard!r}, expected 'loss', 'grads' or None")
        for name, v in (("lr", lr), ("momentum", momentum), ("weight_decay", weight_decay)):
            if not (isinstance(v, (int, float)) and v == v and abs(v) != float("inf")) or v < 0:
                raise ValueError(f"GuardedSGD: {name}={v!r} must be a finite number >= 0")
        # torch.optim.SGD's group keys, so that a state dict goes either way; the last six are fixed
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False, foreach=None,
                                      differentiable=False, fused=None))
        self.guard = guard
        devices = set()
        for i, p in enumerate(self._all_params()):
            if p.dtype != torch.float32:
                raise ValueError(f"GuardedSGD: parameter {i} is {p.dtype}, the step is written for float32")
            if not _dense(p):
                raise ValueError(f"GuardedSGD: parameter {i} (shape {tuple(p.shape)}, strides {p.stride()}) is not dense")
            devices.add(p.device)
        if len(devices) > 1:
            raise ValueError(f"GuardedSGD: parameters on {sorted(map(str, devices))}, one device is needed")
        self.device = devices.pop() if devices else torch.device("cpu")
        self._counters = self._bad = None
        self._checked = {}      # parameter -> the momentum buffer _check has seen with it

    def _all_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for key in ("dampening", "nesterov", "maximize"):     # a torch SGD group handed over as it is
            if self.param_groups[-1].get(key):
                raise ValueError(f"GuardedSGD: {key}={self.param_groups[-1][key]!r} is not built (dampening 0, no Nesterov term, minimize)")

    # ---- device state ------------------------------------------------------------------------------------------------------------
    @property
    def counters_tensor(self):
        """int32 [2] on the parameters' device: steps applied, steps skipped by the guard."""
        if self._counters is None:
            self._counters = torch.zeros(2, dtype=torch.int32, device=self.device)
        return self._counters

    def counters(self):
        """(applied, skipped) as Python ints: the one place that reads the device."""
        a, s = self.counters_tensor.tolist()
        return a, s

    def set_counters(self, applied, skipped):
        """What checkpoint.load restores, so that a resumed run goes on counting."""
        self.counters_tensor.copy_(torch.tensor([int(applied), int(skipped)], dtype=torch.int32))

    # ---- the step ----------------------------------------------------------------------------------------------------------------
    def _loss_ptr(self, loss):
        if loss is None:
            if self.guard == "loss":
                raise ValueError("GuardedSGD.step: guard='loss' needs the loss (a 0-dim or [1] float32 device tensor)")
            return None
        if not (isinstance(loss, torch.Tensor) and loss.dtype == torch.float32 and loss.numel() == 1 and loss.dim() <= 1 and loss.device == self.device):
            what = f"{tuple(loss.shape)} {loss.dtype} on {loss.device}" if isinstance(loss, torch.Tensor) else type(loss).__name__
            raise ValueError(f"GuardedSGD.step: loss must be a 0-dim or [1] float32 tensor on {self.device}, got {what}")
        return c_p(loss.data_ptr())

    @staticmethod
    def _check(i, p, g, m):
        if g.dtype != torch.float32 or g.is_sparse or g.device != p.device or m.dtype != torch.float32 or m.device != p.device:
            raise ValueError(f"GuardedSGD.step: parameter {i}: gradient ({g.dtype}, {g.device}) and momentum buffer ({m.dtype}, {m.device}) "
                             f"must be dense float32 tensors on {p.device}")
        if not (g.shape == p.shape == m.shape and _layout(g) == _layout(p) == _layout(m) and _dense(p)):
            raise ValueError(f"GuardedSGD.step: parameter {i}: data {tuple(p.shape)}/{p.stride()}, gradient {tuple(g.shape)}/{g.stride()} and "
                             f"momentum buffer {tuple(m.shape)}/{m.stride()} must share one dense layout")

    @torch.no_grad()
    def step(self, loss=None, closure=None):
        """One update of every parameter that has a gradient; no host synchronisation.  loss: see `guard`."""
        if closure is not None or callable(loss):
            raise ValueError("GuardedSGD.step: a closure is not supported (the loss is passed as a tensor)")
        if self.device.type != "cuda":
            raise StmError("GuardedSGD.step: the parameters are on the CPU; the step is a HIP kernel for the MI355X and there is no CPU fallback")
        loss_ptr = self._loss_ptr(loss) if self.guard is not None else None
        groups, index = [], 0
        for group in self.param_groups:
            rows = []
            for p in group["params"]:
                i, index = index, index + 1
                g = p.grad
                if g is None:
                    continue
                state = self.state[p]
                m = state.get("momentum_buffer")
                if m is None:
                    m = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                # torch itself keeps a gradient at its parameter's dtype, size and device; what is left to look at in every step is the layout, and a
                # buffer is looked at in full when it is first seen (a loaded state dict may hold anything)
                if not (self._checked.get(p) is m and not g.is_sparse and p.is_contiguous() and g.is_contiguous() and m.is_contiguous()):
                    self._check(i, p, g, m)
                    self._checked[p] = m
                rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel()))
            if rows:
                groups.append((group, rows))
        if not groups:
            return None
        counters = c_p(self.counters_tensor.data_ptr())
        bad_ptr = None
        with torch.cuda.device(self.device):
            stream = _raw_stream()
            if self.guard == "grads":
                if self._bad is None:
                    self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
                bad_ptr = c_p(self._bad.data_ptr())
                first = 1
                for _, rows in groups:
                    for k in range(0, len(rows), MAX_TENSORS):
                        part = rows[k:k + MAX_TENSORS]
                        _lib.private_call("stm_grads_nonfinite_multi_f32", (c_p * len(part))(*[r[1] for r in part]),
                                          (ctypes.c_int64 * len(part))(*[r[3] for r in part]), len(part), bad_ptr, first, stream)
                        first = 0
            first = 1
            for group, rows in groups:
                lr, mu, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
                for k in range(0, len(rows), MAX_TENSORS):
                    part = rows[k:k + MAX_TENSORS]
                    n = len(part)
                    _lib.private_call("stm_sgd_step_multi_f32", (c_p * n)(*[r[0] for r in part]), (c_p * n)(*[r[1] for r in part]),
                                      (c_p * n)(*[r[2] for r in part]), (ctypes.c_int64 * n)(*[r[3] for r in part]), n, loss_ptr, bad_ptr, counters,
                                      first, lr, mu, wd, stream)
                    first = 0
        return None

    # ---- state dicts: torch.optim.SGD's layout -------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """Takes GuardedSGD's own and torch.optim.SGD's state dict: a missing or None momentum buffer becomes zeros at the next step, group keys
        this class does not know are dropped; dampening != 0, nesterov and maximize are refused."""
        groups = []
        for gi, group in enumerate(state_dict["param_groups"]):
            if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
                raise ValueError(f"GuardedSGD.load_state_dict: group {gi} has dampening={group.get('dampening', 0)} nesterov={group.get('nesterov', False)} "
                                 f"maximize={group.get('maximize', False)}; the step is built for dampening 0, no Nesterov term, minimize")
            groups.append({**self.defaults, **{k: v for k, v in group.items() if k == "params" or k in self.defaults}})
        state = {}
        for k, v in state_dict.get("state", {}).items():
            if v.get("momentum_buffer") is not None:
                state[k] = {"momentum_buffer": v["momentum_buffer"]}
        super().load_state_dict({"state": state, "param_groups": groups})


class DataParallelSGD(GuardedSGD):
    """GuardedSGD for one rank of a data-parallel run (stmask_amd.parallel): the same arguments and validation, plus world and rank.  It owns two
    parallel.GradArena of one layout over the trainable parameters: `grads` (every p.grad is a view of its segment, so autograd accumulates in
    place; the tail carries the loss) and `momentum` (its views are the momentum_buffer entries of the state, in torch.optim.SGD's layout, so a
    checkpoint keeps its format and loads either way).  Between backward and step(), parallel.exchange(opt.grads) sums the arena over the ranks.
    step() is then dp_sgd_finish_multi_kernel of csrc/optim.hip: per element  g = s * inv_world;  g' = g + wd * p;  m = mu * m + g';  p = p - lr * m  with s the summed
    gradient and inv_world the fp32 value of 1 / world, and 0.0f written back over every gradient element -- also when the guard skips the step,
    so zero_grad() has nothing left to do and a NaN never survives into the next iteration.  The guard reads the reduced tail slot 0 (the sum of
    the ranks' losses; not finite as soon as one rank's is) and, with guard="grads", a flag that one pass of stm_grads_nonfinite_multi_f32 over
    the reduced arena sets: functions of the reduced buffer alone, so every rank decides alike and the weights cannot drift apart.
    One difference from GuardedSGD: every trainable parameter steps in every applied iteration, with g = 0 when no gradient reached it, so weight
    decay and momentum still act on it (as under torch's DistributedDataParallel, whose buckets are zero-filled)."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, guard="loss", world=1, rank=0, n_tail=8):
        super().__init__(params, lr, momentum=momentum, weight_decay=weight_decay, guard=guard)
        if not (isinstance(world, int) and isinstance(rank, int) and world >= 1 and 0 <= rank < world):
            raise ValueError(f"DataParallelSGD: world={world!r} rank={rank!r}")
        if n_tail < 1:
            raise ValueError(f"DataParallelSGD: n_tail={n_tail}, slot 0 carries the loss")
        from .parallel import GradArena
        import numpy as np
        self.world, self.rank = world, rank
        self.inv_world = float(np.float32(1.0) / np.float32(world))
        self.trainable = [p for p in self._all_params() if p.requires_grad]
        self.grads = GradArena(self.trainable, n_tail, self.device)
        self.momentum = GradArena(self.trainable, 0, self.device)
        self.grads.bind_grads()
        for p, m in zip(self.trainable, self.momentum.views):
            self.state[p]["momentum_buffer"] = m
        self._tables = None      # (the parameters' addresses, [(group, [ctypes arrays and count per launch])])

    def zero_grad(self, set_to_none=True):
        """Nothing: the finish kernel has cleared the arena, and the views stay bound."""

    def _build_tables(self, ptrs):
        slot = {id(p): i for i, p in enumerate(self.trainable)}
        out = []
        for group in self.param_groups:
            rows = [slot[id(p)] for p in group["params"] if id(p) in slot]
            launches = []
            for k in range(0, len(rows), MAX_TENSORS):
                part = rows[k:k + MAX_TENSORS]
                n = len(part)
                launches.append(((c_p * n)(*[ptrs[i] for i in part]), (c_p * n)(*[self.grads.views[i].data_ptr() for i in part]),
                                 (c_p * n)(*[self.momentum.views[i].data_ptr() for i in part]),
                                 (ctypes.c_int64 * n)(*[self.trainable[i].numel() for i in part]), n))
            if launches:
                out.append((group, launches))
        return out

    @torch.no_grad()
    def step(self, loss=None, closure=None):
        """The finish of one iteration, after parallel.exchange(self.grads); no host synchronisation.  The loss is not an argument: it travels in
        the arena's tail (train.train_step_dp writes it)."""
        if closure is not None or loss is not None:
            raise ValueError("DataParallelSGD.step: takes no loss and no closure (the loss travels in the tail of the gradient arena: "
                             "train.train_step_dp)")
        if self.device.type != "cuda":
            raise StmError("DataParallelSGD.step: the parameters are on the CPU; the step is a HIP kernel for the MI355X and there is no CPU fallback")
        for i, (p, g, m) in enumerate(zip(self.trainable, self.grads.views, self.momentum.views)):
            if p.grad is not g or self.state[p].get("momentum_buffer") is not m:
                raise ValueError(f"DataParallelSGD.step: trainable parameter {i}: its gradient or momentum buffer is no longer the arena's view "
                                 "(zero the gradients through this optimizer, not with set_to_none on the module)")
        ptrs = [p.data_ptr() for p in self.trainable]
        if self._tables is None or self._tables[0] != ptrs:
            for i, p in enumerate(self.trainable):
                if not (_dense(p) and _layout(p) == _layout(self.grads.views[i])):
                    raise ValueError(f"DataParallelSGD.step: trainable parameter {i} changed its layout since the arena was laid out")
            self._tables = (ptrs, self._build_tables(ptrs))
        counters = c_p(self.counters_tensor.data_ptr())
        loss_ptr = c_p(self.grads.tail.data_ptr()) if self.guard is not None else None
        bad_ptr = None
        with torch.cuda.device(self.device):
            stream = _raw_stream()
            if self.guard == "grads":
                if self._bad is None:
                    self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
                bad_ptr = c_p(self._bad.data_ptr())
                flat = self.grads.flat
                _lib.private_call("stm_grads_nonfinite_multi_f32", (c_p * 1)(flat.data_ptr()), (ctypes.c_int64 * 1)(flat.numel()), 1, bad_ptr, 1,
                                  stream)
            first = 1
            for group, launches in self._tables[1]:
                lr, mu, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
                for p_arr, g_arr, m_arr, n_arr, n in launches:
                    _lib.private_call("stm_dp_sgd_finish_multi_f32", p_arr, g_arr, m_arr, n_arr, n, loss_ptr, bad_ptr, counters, first,
                                      self.inv_world, lr, mu, wd, stream)
                    first = 0
        return None

    # ---- state dicts: torch.optim.SGD's layout -------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.SGD's layout; the momentum buffers are copies (a saved view would carry the whole arena's storage)."""
        sd = super().state_dict()
        sd["state"] = {k: {"momentum_buffer": v["momentum_buffer"].clone()} for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Takes its own, GuardedSGD's and torch.optim.SGD's state dict: the momentum is copied into the arena (a missing or None buffer: zeros),
        group keys this class does not know are dropped; dampening != 0, nesterov and maximize are refused."""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("DataParallelSGD.load_state_dict: the state dict's parameter groups do not match this optimizer's")
        for gi, group in enumerate(saved):
            if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
                raise ValueError(f"DataParallelSGD.load_state_dict: group {gi} has dampening={group.get('dampening', 0)} "
                                 f"nesterov={group.get('nesterov', False)} maximize={group.get('maximize', False)}; the step is built for "
                                 "dampening 0, no Nesterov term, minimize")
        state = state_dict.get("state", {})
        view = {id(p): m for p, m in zip(self.trainable, self.momentum.views)}
        with torch.no_grad():
            for group, mine in zip(saved, self.param_groups):
                mine.update({k: v for k, v in group.items() if k != "params" and k in self.defaults})
                for key, p in zip(group["params"], mine["params"]):
                    m = view.get(id(p))
                    if m is None:
                        continue
                    got = (state.get(key) or {}).get("momentum_buffer")
                    if got is None:
                        m.zero_()
                    elif got.shape != m.shape:
                        raise ValueError(f"DataParallelSGD.load_state_dict: momentum buffer {key} is {tuple(got.shape)}, the parameter "
                                         f"{tuple(m.shape)}")
                    else:
                        m.copy_(got)
