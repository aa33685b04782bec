"""Data-parallel training, one process per GPU: what the reference's CustomDataParallel(NetLoss(net, criterion)) (train.py:153-175, :226, :310)
computes -- every rank evaluates the criterion on its share of the batch, the loss terms and the gradient are the mean over the ranks -- with
identical weights on every rank and ONE collective per step.

GradArena is one flat fp32 buffer: a segment per trainable parameter, in parameter order, each starting on a 16-byte boundary (the pads are zero
and stay zero), then a tail of n_tail floats.  Every p.grad is a view of its segment (the parameter's shape and dense layout), so autograd
accumulates in place and nothing is packed or unpacked.  The tail rides in the same buffer and so in the same collective: slot 0 the rank's total
loss (the guard of optim.DataParallelSGD reads its sum), slots 1.. the loss terms in the criterion's key order (the log reads their mean).
exchange() is that collective: one sum all-reduce over the whole buffer.  The finish kernel of csrc/optim.hip then averages, steps and writes
zeros back over the gradients (optim.DataParallelSGD.step).

Not built: overlap of the all-reduce with the backward pass (buckets, post-accumulate hooks), multi-GPU validation, more than one node."""
import torch
import torch.distributed as dist

ALIGN = 4      # floats: every segment (and the tail) starts on a 16-byte boundary


def _span_dense(t):
    """Every element of the storage span is an element of t exactly once (contiguous in some dimension order)."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda x: x[1]):
        if stride != expect:
            return False
        expect *= size
    return True


class GradArena:
    """flat: float32 [total]; offsets[i], numels[i]: the segment of params[i]; views[i]: flat's elements offsets[i] .. + numels[i] in the shape
    and strides of params[i]; tail: flat[tail_offset : tail_offset + n_tail].  total = tail_offset + n_tail."""

    def __init__(self, params, n_tail=8, device=None):
        self.params = list(params)
        if n_tail < 0:
            raise ValueError(f"GradArena: n_tail={n_tail}")
        self.offsets, self.numels, at = [], [], 0
        for i, p in enumerate(self.params):
            if p.dtype != torch.float32 or not _span_dense(p):
                raise ValueError(f"GradArena: parameter {i} ({p.dtype}, shape {tuple(p.shape)}, strides {p.stride()}) must be dense float32")
            self.offsets.append(at)
            self.numels.append(p.numel())
            at += -(-p.numel() // ALIGN) * ALIGN
        self.tail_offset, self.n_tail = at, int(n_tail)
        if device is None:
            device = self.params[0].device if self.params else torch.device("cpu")
        self.flat = torch.zeros(at + self.n_tail, dtype=torch.float32, device=device)
        self.views = [self.flat.as_strided(p.shape, p.stride(), off) for p, off in zip(self.params, self.offsets)]
        self.tail = self.flat[at:at + self.n_tail]

    def segment(self, i):
        """The 1-d stretch of flat that holds parameter i (without its pad)."""
        return self.flat[self.offsets[i]:self.offsets[i] + self.numels[i]]

    def pads(self):
        """The padding elements, concatenated (all zero, always)."""
        ends = self.offsets[1:] + [self.tail_offset]
        parts = [self.flat[off + n:end] for off, n, end in zip(self.offsets, self.numels, ends)]
        return torch.cat(parts) if parts else self.flat[:0]

    def bind_grads(self):
        """p.grad = the view of its segment, for every parameter."""
        for p, v in zip(self.params, self.views):
            p.grad = v

    def write_tail(self, values):
        """Overwrites the first len(values) tail slots with the 0-dim tensors `values`: one stack and one small device copy, never accumulated."""
        if len(values) > self.n_tail:
            raise ValueError(f"GradArena.write_tail: {len(values)} values, the tail holds {self.n_tail}")
        self.tail[:len(values)].copy_(torch.stack([v.detach().reshape(()).to(torch.float32) for v in values]))


def world_size(group=None):
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def exchange(arena, group=None):
    """The step's one collective: a sum all-reduce over the whole buffer, tail included, in place.  Backend nccl (RCCL): on the device, ordered
    with the current stream.  Backend gloo with a device arena: staged through the host, as dist.all_gather_detections does (the form of the CPU
    tests and of two ranks on one GPU).  A world of one: nothing."""
    if world_size(group) == 1:
        return
    flat = arena.flat
    if flat.is_cuda and dist.get_backend(group) == "gloo":
        host = flat.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        flat.copy_(host, non_blocking=True)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)


def checksums(tensors):
    """int64 [len(tensors)] on the tensors' device: per tensor the sum of its elements' bit patterns (4-byte types as int32, others as values)."""
    out = []
    for t in tensors:
        t = t.detach().contiguous()
        t = t.view(torch.int32) if t.element_size() == 4 else t
        out.append(t.to(torch.int64).sum())
    return torch.stack(out) if out else torch.zeros(0, dtype=torch.int64)


def _host_collective(fn, t, group):
    """fn(tensor) on t itself, or on a host copy when gloo is handed a device tensor -> the tensor that holds the result."""
    if t.is_cuda and dist.get_backend(group) == "gloo":
        h = t.cpu()
        fn(h)
        return h
    fn(t)
    return t


def broadcast_from_rank0(tensors, group=None):
    """Rank 0's values into every tensor of every rank, in place."""
    if world_size(group) == 1:
        return
    for t in tensors:
        d = t.detach()
        got = _host_collective(lambda x: dist.broadcast(x, 0, group=group), d, group)
        if got is not d:
            d.copy_(got)


def first_difference(tensors, group=None):
    """One all-reduce (MAX over [c, -c] of the per-tensor checksums c): the index of the first tensor whose checksum differs between ranks, or
    None when every rank holds the same."""
    if world_size(group) == 1:
        return None
    c = checksums(tensors)
    both = torch.cat([c, -c])
    both = _host_collective(lambda x: dist.all_reduce(x, op=dist.ReduceOp.MAX, group=group), both, group)
    hi, lo = both[:len(c)], -both[len(c):]
    differ = (hi != lo).nonzero().flatten().tolist()
    return differ[0] if differ else None


class DataParallelTrainer:
    """net_loss (train.NetLoss) and an optim.DataParallelSGD over its parameters, made ready for train.train_step_dp: construction broadcasts the
    parameters and buffers from rank 0 and verifies with one all-reduced checksum comparison that every rank holds the same bytes."""

    def __init__(self, net_loss, optimizer, group=None):
        self.net_loss, self.optimizer, self.group = net_loss, optimizer, group
        named = list(net_loss.named_parameters()) + list(net_loss.named_buffers())
        tensors = [t for _, t in named]
        broadcast_from_rank0(tensors, group)
        bad = first_difference(tensors, group)
        if bad is not None:
            raise RuntimeError(f"DataParallelTrainer: {named[bad][0]} differs between the ranks after the broadcast from rank 0")

    def step(self, batch, loss_log=None):
        from .train import train_step_dp
        return train_step_dp(self.net_loss, self.optimizer, batch, loss_log, group=self.group)
