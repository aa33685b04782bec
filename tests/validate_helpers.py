"""What tests/test_validate_cpu.py and tests/test_gpu_validate.py share: seeded perturbation of a live net, snapshots compared as raw bytes, a
freshly optimised copy (the yardstick of InferenceTwin.refresh), and a three-video validation split with an in-memory frame reader."""
import copy
import os
import random
import re
import threading

import numpy as np
import torch

from stmask_amd import fuse

LENGTHS, SIZES = (3, 5, 2), ((24, 40), (18, 30), (24, 40))


def raw(t):
    """A tensor's bytes (bit-for-bit comparison, NaN included)."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def perturb(net, seed):
    """Seeded noise on every parameter and every BatchNorm statistic (variances stay positive)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in list(net.named_parameters()) + list(net.named_buffers()):
            if not t.is_floating_point():
                t.add_(1)
                continue
            noise = torch.randn(t.shape, generator=g).to(t.device)
            if name.endswith("running_var"):
                t.mul_(1.0 + 0.05 * noise.abs())
            else:                               # 2 % of the tensor's scale: the activations keep their size, every bit of every tensor moves
                t.add_(noise * (0.02 * float(t.abs().mean()) + 1e-3))


def snapshot(net):
    """(state dict as bytes, training flags, requires_grad flags)."""
    return ({k: raw(v) for k, v in net.state_dict().items()}, {n: m.training for n, m in net.named_modules()},
            {n: p.requires_grad for n, p in net.named_parameters()})


def same_snapshot(a, b):
    return a[1] == b[1] and a[2] == b[2] and a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0])


def full_state(net):
    """state_dict() and the non-persistent buffers (bias3), as bytes."""
    out = dict(net.state_dict())
    out.update({k: v for k, v in net.named_buffers() if k not in out})
    return {k: raw(v) for k, v in out.items()}


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


def fresh_copy(net, planar=False, planes="fp16x2"):
    """What exists without the twin: a deepcopy taken through optimize_for_inference."""
    c = copy.deepcopy(net)
    c.eval()
    fuse.optimize_for_inference(c, planar=planar, planes=planes)
    return c


def rng_states(cuda=False):
    return (torch.get_rng_state().clone(), np.random.get_state(), random.getstate(), torch.cuda.get_rng_state().clone() if cuda else None)


def same_rng(a, b):
    return (torch.equal(a[0], b[0]) and a[2] == b[2] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:] and
            (a[3] is None or torch.equal(a[3], b[3])))


def val_ann(annotations=None, sizes=SIZES):
    """Three videos of lengths 3, 5 and 2 in two source sizes; `annotations`: None leaves the key out (the official valid split)."""
    videos = [dict(id=10 + i, height=h, width=w, length=T, file_names=[f"v{i}/{t:05d}.jpg" for t in range(T)])
              for i, (T, (h, w)) in enumerate(zip(LENGTHS, sizes))]
    ann = dict(videos=videos, categories=[dict(id=c, name=f"c{c}") for c in range(1, 41)])
    if annotations is not None:
        ann["annotations"] = annotations
    return ann


class Reader:
    """An in-memory frame_reader that counts the reads of every file (from any thread).  Without `frames`, frame t of video i is filled with
    10 i + t; with frames = {(i, t): uint8 [H, W, 3] array} it hands those out."""

    def __init__(self, wrong=None, frames=None, sizes=SIZES):
        self.reads, self.wrong, self.frames, self.sizes, self.lock = {}, wrong, frames, sizes, threading.Lock()

    def __call__(self, path):
        with self.lock:
            self.reads[path] = self.reads.get(path, 0) + 1
        i, t = int(re.search(r"v(\d+)/", path).group(1)), int(os.path.basename(path).split(".")[0])
        if self.frames is not None:
            return self.frames[(i, t)]
        h, w = self.sizes[i]
        if path == self.wrong:
            h += 1
        return np.full((h, w, 3), 10 * i + t, dtype=np.uint8)
