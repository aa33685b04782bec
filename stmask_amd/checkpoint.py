"""Checkpoints of a training run under the reference's file names (utils/functions.py:96-160, SavePath): {name}_{epoch}_{iteration}.pth, and
{name}_{epoch}_{iteration}_interrupt.pth for the file written when a run is interrupted.  The .pth is net.save_weights(): a plain state dict, the
file the reference's load_weights reads.  Next to it lies PATH.state, which the reference does not have: the optimizer's state dict (torch
SGD's layout), the iteration and epoch, the guard's counters and the loader's position, so that a resumed run continues bit for bit.  Without the
sidecar, load() does what the reference's --resume does: weights only, the iteration from the file name, momentum from zero.
Every file is written under a temporary name in its folder and renamed: an interrupted save leaves the previous file as it was."""
import glob
import os

import torch

STATE_SUFFIX = ".state"
INTERRUPT = "_interrupt"


def save_path(name, epoch, iteration, root="", interrupt=False):
    return os.path.join(root, f"{name}_{epoch}_{iteration}{INTERRUPT if interrupt else ''}.pth")


def parse_path(path):
    """-> (name, epoch, iteration) of a file name save_path made, with or without the _interrupt suffix; ValueError for any other name."""
    stem = os.path.basename(path)
    if stem.endswith(".pth"):
        stem = stem[:-len(".pth")]
    if stem.endswith(INTERRUPT):
        stem = stem[:-len(INTERRUPT)]
    parts = stem.rsplit("_", 2)
    if len(parts) != 3 or not parts[0]:
        raise ValueError(f"{path}: not NAME_EPOCH_ITERATION[.pth]")
    return parts[0], int(parts[1]), int(parts[2])


def get_latest(folder, name):
    """The .pth of `name` in `folder` with the largest iteration (interrupt files count, as in the reference), or None."""
    best, best_iter = None, -1
    for path in sorted(glob.glob(os.path.join(glob.escape(folder), glob.escape(name) + "_*.pth"))):
        try:
            got, _, iteration = parse_path(path)
        except ValueError:
            continue
        if got == name and iteration > best_iter:
            best, best_iter = path, iteration
    return best


def get_interrupt(folder):
    found = sorted(glob.glob(os.path.join(glob.escape(folder), "*" + INTERRUPT + ".pth")))
    return found[0] if found else None


def remove(path):
    """A checkpoint and its sidecar."""
    for p in (path, path + STATE_SUFFIX):
        if os.path.exists(p):
            os.remove(p)


def remove_interrupt(folder):
    for path in glob.glob(os.path.join(glob.escape(folder), "*" + INTERRUPT + ".pth")):
        remove(path)


def _atomic(path, write):
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        write(tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save(path, net, optimizer=None, iteration=0, epoch=0, loader=None):
    """The weights to `path`, everything else a run needs to continue to path + ".state".  Reads the device (the weights, the counters): call it
    between steps, not inside one."""
    _atomic(path, net.save_weights)
    state = {"iteration": int(iteration), "epoch": int(epoch)}
    if optimizer is not None:
        state["optimizer"] = optimizer.state_dict()
        if hasattr(optimizer, "counters"):
            state["counters"] = tuple(optimizer.counters())
    if loader is not None:
        state["loader"] = loader.state()
    _atomic(path + STATE_SUFFIX, lambda tmp: torch.save(state, tmp))


def load(path, net, optimizer=None, loader=None):
    """Restores what the files hold -> {"iteration", "epoch", "sidecar": bool}.  The optimizer and the loader are left as they are when there is
    no sidecar (or it lacks their part)."""
    net.load_weights(path)
    if not os.path.exists(path + STATE_SUFFIX):
        _, epoch, iteration = parse_path(path)
        return {"iteration": iteration, "epoch": epoch, "sidecar": False}
    state = torch.load(path + STATE_SUFFIX, map_location="cpu")
    if optimizer is not None and "optimizer" in state:
        optimizer.load_state_dict(state["optimizer"])
        if "counters" in state and hasattr(optimizer, "set_counters"):
            optimizer.set_counters(*state["counters"])
    if loader is not None and "loader" in state:
        loader.load_state(state["loader"])
    return {"iteration": state["iteration"], "epoch": state["epoch"], "sidecar": True}
