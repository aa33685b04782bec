#!/usr/bin/env python3
"""optim.GuardedSGD (csrc/optim.hip: one fused, guarded pass) against torch.optim.SGD followed by the reference's host check
`if torch.isfinite(loss).item()` (train.py:314-316):  python scripts/bench_sgd_step.py [--out profiles/bench_sgd_step.txt]

(a) the step alone on the parameter shapes of R50 FCA and R50 ada with seeded gradients: device time (HIP events around 20 steps queued while a
    spin kernel holds the device, so the host's share is not in it; for torch's side the step without the check), wall-clock per step, device
    launches of one step seen by torch.profiler, host synchronisations of one step seen by torch's sync debug mode, and the bytes the step has to
    move (counted from the passes: 20 per element fused, +4 with the gradient check; torch's foreach form makes four passes of 12 + 8 + 12 + 12)
    over the measured device time.
(b) train.train_step at 384x640 with 2 clips, max_pos=4096 (no host read in the criterion): GuardedSGD, torch.optim.SGD as train_step runs it
    (no check at all), and torch.optim.SGD behind the reference's check; wall-clock per iteration over 20 iterations after warm-up.

All sides run in one process on one card and alternate within each of 5 groups; the median of the groups is reported with the slowest group beside
it.  torch's optimizer in the same run is the baseline, never an earlier file."""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import layers, synthetic  # noqa: E402
from stmask_amd.config import get_cfg  # noqa: E402
from stmask_amd.model import STMask  # noqa: E402
from stmask_amd.optim import GuardedSGD  # noqa: E402
from stmask_amd.train import NetLoss, train_step  # noqa: E402

DEV = "cuda:0"
CONFIGS = (("STMask_plus_resnet50_config", "r50_fca"), ("STMask_plus_resnet50_ada_config", "r50_ada"))
SGD = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)


_SPIN = {}


def hold_device(seconds):
    """Keep the device busy for about `seconds` with torch's spin kernel, so that what the host queues meanwhile runs back to back afterwards and two
    events around it measure the device alone (a step whose host side is slower than its kernels would otherwise time the host).  False without
    the spin kernel."""
    spin = getattr(torch.cuda, "_sleep", None)
    if spin is None:
        return False
    if "per_cycle" not in _SPIN:
        for cycles in (1_000_000, 20_000_000):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spin(cycles)
            torch.cuda.synchronize()
            _SPIN["per_cycle"] = (time.perf_counter() - t0) / cycles
    spin(int(seconds / _SPIN["per_cycle"]))
    return True


def alternating(fns, reps, groups=5, warm=3, device_fns=None):
    """{name: (median, slowest) over the groups} of the wall-clock microseconds of one call (`reps` calls between two synchronisations) and, for the
    names of device_fns, of the device microseconds of one call of that function: HIP events around `reps` calls queued behind hold_device().
    Within a group every side is timed once, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    dev, wall = {k: [] for k in (device_fns or {})}, {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e6 / reps)
            if k in dev:
                held = hold_device(1.5 * wall[k][-1] * 1e-6 * reps)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    device_fns[k]()
                e1.record()
                e1.synchronize()
                dev[k].append(e0.elapsed_time(e1) * 1000.0 / reps if held else float("nan"))
    stat = lambda per: {k: (statistics.median(v), max(v)) for k, v in per.items()}      # noqa: E731
    return stat(dev), stat(wall)


def device_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return str(n) if n else "not measured"
    except Exception as exc:  # noqa: BLE001  (a measuring aid: the timings do not depend on it)
        return f"not measured ({type(exc).__name__})"


def host_syncs(fn):
    """Synchronising calls torch reports for one fn() (sync debug mode "warn")."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in seen if "called a synchronizing" in str(w.message))


def param_shapes(name):
    return [tuple(p.shape) for p in STMask(get_cfg(name)).parameters()]


def step_alone(emit):
    emit("(a) the optimizer step alone, seeded gradients; microseconds, median of 5 alternating groups (slowest group); GB/s = counted bytes / device time")
    emit(f"{'config':>8} {'side':>26} {'tensors':>8} {'Melem':>7} {'device us':>19} {'wall us':>19} {'launches':>9} {'host syncs':>11} {'MB moved':>9} {'GB/s':>7}")
    verdict = []
    for name, tag in CONFIGS:
        shapes = param_shapes(name)
        n_elem = sum(int(torch.Size(s).numel()) for s in shapes)
        gen = torch.Generator().manual_seed(0)
        loss = torch.tensor(1.0, device=DEV)

        def make():
            ps = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.05).to(DEV)) for s in shapes]
            for p in ps:
                p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(DEV)
            return ps

        sides = {}
        for label, guard in (("GuardedSGD guard=loss", "loss"), ("GuardedSGD guard=grads", "grads")):
            opt = GuardedSGD(make(), guard=guard, **SGD)
            sides[label] = (lambda o: lambda: o.step(loss))(opt)
        ref = torch.optim.SGD(make(), **SGD)

        def reference():
            if torch.isfinite(loss).item():
                ref.step()

        sides["torch SGD + isfinite.item"] = reference
        # the device time of the reference side is that of torch's step alone: its check waits for the device by design
        dev, wall = alternating(sides, reps=20, device_fns=dict(sides, **{"torch SGD + isfinite.item": ref.step}))
        bytes_of = {"GuardedSGD guard=loss": 20 * n_elem, "GuardedSGD guard=grads": 24 * n_elem, "torch SGD + isfinite.item": 44 * n_elem}
        for label, fn in sides.items():
            emit(f"{tag:>8} {label:>26} {len(shapes):>8} {n_elem / 1e6:>7.1f} {dev[label][0]:>9.1f} ({dev[label][1]:>7.1f}) "
                 f"{wall[label][0]:>9.1f} ({wall[label][1]:>7.1f}) {device_launches(fn):>9} {host_syncs(fn):>11} {bytes_of[label] / 1e6:>9.1f} "
                 f"{bytes_of[label] / dev[label][0] / 1e3:>7.0f}")
        verdict.append((tag, dev["GuardedSGD guard=loss"][0], dev["torch SGD + isfinite.item"][0]))
        del sides, ref
        torch.cuda.empty_cache()
    return verdict


def whole_step(emit):
    emit("")
    emit("(b) train.train_step, 384x640, 2 clips, max_pos=4096, SGD(lr 1e-3, momentum 0.9, weight decay 1e-4); wall-clock milliseconds per iteration "
         "over 20 iterations, median of 5 alternating groups (slowest group)")
    emit(f"{'config':>8} {'GuardedSGD guard=loss':>24} {'torch SGD, no check':>24} {'torch SGD + isfinite.item':>27} {'reference loop / guarded':>25}")
    verdict = []
    for name, tag in CONFIGS:
        cfg = get_cfg(name)
        net = STMask(cfg)
        synthetic.fill_state_dict(net, seed=0)
        net = net.to(DEV).train()
        nl = NetLoss(net, layers.MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3, max_pos=4096))
        batch = synthetic.synthetic_train_batch(2, 384, 640, seed=0, device=DEV)
        # lr 0: the three sides share one net, and the timing must not depend on where the weights have wandered; the kernels do the same work
        guarded = GuardedSGD(net.parameters(), **dict(SGD, lr=0.0))
        plain = torch.optim.SGD(net.parameters(), **dict(SGD, lr=0.0))

        def reference_loop():                                           # reference train.py:305-316
            plain.zero_grad()
            losses = nl(*batch)
            loss = sum(losses.values())
            loss.backward()
            if torch.isfinite(loss).item():
                plain.step()

        sides = {"guarded": lambda: train_step(nl, guarded, batch), "plain": lambda: train_step(nl, plain, batch), "reference": reference_loop}
        _, wall = alternating(sides, reps=20, warm=3)
        cell = lambda k: f"{wall[k][0] / 1e3:>9.2f} ({wall[k][1] / 1e3:>7.2f})"      # noqa: E731
        emit(f"{tag:>8} {cell('guarded'):>24} {cell('plain'):>24} {cell('reference'):>27} {wall['reference'][0] / wall['guarded'][0]:>25.3f}")
        verdict.append((tag, wall["guarded"][0], wall["reference"][0]))
        del net, nl, guarded, plain, sides
        torch.cuda.empty_cache()
    return verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_sgd_step.txt"))
    ap.add_argument("--skip_train_step", action="store_true", help="part (a) only")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"bench_sgd_step.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    a = step_alone(emit)
    b = [] if args.skip_train_step else whole_step(emit)
    emit("")
    for tag, ours, theirs in a:
        emit(f"{tag}: the fused step alone takes {ours / theirs:.2f} of torch's device time" + (" -- SLOWER than torch's" if ours > theirs else ""))
    for tag, ours, theirs in b:
        emit(f"{tag}: an iteration with GuardedSGD takes {ours / theirs:.3f} of the reference loop's wall-clock")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
