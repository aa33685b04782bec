"""Host cost of one call through the ctypes binding, declared signatures against per-call casts.  No GPU: every call below returns before it
touches a device.

The library is opened twice in one process: `new` is stmask_amd._lib.lib() (restype / argtypes set from the tables of _lib.HEADERS, plain Python arguments),
`old` a bare ctypes.CDLL handle used the way the package used it before the table existed (no argtypes, every scalar wrapped at the call site).
  query   stm_conv_kxr_tile_pixels(3, 1, 4): a 3-argument pure function
  refuse  stm_ohem_conf_loss_f32 with C = 1: 14 arguments, refused with STM_EUNSUPPORTED (-5) from the shapes alone
  status  stm_encode_boxes_f32 with n = 0 (returns 0 before it looks at a pointer) through the whole idiom of a call site:
          _lib.call(name, ...) against check(old_lib().name(...), name), old_lib() standing in for the lib() lookup every call site made
Each figure is ns per call over `--calls` calls, median and range of `--repeats` repeats.
Usage: python scripts/bench_binding_calls.py [--calls 100000] [--repeats 5]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stmask_amd import _lib  # noqa: E402
from stmask_amd._lib import c_i, c_l, c_p, c_sz, call, check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    new, old, c_d = _lib.lib(), ctypes.CDLL(_lib.LIB_PATH), ctypes.c_double
    name = "stm_encode_boxes_f32"

    def old_lib():
        return old

    def null():
        return c_p(0)                    # a pointer argument as ops._p builds it, in both styles

    cases = [
        ("query", lambda: old.stm_conv_kxr_tile_pixels(c_i(3), c_i(1), c_i(4)), lambda: new.stm_conv_kxr_tile_pixels(3, 1, 4)),
        ("refuse", lambda: old.stm_ohem_conf_loss_f32(null(), null(), null(), null(), null(), c_i(2), c_i(300), c_i(1), c_i(3), c_d(1.0), c_i(0), null(),
                                                      c_sz(0), null()),
         lambda: new.stm_ohem_conf_loss_f32(null(), null(), null(), null(), null(), 2, 300, 1, 3, 1.0, 0, null(), 0, null())),
        ("status", lambda: check(old_lib().stm_encode_boxes_f32(null(), null(), null(), c_l(0), null()), name), lambda: call(name, null(), null(), null(), 0, null())),
    ]
    assert cases[0][1]() == cases[0][2]() > 0 and cases[1][1]() == cases[1][2]() == -5
    print(f"{args.calls} calls x {args.repeats} repeats, ns per call: median (min .. max)")
    for what, f_old, f_new in cases:
        ns = {"old": [], "new": []}
        for _ in range(args.repeats):
            for key, f in (("old", f_old), ("new", f_new)):          # alternate, so that a drifting clock hits both
                t0 = time.perf_counter_ns()
                for _ in range(args.calls):
                    f()
                ns[key].append((time.perf_counter_ns() - t0) / args.calls)
        for key in ("old", "new"):
            print(f"  {what:7s} {key}  {statistics.median(ns[key]):8.1f}  ({min(ns[key]):.1f} .. {max(ns[key]):.1f})")


if __name__ == "__main__":
    main()
