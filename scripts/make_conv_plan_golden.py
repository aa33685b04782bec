"""Writes tests/golden/conv_plan.json: what the launcher did BEFORE its rules moved into csrc/conv_plan.h, for every case of
tests/conv_plan_cases.py.

The library it drives is a build of that earlier commit whose launch sites print one line per launch instead of launching.
scripts/conv_plan_golden_parent.md holds the commit, the complete patch and the build commands.  On any machine (no GPU is used):

    python scripts/make_conv_plan_golden.py /path/to/libstmask_hip_parentplan.so

The library is loaded on its own, not through stmask_amd._lib.lib(): it is an older build and lacks the entries added since.  The public
entries are called with placeholder addresses: nothing on the host reads through them."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from stmask_amd import _lib   # noqa: E402
import conv_plan_cases as cc   # noqa: E402


def run_public(lib, case):
    g = cc.geom(case)
    gp = ctypes.byref(g) if g is not None else None
    lib.stm_conv_set_pixel_gate(case["gate"])
    if case["windows"] is not None:
        wp, wins, n = cc.window_args(case)
        if case["pool"]:
            rc = lib.stm_conv2d_planar_windows_pool_f32(case["x"], wp, wins, n, case["bias"], case["pool"], gp, None)
        else:
            rc = lib.stm_conv2d_planar_windows_f32(case["x"], wp, wins, n, case["bias"], case["out32"], case["outpl"], gp, case["relu"], None)
    elif case["dual"]:
        d = case["dual"]
        rc = lib.stm_conv2d_planar_dual_f32(case["x"], d["x2"], d["C2"], d["H2"], d["W2"], d["s2"], d["np"], d["ps"], case["w"], case["bias"],
                                            case["res32"], case["respl"], case["out32"], case["outpl"], gp, case["relu"], case["ws"],
                                            case["ws_bytes"], None)
    else:
        rc = lib.stm_conv2d_planar_ws_f32(case["x"], case["w"], case["bias"], case["res32"], case["respl"], case["out32"], case["outpl"], gp,
                                          case["relu"], case["ws"], case["ws_bytes"], None)
    lib.stm_conv_set_pixel_gate(None)
    buf = ctypes.create_string_buffer(4096)
    assert lib.stm_dbg_plan_text(buf, len(buf)) < len(buf)
    return rc, buf.value.decode(), (lib.stm_last_error_string().decode() if rc else "")


def load(path):
    """The patched library with the argument types of the entries this script calls (the table of stmask_amd/_lib.py) and of the patch's own entry."""
    lib = ctypes.CDLL(path)
    for name in ("stm_conv2d_planar_ws_f32", "stm_conv2d_planar_dual_f32", "stm_conv2d_planar_windows_f32", "stm_conv2d_planar_windows_pool_f32",
                 "stm_conv_set_pixel_gate", "stm_debug_reload_tunables", "stm_last_error_string"):
        ret, params = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._KINDS[ret], [_lib._KINDS[k] for k in params]
    lib.stm_dbg_plan_text.restype, lib.stm_dbg_plan_text.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]
    return lib


def main():
    lib = load(sys.argv[1])
    golden = {}
    for name, case in cc.CASES.items():
        for k in cc.TUNABLES:
            os.environ.pop(k, None)
        os.environ.update(case["env"])
        lib.stm_debug_reload_tunables()
        rc, text, err = run_public(lib, case)
        golden[name] = {"rc": rc, "text": "" if rc else text, "error": err}
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json"), "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(golden), "cases;", sum(1 for v in golden.values() if v["rc"]), "refused")


if __name__ == "__main__":
    main()
