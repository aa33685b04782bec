"""Which kernel each case of tests/conv_rows_cases.py launches, asked of the dry run (stm_debug_conv2d_planar_plan) on the CPU, and the claim
tests/test_gpu_conv_rows.py rests on: together with the oracle tests of tests/test_gpu_conv.py, whose shapes the case module holds as data, the
list launches EVERY kernel of the planar convolution -- all 26 rows of PLANAR_ROWS, the window-set entries, both kx-reuse entries and the split-K
finishing kernel.  A change of a threshold in csrc/conv_plan.h that moves a case onto another kernel fails here, before the GPU coverage shrinks."""
import os
import re

import pytest

import conv_plan_cases as cc
import conv_rows_cases as rc
from stmask_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def plan(monkeypatch):
    """plan(case, env) -> [(kernel, splitk)]: the dry run of a conv_plan_cases case under exactly the switches of env."""
    lib = _lib.lib()

    def run(case, env):
        for k in cc.TUNABLES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        lib.stm_debug_reload_tunables()
        return rc.launches(lib, case)

    yield run
    monkeypatch.undo()
    lib.stm_debug_reload_tunables()


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_launches_the_kernel_it_names(name, plan):
    case = rc.CASES[name]
    for res in (case["call"]["res"], None, "f32", "planes"):          # (the residual form is the GPU test's to vary: the plan does not read it)
        assert plan(rc.plan_case(dict(case["call"], res=res)), case["env"]) == case["expect"], (name, res)
    assert set(case["env"]) <= set(cc.TUNABLES)                        # the switches the library already has
    if case["partner"]:
        other = rc.CASES[case["partner"][0]]
        assert other["data"] == case["data"] and case["partner"][1] in ("bitwise", "splitk")
        assert (len(other["expect"]) == 1) and ((len(case["expect"]) == 2) == (case["partner"][1] == "splitk"))


def test_case_list_is_what_the_issue_names():
    """Shapes with a partial last pixel tile; the seven rows by the cases meant for them; every three-product shape on every tile form."""
    by_kernel = {}
    for name, case in rc.CASES.items():
        for kernel, _ in case["expect"]:
            by_kernel.setdefault(kernel, []).append(name)
    for kernel, cases in rc.SEVEN_ROWS.items():
        names = [n for pat in cases.split(", ") for n in rc.CASES if re.fullmatch(pat.replace("*", r"\d+"), n)]
        assert names and sorted(names) == sorted(by_kernel[kernel]), (kernel, names, by_kernel.get(kernel))
    assert len(rc.SEVEN_ROWS) == 7 and set(rc.SEVEN_ROWS) <= set(cc.KERNELS)
    assert sorted(n for n in rc.CASES if n.startswith("three_")) == sorted(f"three_{i}_{t}" for i in range(3) for t in ("t64", "t128_mg1", "t128_mg2"))
    starts = rc.level_starts(rc.HEAD_B, rc.HEAD_SIZES)
    assert starts[-1] == 969 and starts[-1] % 128 == 73 and starts[-1] % 256 == 201
    assert any(s % 128 for s in starts[1:-1])                           # tiles straddle levels


def test_every_kernel_is_compared_with_the_oracle(plan):
    """The union over this list and the oracle tests of tests/test_gpu_conv.py == the kernels of the library."""
    new, old = set(), {}
    for case in rc.CASES.values():
        new |= {k for k, _ in plan(rc.plan_case(case["call"]), case["env"])}
    for test, env, case in rc.existing_launches():
        for k, _ in plan(case, env):
            old.setdefault(k, test)
    elsewhere = set(rc.REACHED_ELSEWHERE)
    unreached = set(cc.KERNELS) - new - set(old) - elsewhere
    assert not unreached, sorted(unreached)
    assert new | set(old) | elsewhere == set(cc.KERNELS) and len(cc.KERNELS) == 31 and len(set(cc.ROWS)) == 26
    # the seven rows, the finishing kernel over groups and levels and the plain kx-reuse entry over levels come from the new list
    assert set(rc.SEVEN_ROWS) <= new and not set(rc.SEVEN_ROWS) & set(old), sorted(set(rc.SEVEN_ROWS) & set(old))
    assert {rc.FINISH, rc.KX3} <= new
    # ... the window-set entries from the window test's shapes, the gated set from the test named for it
    assert {"conv_planar_kernel<2,2,2,1,3,0,0,1>", "conv_planar_kx3_kernel<0,1>"} <= set(old)
    assert not (elsewhere & (new | set(old)))                           # (listed there only because nothing here reaches it)
    for kernel, (module, test) in rc.REACHED_ELSEWHERE.items():
        with open(os.path.join(HERE, module)) as f:
            assert re.search(r"^def %s\(" % test, f.read(), re.M), (kernel, module, test)
