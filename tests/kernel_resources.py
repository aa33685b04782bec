"""hipcc's resource report (-Rpass-analysis=kernel-resource-usage) for one translation unit of stmask_amd/csrc, compiled device-only with the
flags the library is built with.  The one place the tests spell that command line."""
import collections
import functools
import os
import re
import subprocess

from stmask_amd import _lib

CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]


class Resources(collections.namedtuple("Resources", "vgpr sgpr lds scratch occupancy")):
    """One kernel's row; .spills = (VGPRs Spill, SGPRs Spill) rides along."""


def makefile_flags():
    """csrc/Makefile's HIPFLAGS line without what only the host pass or the link needs."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)$", text, flags=re.M).group(1)
    line = re.search(r"^HIPFLAGS \?= (.*)$", text, flags=re.M).group(1)
    return [f.replace("$(ARCH)", arch) for f in line.split() if f not in ("-fPIC", "-Wall", "-Wno-unused-function")]


@functools.lru_cache(maxsize=None)
def kernel_resources(source):
    """{kernel name as the report prints it (mangled): Resources} of csrc/<source>; compiled once per session."""
    assert FLAGS == makefile_flags(), (FLAGS, makefile_flags())
    cmd = [HIPCC, *FLAGS, "--cuda-device-only", "-c", os.path.join(CSRC, source), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    rows = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", out)[1:]:
        field = lambda name: int(re.search(re.escape(name) + r": (\d+)", b).group(1))          # noqa: E731
        row = Resources(field(" VGPRs"), field("TotalSGPRs"), field("LDS Size [bytes/block]"), field("ScratchSize [bytes/lane]"),
                        field("Occupancy [waves/SIMD]"))
        row.spills = (field("VGPRs Spill"), field("SGPRs Spill"))
        rows[b.split()[0]] = row
    assert rows, out[-2000:]
    return rows
