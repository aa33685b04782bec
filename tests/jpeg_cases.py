"""The JPEG fixtures (tests/golden/jpeg_cases.npz, written by tests/golden/gen_jpeg_cases.py) and the host program that runs the decoder's
arithmetic on the CPU (tests/jpeg_host_main.cpp), shared by tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np

from stmask_amd import jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Case:
    """name, the file's bytes, PIL's RGB decode (None where PIL refuses the file) and, for a damaged file, `verdict`: how the host program ended
    it under the sanitizers when the fixtures were written -- "flagged <status word>", "equal" (to .rgb), or "refused" (parse refuses the file
    before any kernel sees it)."""

    def __init__(self, name, data, rgb, verdict=None):
        self.name, self.data, self.rgb, self.verdict = name, data, rgb, verdict


@functools.lru_cache(maxsize=None)
def load():
    """-> (grid cases, unsupported cases, damaged cases); the arrays are shared: do not write to them."""
    z = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    names, n_grid, n_whole = [str(n) for n in z["names"]], int(z["n_grid"]), int(z["n_whole"])
    cases = []
    for i, n in enumerate(names):
        rgb = z[f"rgb_{i}"]
        rgb.setflags(write=False)
        cases.append(Case(n, z[f"data_{i}"].tobytes(), rgb if rgb.size else None, str(z[f"verdict_{i}"]) if f"verdict_{i}" in z.files else None))
    return cases[:n_grid], cases[n_grid:n_whole], cases[n_whole:]


def by_name(name):
    return next(c for c in load()[0] if c.name == name)


EDGE_GROUPS = ("narrow", "layout", "tables", "magnitudes", "staging", "extent")


@functools.lru_cache(maxsize=None)
def load_edge():
    """The edge fixtures (tests/golden/jpeg_edge_cases.npz, written by tests/golden/gen_jpeg_edge_cases.py): files PIL's encoder does not
    write, or the grid does not reach, each with PIL's RGB -> [Case]; a name starts with its group, one of EDGE_GROUPS.  Shared: do not write."""
    z = np.load(os.path.join(HERE, "golden", "jpeg_edge_cases.npz"))
    cases = []
    for i, n in enumerate(str(n) for n in z["names"]):
        rgb = z[f"rgb_{i}"]
        rgb.setflags(write=False)
        cases.append(Case(n, z[f"data_{i}"].tobytes(), rgb))
    return cases


def edge_by_name(name):
    return next(c for c in load_edge() if c.name == name)


def damaged():
    """The damaged files: three fixtures cut at 25 %, 50 % and 99 % of their entropy-coded bytes and with one byte inverted at five seeded
    positions -> [Case]; .rgb is PIL's decode of the damaged bytes, or None where PIL refuses them."""
    return load()[2]


def device_damaged():
    """... those of them that parse() takes, so that the kernels see them (a cut that loses restart markers is refused as Malformed before)."""
    out = []
    for c in damaged():
        try:
            jpeg.parse(c.data)
        except ValueError:
            continue
        out.append(c)
    return out


def write_job(path, cases, lenient, order="rgb"):
    """The batch of `cases` as tests/jpeg_host_main.cpp reads it.  lenient: one flag per case (a damaged file: flagged or equal)."""
    batch = jpeg.pack_batch([c.data for c in cases], order, [c.name for c in cases])
    blob = np.zeros(batch.blob_bytes, dtype=np.uint8)
    batch.fill(blob)
    want = np.zeros(batch.out_bytes, dtype=np.uint8)
    for i, c in enumerate(cases):
        if c.rgb is None:
            continue
        px = c.rgb if order == "rgb" else c.rgb[:, :, ::-1]
        o = int(batch.images[i].out_off)
        want[o:o + px.size] = np.ascontiguousarray(px).reshape(-1)
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", batch.n_images, batch.n_segments, batch.images_off, batch.segments_off, batch.blob_bytes, batch.out_bytes,
                            int(order == "bgr"), 0))
        f.write(blob.tobytes())
        f.write(want.tobytes())
        f.write(np.asarray(lenient, dtype=np.int32).tobytes())
    return batch


def sources():
    """A two-video annotation over fixture files, for the dataset tests: 33 x 31 frames of four encodings and 96 x 160 frames with one restart
    interval per MCU row.  -> (annotation dict, path -> BGR pixels as PIL decodes the file (the host reader), path -> CompressedFrame (the device
    reader), {path: Case})."""
    import train_data_cases as C
    files = {f"a/{k}.jpg": by_name(n) for k, n in enumerate(("33x31_444_q90", "33x31_422_q30opt", "33x31_420_q75rst3", "33x31_grey_q90"))}
    files.update({f"b/{k}.jpg": by_name("96x160_420_rstrows1") for k in range(3)})
    vids = [{"id": 1, "height": 31, "width": 33, "length": 4, "file_names": [f"a/{k}.jpg" for k in range(4)]},
            {"id": 2, "height": 160, "width": 96, "length": 3, "file_names": [f"b/{k}.jpg" for k in range(3)]}]
    anns = [C._track(11, 1, 3, 31, 33, [(3.3, 2.2, 10.7, 8.1), (4.1, 2.9, 10.2, 8.4), (5.0, 3.0, 11.0, 9.0), (6.0, 4.0, 11.0, 9.0)]),
            C._track(12, 1, 7, 31, 33, [(18.0, 12.0, 12.5, 9.0), (19.0, 13.0, 12.0, 8.0), None, (20.0, 14.0, 10.0, 8.0)], compressed=True),
            C._track(21, 2, 12, 160, 96, [(10.0, 30.0, 50.0, 80.0), (12.0, 32.0, 50.0, 81.0), (14.0, 34.0, 51.0, 82.0)])]
    ann = {"videos": vids, "categories": [{"id": c, "name": f"c{c}"} for c in C.CAT_IDS], "annotations": anns}
    host = lambda p: np.ascontiguousarray(files[p].rgb[:, :, ::-1])                        # noqa: E731
    return ann, host, lambda p: jpeg.CompressedFrame(files[p].data, name=p), files


CXX = ("g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")     # the last two: the compiler the library is built with


def build_host_program(out_dir, sanitize=True):
    """tests/jpeg_host_main.cpp + csrc/jpeg_core.h -> a stand-alone program, with AddressSanitizer and UBSan when `sanitize`.  The first C++
    compiler of CXX that exists is used; a machine that can build the library has the last ones, so none at all is an error."""
    cxx = next((p for p in (shutil.which(c) for c in CXX) if p), None)
    if cxx is None:
        raise RuntimeError(f"no C++ compiler among {', '.join(CXX)}: the host program cannot be built")
    exe = os.path.join(str(out_dir), "jpeg_host_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, os.path.join(HERE, "jpeg_host_main.cpp"), "-o", exe])
    return exe


def run_host_program(exe, job):
    """-> (exit status, {image index: "equal" | "differs" | "flagged <status>"}, everything it wrote)."""
    r = subprocess.run([exe, str(job)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    lines = {}
    for line in r.stdout.splitlines():
        parts = line.split(None, 1)
        if len(parts) == 2 and parts[0].isdigit():
            lines[int(parts[0])] = parts[1]
    return r.returncode, lines, r.stdout + r.stderr
