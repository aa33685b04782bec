"""The drop-in boundary: the import shims must not shadow an installed mmcv, the reference's call
sites bind against them, and stmask_amd.model.STMask has the reference STMask()'s state-dict keys and shapes for the four
benchmark configs -- checked against tests/golden/reference_state_dicts.json, the record scripts/check_reference_dropin.py
--write-golden took of the reference's own nets built on the shims.  CPU only."""
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT

SHIMS = os.path.join(ROOT, "stmask_amd", "shims")


def _run(code, extra_path=()):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([SHIMS, ROOT, *extra_path]))
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_shim_extends_an_installed_mmcv_instead_of_shadowing_it(tmp_path):
    pkg = tmp_path / "mmcv"
    (pkg / "parallel").mkdir(parents=True)
    (pkg / "ops").mkdir()
    (pkg / "__init__.py").write_text("from .image import imread\n__version__ = '9.9'\n")
    (pkg / "image.py").write_text("def imread(p): return 'real:' + p\n")
    (pkg / "parallel" / "__init__.py").write_text("class DataContainer: pass\n")
    (pkg / "ops" / "__init__.py").write_text("raise ImportError('CUDA extension missing')\n")
    p = _run("import mmcv, mmcv.ops\nfrom mmcv.parallel import DataContainer\nfrom mmcv.ops import DeformConv2d, roi_align\n"
             "import stmask_amd.mmcv_ops as m\nassert mmcv.__version__ == '9.9' and mmcv.imread('a') == 'real:a'\n"
             "assert DeformConv2d is m.DeformConv2d and roi_align is m.roi_align\nprint('ok')", [str(tmp_path)])
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-1500:]


def test_shim_without_installed_mmcv_pretends_nothing():
    p = _run("import mmcv\nfrom mmcv.ops import DeformConv2d\nassert mmcv.is_str('a') and mmcv.is_list_of([1], int)\n"
             "try:\n    mmcv.imread\nexcept AttributeError as e:\n    print('ok', 'no mmcv package is installed' in str(e))")
    assert p.returncode == 0 and "ok True" in p.stdout, p.stderr[-1500:]


def test_shims_and_state_dicts_match_the_stored_reference_record():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_reference_dropin.py"),
                        "--golden", os.path.join(GOLDEN, "reference_state_dicts.json")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.count("state-dict entries identical") == 4 and "installed package intact" in p.stdout
