"""What is about include/stmask_hip_eval.h (video mask AP on the device) alone: its limits against vis_eval.py and what its entries refuse without
a device.  tests/test_abi.py compares the header with _lib.EVAL_SIGNATURES, as it does for every header."""
import re

import pytest

from abi_header import header_raw
from stmask_amd import _lib


def test_header_limits_match_the_python_side():
    from stmask_amd import vis_eval
    defines = dict(re.findall(r"^#define (STM_VIS_[A-Z_]+) (\d+)", header_raw("stmask_hip_eval.h"), flags=re.M))
    assert int(defines["STM_VIS_MAX_DET"]) == vis_eval.MAX_DET == vis_eval.MAX_DETS[-1] == 100
    assert int(defines["STM_VIS_MAX_GT"]) == vis_eval.MAX_GT
    assert int(defines["STM_VIS_MAX_THREADS"]) >= len(vis_eval.IOU_THRS) * len(vis_eval.AREA_RNG) == 40
    assert (int(defines["STM_VIS_RLE_UNTERMINATED"]), int(defines["STM_VIS_RLE_RANGE"]), int(defines["STM_VIS_RLE_SUM"])) == (
        vis_eval.RLE_UNTERMINATED, vis_eval.RLE_RANGE, vis_eval.RLE_SUM)


def test_call_checks_the_eval_entries_without_a_device():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_vis_rle_decode", None, None)                        # argument count
    n3, n4 = [None] * 3, [None] * 4
    # sizes refused before any pointer is looked at, NULL pointers before any launch
    for n, total in ([-1, 0], [1, -1], [1, 2 ** 31]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_vis_rle_decode", *n3, n, total, *n4, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_vis_rle_decode", *n3, 2, 10, *n4, None)
    assert "NULL" in str(e.value)
    with pytest.raises(_lib.StmError):
        _lib.call("stm_vis_rle_check", *n3, -1, 0, *n3, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_vis_rle_check", *n3, 2, 10, *n3, None)
    assert "NULL" in str(e.value)
    for n_pairs, n_tracks, frames, n_masks in ([-1, 0, 0, 0], [2 ** 31, 1, 1, 1], [1, -1, 0, 0], [1, 0, -1, 0], [1, 0, 0, -1]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_vis_tube_iou", None, None, n_pairs, None, None, n_tracks, frames, *n4, n_masks, *n3, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_vis_tube_iou", None, None, 3, None, None, 2, 2, *n4, 4, *n3, None)
    assert "NULL" in str(e.value)

    def match(n_groups, max_d, max_g, n_thr, n_area):
        _lib.call("stm_vis_match", *n4, n_groups, max_d, max_g, *n4, n_thr, None, n_area, *n3, None)

    for bad in ([-1, 1, 1, 10, 4], [1, 101, 1, 10, 4], [1, 1, 1025, 10, 4], [1, -1, 1, 10, 4], [1, 1, -1, 10, 4], [1, 1, 1, 0, 4], [1, 1, 1, 10, 0],
                [1, 1, 1, 13, 5]):
        with pytest.raises(_lib.StmError):
            match(*bad)
    with pytest.raises(_lib.StmError) as e:
        match(1, 101, 1, 10, 4)
    assert "101" in str(e.value) and "100" in str(e.value)
    with pytest.raises(_lib.StmError) as e:
        match(2, 100, 1024, 10, 4)
    assert "NULL" in str(e.value)
    # nothing to do launches nothing: no device, no pointers, no error
    _lib.call("stm_vis_rle_decode", *n3, 0, 0, *n4, None)
    _lib.call("stm_vis_rle_check", *n3, 0, 0, *n3, None)
    _lib.call("stm_vis_tube_iou", None, None, 0, None, None, 0, 0, *n4, 0, *n3, None)
    match(0, 0, 0, 10, 4)
