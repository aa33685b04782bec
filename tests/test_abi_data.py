"""What is about include/stmask_hip_data.h (training batches on the device) alone: what its entries refuse without a device.  tests/test_abi.py
compares the header with _lib.DATA_SIGNATURES and its structs with their mirrors, as it does for every header."""
import ctypes

import pytest

from stmask_amd import _lib


def test_call_checks_the_data_entries_without_a_device():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_data_masks_u8", None, None)                         # argument count
    n3, n4, n5 = [None] * 3, [None] * 4, [None] * 5
    # sizes refused before any pointer is looked at, NULL pointers before any launch
    for n, h, w, Hp, Wp in ([-1, 24, 40, 32, 64], [1, 0, 40, 32, 64], [1, 24, 40, 16, 64], [1, 24, 40, 32, 32]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_data_frames_u8_f32", None, n, None, h, w, Hp, Wp, None, None, 1, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_data_masks_u8", *n3, 1, None, n, 0, None, h, w, Hp, Wp, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_data_boxes_f32", None, None, n, None, h, w, Hp, Wp, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_data_masks_u8", *n3, 1, None, 1, 0, None, 24, 40, 32, 42, None)
    assert "multiple of 4" in str(e.value)
    for name, args in (("stm_data_frames_u8_f32", (None, 2, None, 24, 40, 32, 64, None, None, 1, None)),
                       ("stm_data_rle_starts", (*n5, 2, 10, *n4, None)),
                       ("stm_data_masks_u8", (*n3, 2, None, 2, 10, None, 24, 40, 32, 64, None)),
                       ("stm_data_boxes_f32", (None, None, 2, None, 24, 40, 32, 64, None))):
        with pytest.raises(_lib.StmError) as e:
            _lib.call(name, *args)
        assert "NULL" in str(e.value), name
    with pytest.raises(_lib.StmError):
        _lib.call("stm_data_rle_starts", *n5, -1, 0, *n4, None)
    with pytest.raises(_lib.StmError):
        _lib.call("stm_data_rle_starts", *n5, 1, -1, *n4, None)
    # a frame descriptor with a row stride below 3 * W0 is refused on the host
    d = (_lib.DataFrameDesc * 1)()
    d[0].ptr, d[0].H0, d[0].W0, d[0].row_stride_bytes = 4096, 4, 4, 11
    m3 = (ctypes.c_double * 3)(1, 1, 1)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_data_frames_u8_f32", d, 1, ctypes.c_void_p(4096), 24, 40, 32, 64, m3, m3, 1, None)
    assert "row stride" in str(e.value)
    # nothing to do launches nothing: no device, no pointers, no error
    _lib.call("stm_data_frames_u8_f32", None, 0, None, 24, 40, 32, 64, None, None, 1, None)
    _lib.call("stm_data_rle_starts", *n5, 0, 0, *n4, None)
    _lib.call("stm_data_masks_u8", *n3, 1, None, 0, 0, None, 24, 40, 32, 64, None)
    _lib.call("stm_data_boxes_f32", None, None, 0, None, 24, 40, 32, 64, None)
