"""What is about include/stmask_hip_tracker.h (the tracker's decisions on the device) alone: what its entries refuse without a device.
tests/test_abi.py compares the header with _lib.TRACKER_SIGNATURES, as it does for every header."""
import pytest

from stmask_amd import _lib


def test_call_checks_the_tracker_entries_without_a_device():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_track_resolve_tf", None, None)                      # argument count
    none = [None] * 5
    for bad in ([0, 0, 0, 0], [1025, 0, 0, 0], [1, -1, 0, 0], [1, 0, -1, 0], [1, 0, 0, -1], [1, 2 ** 31 - 1, 1, 0]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_track_resolve_tf", *none, *bad, None, None, None, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_track_resolve_tf", *none, 2, 3, 4, 0, None, None, None, None)
    assert "NULL" in str(e.value)
    for bad in ([0, 0], [1025, 0], [1, -1]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_track_drop_plan", None, None, *bad, None, None, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_track_drop_plan", None, None, 2, 3, None, None, None)
    assert "NULL" in str(e.value)
