"""What is about include/stmask_hip_train.h (the batched mask term of the training criterion) alone: what its entries refuse without a device.
tests/test_abi.py compares the header with _lib.TRAIN_SIGNATURES, as it does for every header."""
import pytest

from stmask_amd import _lib


def test_call_checks_the_train_entries_without_a_device():
    """Every refusal comes from the shapes, before a launch: nothing here needs a device."""
    lib = _lib.lib()
    assert lib.stm_mbox_workspace_bytes(0, 5) == 64 and lib.stm_mbox_workspace_bytes(1 << 11, (1 << 11) + 1) == 64
    assert lib.stm_mbox_workspace_bytes(2, 300) > 2 * 300 * 8
    for shape in ([0, 12, 20, 8], [65536, 12, 20, 8], [2, 0, 20, 8], [2, 12, 20, 16], [2, 1 << 15, 1 << 15, 8]):       # what the launch entry refuses
        assert lib.stm_lincomb_rows_proto_backward_workspace_bytes(*shape) == 64, shape
    assert lib.stm_lincomb_rows_proto_backward_workspace_bytes(2, 12, 20, 8) == 8 * 2 * 240 * 8 * 4 + 64              # 8 splits of [2,12,20,8] fp32
    assert lib.stm_lincomb_rows_proto_backward_workspace_bytes(3, 128, 176, 8) == 64                                   # more than 256 workgroups: no split
    with pytest.raises(_lib.StmError):
        _lib.call("stm_mbox_positives", None, None)                        # argument count
    for B, P, rows in ([0, 1, 0], [1, 0, 0], [1 << 11, (1 << 11) + 1, 0], [1, 1, -1], [1, 1, 65536]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_positives", None, None, B, P, rows, None, 0, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_mbox_positives", None, None, 2, 300, 0, None, 0, None)
    assert "NULL" in str(e.value)
    none7 = [None] * 7
    for n_rows, B, P, M in ([0, 2, 300, 8], [65536, 2, 300, 8], [4, 0, 300, 8], [4, 2, 300, 16], [4, 1 << 11, (1 << 11) + 1, 32]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_gather_f32", None, None, 0, None, None, None, 3, *none7, n_rows, B, P, M, 48, 80, None, 0, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_scatter_coeff_f32", None, None, None, None, None, n_rows, B, P, M, None, 0, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_mbox_gather_f32", None, None, 0, None, None, None, 3, *none7, 4, 2, 300, 8, 48, 80, None, 0, None)
    assert "NULL" in str(e.value)
    for n_rows in (0, 65536):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_reduce_f32", None, None, None, None, None, n_rows, 1.0, None)
        with pytest.raises(_lib.StmError):
            _lib.call("stm_mbox_reduce_backward_f32", None, None, None, None, None, n_rows, 1.0, None)
    for h, w, m, n in ([12, 20, 16, 4], [0, 20, 8, 4], [12, 20, 8, 0], [12, 20, 8, 65536]):
        with pytest.raises(_lib.StmError):
            _lib.call("stm_lincomb_rows_proto_backward_f32", None, None, 2, None, None, None, None, None, h, w, m, n, None, 0, None)
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_lincomb_rows_proto_backward_f32", None, None, 2, None, None, None, None, None, 12, 20, 8, 4, None, 0, None)
    assert "NULL" in str(e.value)
