"""What is about include/stmask_hip_output.h (the batched output stage) alone: the status bits of a row record and what its entry refuses without a
device.  tests/test_abi.py compares the header with _lib.OUTPUT_SIGNATURES and its structs with their mirrors, as it does for every header."""
import re

import pytest

from abi_header import header_text
from stmask_amd import _lib


def test_row_status_bits_match_the_python_side():
    text = header_text("stmask_hip_output.h")
    for bit, name in ((1, "STM_ROW_KEPT"), (2, "STM_ROW_RUN_OVERFLOW"), (4, "STM_ROW_ARENA_OVERFLOW"), (8, "STM_ROW_BAD_FRAME")):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == bit
    assert (_lib.ROW_KEPT, _lib.ROW_RUN_OVERFLOW, _lib.ROW_ARENA_OVERFLOW, _lib.ROW_BAD_FRAME) == (1, 2, 4, 8)


def test_call_counts_the_arguments_of_the_output_table():
    with pytest.raises(_lib.StmError):
        _lib.call("stm_output_stage_multi_f32", None, 1)
    # n == 0 is STM_OK before any pointer is looked at; n < 0 and NULL pointers are refused without a device
    args = [None, 0, 4, 4, None, None, None, 0, None, 0, None, None, None, 0, 0.0, 0.5, 16, None, 0, None, 0, None]
    _lib.call("stm_output_stage_multi_f32", *args)
    args[1] = -1
    with pytest.raises(_lib.StmError):
        _lib.call("stm_output_stage_multi_f32", *args)
    args[1] = 2
    with pytest.raises(_lib.StmError) as e:
        _lib.call("stm_output_stage_multi_f32", *args)
    assert "non-NULL" in str(e.value)
