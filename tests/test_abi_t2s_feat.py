"""What is about include/stmask_hip_t2s_feat.h (T2S_concat_feat and its adjoint) alone: what the entry points and their wrappers refuse is refused
from the shapes, without a device.  tests/test_abi.py compares the header with _lib.T2S_FEAT_SIGNATURES, as it does for every header."""
import pytest
import torch

from stmask_amd import _lib, layers, ops


def test_entry_points_refuse_from_the_shapes_without_a_device():
    fwd = lambda *dims: _lib.call("stm_t2s_feat_forward_f32", None, None, None, *dims, None)                        # noqa: E731
    bwd = lambda *dims: _lib.call("stm_t2s_feat_backward_f32", None, None, None, None, None, None, *dims, None)     # noqa: E731
    with pytest.raises(_lib.StmError):
        _lib.call("stm_t2s_feat_forward_f32", None, None)                                  # argument count
    #            bs  C  Cu  H  W  P
    for bad in ([0, 8, 4, 3, 4, 3], [1, 0, 4, 3, 4, 3], [1, 8, 0, 3, 4, 3], [1, 8, 4, 0, 4, 3], [1, 8, 4, 3, 0, 3], [1, 8, 4, 3, 4, 4], [1, 8, 4, 3, 4, 0],
                [1, 8, 4, 3, 4, -3], [1, 8, 4, 4096, 4096, 13], [1, 128, 4, 4096, 4096, 3], [1, 8, 128, 4096, 4096, 3]):
        for f in (fwd, bwd):
            with pytest.raises(_lib.StmError):
                f(*bad)
    for f in (fwd, bwd):
        with pytest.raises(_lib.StmError) as e:
            f(1, 8, 4, 3, 4, 3)                                                            # sizes fine: NULL pointers, before any launch
        assert "NULL" in str(e.value)


def test_wrappers_refuse_from_the_shapes_without_a_device():
    fpn, t2s = torch.zeros(4, 8, 3, 4), torch.zeros(4, 4, 3, 4)
    meta = lambda *shape: torch.empty(*shape, device="meta")                               # noqa: E731  (sizes only: nothing is allocated)
    bad = [(fpn[:3], t2s[:3], 3),                                                          # an odd image count
           (fpn, torch.zeros(4, 4, 3, 5), 3), (fpn, torch.zeros(4, 4, 2, 4), 3), (fpn, torch.zeros(2, 4, 3, 4), 3),
           (fpn, t2s.double(), 3), (fpn.half(), t2s.half(), 3),
           (fpn, t2s, 4), (fpn, t2s, 0), (fpn, t2s, -1),
           (fpn.transpose(2, 3).contiguous().transpose(2, 3), t2s, 3), (fpn, torch.zeros(4, 8, 3, 4)[:, ::2], 3),      # not contiguous
           (meta(2, 8, 4096, 4096), meta(2, 4, 4096, 4096), 13), (meta(2, 128, 4096, 4096), meta(2, 4, 4096, 4096), 3)]
    for f, t, P in bad:
        with pytest.raises(_lib.StmError):
            ops.t2s_check_shapes("t2s_concat_feat", f, t, P)
        if not f.is_meta:
            with pytest.raises(_lib.StmError):
                layers.t2s_concat_feat(f, t, patch_size=P, fused=True)
    if torch.cuda.is_available():
        with pytest.raises(_lib.StmError):
            ops.t2s_check_shapes("t2s_concat_feat", fpn.cuda(), t2s, 3)                    # two devices
    # shapes that are fine reach the device check: the product path has no CPU fallback
    with pytest.raises(_lib.StmError) as e:
        layers.t2s_concat_feat(fpn, t2s, patch_size=3, fused=True)
    assert "CPU" in str(e.value)
