"""stm_preprocess_u8_multi_f32: one launch (per 64 frames) pre-processes frames of different tensors and source sizes into one batch.  Image by
image bit-identical to the CPU oracle (orc_preprocess_u8) and to stm_preprocess_u8_f32.  The argument-error test runs without a GPU."""
import ctypes

import pytest
import torch

import oracle
from stmask_amd import _lib, ops, preprocess

SOURCES = [(720, 1280), (1080, 1920), (480, 854), (360, 640), (361, 643)]


def rand_u8(*shape, seed=0):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_mixed_sources_bit_equal_per_image(mode):
    host = [rand_u8(h, w, 3, seed=i) for i, (h, w) in enumerate(SOURCES)]
    frames = [f.cuda() for f in host]
    out = ops.preprocess_frames_multi(frames, mode=mode)
    assert out.shape == (len(SOURCES), 3, 384, 640)
    for i, f in enumerate(frames):
        assert torch.equal(out[i].cpu(), oracle.preprocess_frames(host[i][None], mode=mode)[0]), (i, SOURCES[i])
        assert torch.equal(out[i], ops.preprocess_frames(f[None], mode=mode)[0]), (i, SOURCES[i])


@pytest.mark.gpu
def test_more_than_64_frames_into_a_given_batch():
    """The chunk loop (64 descriptors per launch): 70 frames of two sizes, written in place into rows of a caller's tensor."""
    host = [rand_u8(*((45, 80) if i % 3 else (37, 53)), 3, seed=100 + i) for i in range(70)]
    big = torch.full((72, 3, 64, 96), -7.0, device="cuda")
    out = ops.preprocess_frames_multi([f.cuda() for f in host], out=big[1:71], size=(96, 54))
    assert out.data_ptr() == big[1].data_ptr()
    assert (big[0] == -7).all() and (big[71] == -7).all()          # nothing written outside the rows given
    for i, f in enumerate(host):
        assert torch.equal(big[1 + i].cpu(), oracle.preprocess_frames(f[None], size=(96, 54))[0]), i


@pytest.mark.gpu
def test_strided_source_crop_view():
    full = rand_u8(400, 700, 3, seed=7).cuda()
    crop = full[13:373, 21:661]                                      # rows 2100 bytes apart, 640 pixels each
    assert not crop.is_contiguous() and crop.stride(1) == 3
    other = rand_u8(720, 1280, 3, seed=8).cuda()
    out = ops.preprocess_frames_multi([crop, other])
    assert torch.equal(out[0].cpu(), oracle.preprocess_frames(crop.cpu().contiguous()[None])[0])
    assert torch.equal(out[1], ops.preprocess_frames(other[None])[0])


@pytest.mark.gpu
def test_eval_frames_multi_meta_per_frame():
    frames = [rand_u8(h, w, 3, seed=i).cuda() for i, (h, w) in enumerate(SOURCES[:3])]
    x, metas = preprocess.preprocess_eval_frames_multi(frames, [0, 5, 2])
    for i, f in enumerate(frames):
        xi, mi = preprocess.preprocess_eval_frames(f[None], idx=[0, 5, 2][i])
        assert torch.equal(x[i], xi[0]) and metas[i] == mi
        assert metas[i]["ori_shape"] == (SOURCES[i][0], SOURCES[i][1], 3)


def test_multi_argument_errors_without_gpu():
    """NULL pointers, n = 0 and bad sizes return STM_E* codes with a message (host-side checks, nothing launched)."""
    lib = _lib.lib()
    dummy = ctypes.c_void_p(64)
    rc = lib.stm_preprocess_u8_multi_f32(None, 1, dummy, 360, 640, 384, 640, None, None, 0, None)
    assert rc == -2 and b"non-NULL" in lib.stm_last_error_string()
    d = (_lib.FrameDesc * 2)()
    for i in range(2):
        d[i].ptr, d[i].H0, d[i].W0, d[i].row_stride_bytes = 64, 10, 10, 30
    rc = lib.stm_preprocess_u8_multi_f32(d, 0, dummy, 360, 640, 384, 640, None, None, 0, None)
    assert rc == -1 and b"bad sizes" in lib.stm_last_error_string()
    rc = lib.stm_preprocess_u8_multi_f32(d, 2, dummy, 360, 640, 352, 640, None, None, 0, None)     # padded height below the image
    assert rc == -1
    rc = lib.stm_preprocess_u8_multi_f32(d, 2, dummy, 360, 640, 384, 640, None, None, 4, None)     # mode
    assert rc == -1
    rc = lib.stm_preprocess_u8_multi_f32(d, 2, dummy, 360, 640, 384, 640, None, None, 1, None)     # mean / std missing
    assert rc == -2
    d[1].row_stride_bytes = 29                                                                    # rows shorter than 3 * W0
    rc = lib.stm_preprocess_u8_multi_f32(d, 2, dummy, 360, 640, 384, 640, None, None, 0, None)
    assert rc == -1 and b"frame 1" in lib.stm_last_error_string()
    d[1].row_stride_bytes, d[1].W0 = 30, 0
    assert lib.stm_preprocess_u8_multi_f32(d, 2, dummy, 360, 640, 384, 640, None, None, 0, None) == -1
    d[1].W0, d[1].ptr = 10, None
    assert lib.stm_preprocess_u8_multi_f32(d, 2, dummy, 360, 640, 384, 640, None, None, 0, None) == -2
    assert lib.stm_struct_bytes(4) == ctypes.sizeof(_lib.FrameDesc) == 24
