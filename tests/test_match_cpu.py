"""Training target assignment without a GPU: the torch restatement (tests/match_restate.py) is held to the reference's fp32 goldens
(tests/golden/match_cases.npz), and the new C-ABI entries and layer functions report what is out of contract instead of running it."""
import ctypes

import pytest
import torch

import match_cases as MC
import match_restate as R
from stmask_amd import _lib, layers


@pytest.mark.parametrize("name", MC.names())
def test_restatement_equals_the_reference_fp32(name):
    """Integers exactly; loc_t columns 0-1 bit for bit; columns 2-3 (one log and one division after the same fp32 quotient) within four fp32
    roundings of the stored values' magnitude."""
    c = MC.case(name)
    pos, neg = MC.thresholds()
    r = R.match(pos, neg, c["bbox"], c["labels"], c["ids"], c["priors"], c["conf"])
    assert torch.equal(r["idx_t"], c["idx_t"])
    assert torch.equal(r["conf_t"], c["conf_t"])
    assert torch.equal(r["ids_t"], c["ids_t"])
    assert torch.equal(r["gt_boxes_t"], c["bbox"][c["idx_t"]])
    assert torch.equal(r["loc_t"][:, :2], c["loc_t"][:, :2])
    wh, ref = r["loc_t"][:, 2:], c["loc_t"][:, 2:]
    assert bool(((wh - ref).abs() <= 4 * 2.0 ** -24 * ref.abs().clamp(min=1)).all())
    assert r["n_keep"] == c["n_keep"] and int(r["multi"].sum()) == c["n_multi"]
    assert R.margin(r) > 1e-4


def test_cases_reach_their_paths():
    """What each case is there for, read from the fixture: the multi-instance rule fires, the tiny box skips the classification term and is
    positive only through its forced match, and the twin boxes get two different priors."""
    assert MC.case("p300_multi")["n_multi"] > 0
    tiny = MC.case("p300_tiny")
    assert tiny["n_keep"] == 0 and int((tiny["conf_t"] > 0).sum()) == 1
    twin = MC.case("lvl24x40_twin")
    ov = R.overlaps(twin["bbox"], R.point_form(twin["priors"]))
    assert int(ov[0].argmax()) == int(ov[1].argmax())
    assert sorted(twin["idx_t"][twin["conf_t"] > 0].tolist()) == [0, 1]
    for n in ("full_g1", "full_g7", "full_g20", "full_g40", "p300_g65", "p300_g128"):
        assert MC.case(n)["n_keep"] > 0


def test_restated_encode_equals_the_reference():
    m, p, out = MC.encode_case()
    e = R.encode(m, p)
    assert torch.equal(e[:, :2], out[:, :2])
    assert bool(((e[:, 2:] - out[:, 2:]).abs() <= 4 * 2.0 ** -24 * out[:, 2:].abs().clamp(min=1)).all())


def _fake(addr):
    return ctypes.c_void_p(addr)


def _call_match(lib, boxes=0x10000, labels=0x20000, ids=0x30000, offs=0x40000, B=1, G_total=3, G_max=3, priors=0x50000, P=300, conf=0x60000,
                C=41, outs=(0x70000, 0x80000, 0x90000, 0xA0000, 0xB0000), ws=0xC0000, ws_bytes=1 << 30):
    """stm_match_priors_f32 with made-up addresses: every call here must be refused before any device work."""
    return lib.stm_match_priors_f32(_fake(boxes), _fake(labels), _fake(ids), _fake(offs), B, G_total, G_max, _fake(priors), 0, P, _fake(conf), C,
                                    ctypes.c_double(0.5), ctypes.c_double(0.4), *[_fake(o) for o in outs], None, _fake(ws),
                                    ctypes.c_size_t(ws_bytes), None)


def test_match_argument_errors_are_codes_with_messages():
    lib = _lib.lib()
    msg = lib.stm_last_error_string
    assert _call_match(lib, boxes=0) == -2 and b"non-NULL" in msg()                              # STM_ENULL
    assert _call_match(lib, outs=(0x70000, 0x80000, 0, 0xA0000, 0xB0000)) == -2 and b"non-NULL" in msg()
    assert _call_match(lib, G_total=0, G_max=0) == -1 and b"at least one ground-truth box" in msg()   # G = 0: STM_EINVAL
    assert _call_match(lib, B=2, G_total=1, G_max=1) == -1                                       # one of two images has no box
    assert _call_match(lib, G_total=129, G_max=129) == -5 and b"limit 128" in msg()              # STM_EUNSUPPORTED
    assert _call_match(lib, G_total=40, G_max=40, P=37) == -1 and b"40 boxes for 37 priors" in msg()
    assert _call_match(lib, C=1) == -5 and _call_match(lib, C=129) == -5
    assert _call_match(lib, boxes=0x10004) == -1 and b"16-byte aligned" in msg()                 # misaligned boxes
    assert _call_match(lib, priors=0x50008) == -1 and b"16-byte aligned" in msg()
    assert _call_match(lib, ws=0) == -4 and _call_match(lib, ws_bytes=64) == -4 and b"workspace" in msg()   # STM_EWORKSPACE
    need = lib.stm_match_workspace_bytes(8, 15345, 320, 40)
    assert need >= 4 * (320 * 15345 + 3 * 8 * 15345) and lib.stm_match_workspace_bytes(1, 300, 0, 0) == 0


def test_encode_argument_errors_are_codes_with_messages():
    lib = _lib.lib()
    assert lib.stm_encode_boxes_f32(None, None, None, ctypes.c_int64(5), None) == -2 and b"non-NULL" in lib.stm_last_error_string()
    assert lib.stm_encode_boxes_f32(None, None, None, ctypes.c_int64(-1), None) == -1
    assert lib.stm_encode_boxes_f32(None, None, None, ctypes.c_int64(0), None) == 0
    assert lib.stm_encode_boxes_f32(_fake(0x10004), _fake(0x20000), _fake(0x30000), ctypes.c_int64(5), None) == -1
    assert b"16-byte aligned" in lib.stm_last_error_string()


def test_variants_outside_every_config_are_not_implemented():
    m, p, _ = MC.encode_case()
    with pytest.raises(NotImplementedError):
        layers.encode(m, p, use_yolo_regressors=True)
    c = MC.case("p37_g1")
    P = c["priors"].shape[0]
    targets = (torch.zeros(1, P, 4), torch.zeros(1, P, dtype=torch.int64), torch.zeros(1, P, dtype=torch.int64), torch.zeros(1, P, dtype=torch.int64))
    for flag in ("use_yolo_regressors", "use_prediction_matching", "use_change_matching"):
        with pytest.raises(NotImplementedError):
            layers.match(0.5, 0.4, c["bbox"], c["labels"], c["ids"], c["priors"], None, c["conf"], *targets, 0, **{flag: True})
        with pytest.raises(NotImplementedError):
            layers.match_batch(0.5, 0.4, [c["bbox"]], [c["labels"]], [c["ids"]], c["priors"], c["conf"][None], **{flag: True})


def test_cpu_tensors_fail_loudly():
    """No CPU fallback: the layer functions need their tensors on the device."""
    c = MC.case("p37_g1")
    m, p, _ = MC.encode_case()
    with pytest.raises(_lib.StmError):
        layers.encode(m, p)
    with pytest.raises(_lib.StmError):
        layers.match_batch(0.5, 0.4, [c["bbox"]], [c["labels"]], [c["ids"]], c["priors"], c["conf"][None])
    assert layers.encode(m[:0], p[:0]).shape == (0, 4)
