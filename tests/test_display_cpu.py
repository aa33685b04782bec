"""Display mode on the host: the documented compositing order against the reference's own prep_display bytes, the palette rule, row
selection, the box-band rule and the argument checks of stm_render_overlay_u8 (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import display_model as dm
from stmask_amd import _lib, display, output_utils


@pytest.fixture(scope="module")
def z():
    return dm.load()


@pytest.mark.parametrize("name", list(dm.CASES))
def test_restatement_equals_reference_bytes(z, name):
    det, base, meta, mode = dm.case_inputs(z, name)
    dm.check_against_golden(z, name, dm.restate(det, base, meta, mode, z["COLORS"].tolist()).numpy())


def test_fixtures_cover_what_they_claim(z):
    """Threshold and centre-test removals, 24+ drawn rows, repeated ids, 0.5 plateaus, crop-edge masks, and a sum order that matters."""
    assert float(z["eval_conf_thresh"]) == 0.05 and int(z["top_k"]) == 100 and float(z["score_threshold"]) == 0
    det, base, meta, mode = dm.case_inputs(z, "src_many_720x1280")
    n_in = det["score"].shape[0]
    thr, *_ = output_utils.select_rows(det, meta, 0.05, preserve_aspect_ratio=False)
    both, crop_h, crop_w, *_ = output_utils.select_rows(det, meta, 0.05, preserve_aspect_ratio=True)
    assert thr["score"].shape[0] < n_in and both["score"].shape[0] < thr["score"].shape[0]
    det_c, *_ = dm.case_inputs(z, "src_crowd_333x500")
    crowd, *_ = display.select(det_c, meta, "source")
    assert crowd.shape[0] >= 24
    ids = det["box_ids"].tolist()
    assert len(set(ids)) < len(ids)
    k = z["src_many_720x1280/mask_u8"]
    assert (k == 128).any() and (k[:, crop_h - 1, :] > 128).any()
    # a plain sequential sum of the terms differs from the reference bytes on the crowded frame: the grouping is pinned
    m, ids_c, _, ch, cw, oh, ow = display.select(det_c, dm.display_cases.meta(dm.CASES["src_crowd_333x500"]), "source")
    img = dm.base_image(dm.case_inputs(z, "src_crowd_333x500")[1], None, "source")
    cov = dm.coverage(m, ch, cw, oh, ow)
    col = display.palette_colors(ids_c, z["COLORS"].tolist(), bgr=True)
    a = torch.tensor(0.45)
    out = img.clone()
    for j in reversed(range(cov.shape[0])):                 # back to front: img = img * inv_j + mc_j
        mm = cov[j].float()[..., None]
        out = out * (mm * (-a) + 1) + (mm * col[j].view(1, 1, 3)) * a
    with pytest.raises(AssertionError):
        dm.check_against_golden(z, "src_crowd_333x500", (out * 255).byte().numpy())


def test_palette_index_rule(z):
    colors = z["COLORS"].tolist()
    ids = torch.tensor([0, 1, 3, 4, 7, 19, 100])
    c = display.palette_colors(ids, colors)
    for r, i in enumerate(ids.tolist()):
        ref = torch.tensor(colors[(i * 5) % len(colors)], dtype=torch.float32) / 255.0
        assert torch.equal(c[r], ref)
    assert torch.equal(display.palette_colors(ids, colors, bgr=True), c.flip(1))
    assert len(display.PALETTE) == 20 and all(len(p) == 3 and all(0 <= v <= 255 for v in p) for p in display.PALETTE)
    d = display.palette_colors(torch.tensor([2]))
    assert torch.equal(d[0], torch.tensor(display.PALETTE[10], dtype=torch.float32) / 255.0)


@pytest.mark.parametrize("name", ["src_many_720x1280", "ref_many_360x640", "src_crowd_333x500"])
def test_row_selection_follows_postprocess_ytbvis(z, name):
    det, base, meta, mode = dm.case_inputs(z, name)
    m, ids, pix, crop_h, crop_w, out_h, out_w = display.select(det, meta, mode)
    post = output_utils.postprocess_ytbvis({"detection": det}, meta, display_mask=True, score_threshold=0.05,
                                           preserve_aspect_ratio=mode == "source")
    assert torch.equal(ids, post["box_ids"]) and torch.equal(pix, post["box"])
    assert torch.equal(dm.coverage(m, crop_h, crop_w, out_h, out_w), post["segm"].bool())
    # top_k and the score cut
    m2, ids2, *_ = display.select(det, meta, mode, top_k=5)
    assert torch.equal(ids2, ids[:5])
    s = post["score"]
    cut = int(torch.nonzero(s < 0.5)[0])
    m3, ids3, *_ = display.select(det, meta, mode, score_threshold=0.5)
    assert (ids3 is None and cut == 0) or torch.equal(ids3, ids[:cut])
    empty = display.select(None, meta, mode)
    assert empty[0] is None and empty[5:] == (out_h, out_w)


def band(h, w, box):
    """The documented outline rule on a blank [h, w] canvas."""
    x1, y1, x2, y2 = box
    x1, x2, y1, y2 = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    yy, xx = np.mgrid[0:h, 0:w]
    vert = ((abs(xx - x1) <= 1) | (abs(xx - x2) <= 1)) & (yy >= y1 - 1) & (yy <= y2 + 1)
    horz = ((abs(yy - y1) <= 1) | (abs(yy - y2) <= 1)) & (xx >= x1 - 1) & (xx <= x2 + 1)
    return vert | horz


def test_box_band_rule_small_cases():
    b = band(8, 10, (2, 2, 6, 5))
    # the outline of (2, 2)-(6, 5): columns 1..3 and 5..7 over rows 1..6, rows 1..3 and 4..6 over columns 1..7
    expect = np.zeros((8, 10), bool)
    expect[1:7, 1:4] = expect[1:7, 5:8] = True
    expect[1:4, 1:8] = expect[4:7, 1:8] = True
    assert (b == expect).all()
    # clipped at the frame: a box clamped to max_w = w paints only column w - 1 of its right edge
    c = band(6, 6, tuple(display.clamp_boxes(torch.tensor([[0, 0, 9, 9]]), 6, 6)[0].tolist()))
    assert c[1:, 1:4].all() and c[5, 1:].all() and c[1:, 5].all() and not c[0, :].any() and not c[:, 0].any()
    assert display.clamp_boxes(torch.tensor([[-5, 1, 400, 300]]), 320, 180).tolist() == [[2, 2, 320, 180]]
    # swapped corners draw the same band
    assert (band(9, 9, (6, 5, 2, 2)) == band(9, 9, (2, 2, 6, 5))).all()


def _frame(**kw):
    f = _lib.RenderFrame()
    f.base, f.out, f.base_row_stride, f.out_row_stride = 64, 64, 12, 12
    f.base_fmt, f.base_h, f.base_w, f.out_h, f.out_w = 0, 2, 4, 2, 4
    f.inst_begin, f.n_inst, f.crop_h, f.crop_w = 0, 1, 8, 8
    for k, v in kw.items():
        setattr(f, k, v)
    return f


@pytest.mark.parametrize("bad,code", [
    (dict(n_inst=-1), -1), (dict(inst_begin=-2), -1), (dict(inst_begin=1), -1), (dict(base=None), -2), (dict(out=None), -2),
    (dict(crop_h=9), -1), (dict(crop_w=0), -1), (dict(out_row_stride=11), -1), (dict(base_h=3), -1), (dict(base_fmt=2), -1),
    (dict(base_fmt=1, base_h=8, base_w=8, base_crop_h=9, base_crop_w=8), -1),
])
def test_bad_descriptors_are_refused_before_any_launch(bad, code):
    L = _lib.lib()
    arr = (_lib.RenderFrame * 1)(_frame(**bad))
    fake = ctypes.c_void_p(64)
    rc = L.stm_render_overlay_u8(arr, 1, fake, 1, 8, 8, fake, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(1 << 20), None)
    assert rc == code, L.stm_last_error_string()
    assert b"stm_render_overlay_u8" in L.stm_last_error_string()


def test_bad_counts_and_pointers_are_refused():
    L = _lib.lib()
    fake = ctypes.c_void_p(64)
    arr = (_lib.RenderFrame * 1)(_frame())
    assert L.stm_render_overlay_u8(arr, -1, fake, 1, 8, 8, fake, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(1 << 20), None) == -1
    assert L.stm_render_overlay_u8(arr, 1, fake, -1, 8, 8, fake, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(1 << 20), None) == -1
    assert L.stm_render_overlay_u8(None, 1, fake, 1, 8, 8, fake, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(1 << 20), None) == -2
    assert L.stm_render_overlay_u8(arr, 1, None, 1, 8, 8, fake, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(1 << 20), None) == -2
    assert L.stm_render_overlay_u8(arr, 1, fake, 1, 8, 8, None, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(1 << 20), None) == -2
    assert L.stm_render_overlay_u8(arr, 1, fake, 1, 8, 8, fake, None, ctypes.c_float(0.45), fake, ctypes.c_size_t(4), None) == -4
    assert L.stm_render_overlay_u8(arr, 0, None, 0, 0, 0, None, None, ctypes.c_float(0.45), None, ctypes.c_size_t(0), None) == 0


def test_abi_6_binding():
    L = _lib.lib()
    assert L.stm_version() == _lib.ABI_VERSION == 6
    assert L.stm_struct_bytes(5) == ctypes.sizeof(_lib.RenderFrame) == 128
    assert L.stm_render_workspace_bytes(10) >= 160
