"""Display mode on the MI355X: stm_render_overlay_u8 against the reference's own prep_display bytes (tests/golden/display_cases.npz), the
batched form against the single-frame form, coverage against the json masks, box outlines against the documented band rule, and
VideoBatcher's on_frame hook."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import display_model as dm
from conftest import ROOT
from stmask_amd import _lib, display, output_utils

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def z():
    return dm.load()


@pytest.mark.parametrize("name", list(dm.CASES))
def test_kernel_equals_reference_bytes(z, name):
    det, base, meta, mode = dm.case_inputs(z, name, DEV)
    out = display.render(det, base, meta, mode=mode, palette=z["COLORS"].tolist(), boxes=False)
    torch.cuda.synchronize()
    dm.check_against_golden(z, name, out.cpu().numpy())


def _mixed_frames(z, n):
    """n source-mode frames of mixed sizes and row counts (0 .. 44 rows, widths not a multiple of 4 included)."""
    names = ["src_empty_333x500", "src_one_480x854", "src_many_720x1280", "src_crowd_333x500"]      # one prototype size (96 x 160)
    sizes = [(72, 128), (101, 151), (333, 500), (97, 130), (64, 64), (480, 854)]
    dets, bases, metas = [], [], []
    g = torch.Generator().manual_seed(5)
    for i in range(n):
        det, _, meta, _ = dm.case_inputs(z, names[i % len(names)], DEV)
        k = int(det["score"].shape[0])
        if k:
            keep = torch.randperm(k, generator=g)[:max(0, k - (i % 5))].sort().values.to(DEV)
            det = {key: v.index_select(0, keep) for key, v in det.items()}
        h, w = sizes[i % len(sizes)]
        meta = dict(meta, ori_shape=(h, w, 3))
        dets.append(det)
        bases.append(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV))
        metas.append(meta)
    return dets, bases, metas


def test_batch_of_mixed_frames_equals_single_frames(z):
    dets, bases, metas = _mixed_frames(z, 70)
    batch = display.render_batch(dets, bases, metas, mode="source")
    assert len(batch) == 70
    for i in range(70):
        one = display.render(dets[i], bases[i], metas[i], mode="source")
        assert torch.equal(one, batch[i]), i
    # reference mode in one batch (frames with rows share one prototype size)
    names = ["ref_many_360x640", "ref_empty_360x640", "ref_one_360x640"]
    ins = [dm.case_inputs(z, n, DEV) for n in names]
    rb = display.render_batch([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], mode="reference", palette=z["COLORS"].tolist(),
                              boxes=False)
    torch.cuda.synchronize()
    for n, o in zip(names, rb):
        dm.check_against_golden(z, n, o.cpu().numpy())


def _decode_rle(counts, h, w):
    """COCO compressed RLE string -> bool [h, w] (inverse of output_utils.rle_counts_to_string; column-major runs)."""
    runs, p, s = [], 0, counts
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(runs) > 2:
            x += runs[-2]
        runs.append(x)
    flat = np.zeros(h * w, dtype=bool)
    pos, val = 0, False
    for r in runs:
        flat[pos:pos + r] = val
        pos += r
        val = not val
    return flat.reshape(w, h).T


@pytest.mark.parametrize("name", ["src_many_720x1280", "src_crowd_333x500", "src_small_72x128"])
def test_coverage_equals_json_masks(z, name):
    det, base, meta, mode = dm.case_inputs(z, name, DEV)
    n = int(det["score"].shape[0])
    det = dict(det, box_ids=torch.arange(n, device=DEV))
    pal = [(2 + (7 * i) % 250, 2 + (13 * i) % 250, 2 + (29 * i) % 250) for i in range(5 * n + 1)]   # row i -> entry 5 i: unique, no zero channel
    black = torch.zeros_like(base)
    out = display.render(det, black, meta, mode="source", palette=pal, alpha=1.0, boxes=False).cpu().numpy()
    post = output_utils.postprocess_ytbvis({"detection": det}, meta, score_threshold=0.05, preserve_aspect_ratio=True)
    h, w = meta["ori_shape"][:2]
    masks = [_decode_rle(s["counts"], h, w) for s in post["segm"]]
    union = np.any(masks, 0)
    assert ((out != 0).any(2) == union).all()
    top = np.full((h, w), -1)
    for j in reversed(range(len(masks))):
        top[masks[j]] = j
    ids = post["box_ids"].cpu().numpy()
    for j in range(len(masks)):
        sel = top == j
        if sel.any():
            expect = np.array(pal[(int(ids[j]) * 5) % len(pal)][::-1])                             # BGR frame
            assert (np.abs(out[sel].astype(int) - expect) <= 1).all(), j


def test_box_outlines_follow_the_band_rule(z):
    from test_display_cpu import band
    det, base, meta, mode = dm.case_inputs(z, "src_crowd_333x500", DEV)
    det = dict(det, mask=torch.zeros_like(det["mask"]))                    # outlines only
    out = display.render(det, base, meta, mode="source").cpu().numpy()
    m, ids, pix, *_ = display.select(det, meta, "source")
    h, w = meta["ori_shape"][:2]
    expect = np.floor(base.cpu().numpy().astype(np.float32) / np.float32(255.0) * np.float32(255.0)).astype(np.uint8)
    cols = np.rint(display.palette_colors(ids, bgr=True).cpu().numpy() * 255).astype(np.uint8)
    boxes = display.clamp_boxes(pix, w, h).cpu().numpy()
    for j in reversed(range(len(boxes))):
        expect[band(h, w, tuple(boxes[j]))] = cols[j]
    assert len(boxes) >= 24 and (out == expect).all()
    # no boxes, no masks: the base alone
    plain = display.render(det, base, meta, mode="source", boxes=False).cpu().numpy()
    assert (plain == np.floor(base.cpu().numpy().astype(np.float32) / np.float32(255.0) * np.float32(255.0)).astype(np.uint8)).all()


def test_abi_symbol_struct_and_header_agree():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "stmask_hip.h")).read()
    assert int(re.search(r"#define STM_ABI_VERSION (\d+)", header).group(1)) == L.stm_version() == _lib.ABI_VERSION == 6
    assert L.stm_struct_bytes(5) == ctypes.sizeof(_lib.RenderFrame)
    assert hasattr(L, "stm_render_overlay_u8") and "stm_render_overlay_u8" in _lib.ABI_SYMBOLS


def test_video_batcher_on_frame():
    from test_gpu_serve import LENGTHS, demo_net, queue
    from stmask_amd.serve import VideoBatcher
    net = demo_net()
    vids = queue()
    plain = VideoBatcher(net, 2).run(vids)
    seen = []
    vb = VideoBatcher(net, 2)
    orig = vb.pipe.detections
    step_dets = []

    def detections():
        d = orig()
        step_dets.append([{k: v.clone() for k, v in x.items()} if x else x for x in d])
        return d

    vb.pipe.detections = detections
    got = vb.run(vids, on_frame=lambda vid, fid, img: seen.append((vid, fid, img.clone())))
    assert got == plain
    assert len(seen) == sum(LENGTHS)
    by_id = {v[0]: v[1] for v in vids}
    from stmask_amd.serve import schedule
    plan = schedule(LENGTHS, 2)
    k = 0
    n_drawn = 0
    for s, row in enumerate(plan):
        for b, c in enumerate(row):
            if c is None:
                continue
            vid, fid, img = seen[k]
            k += 1
            assert (vid, fid) == (vids[c[0]][0], c[1])
            frame = by_id[vid][fid].to(DEV)
            meta = {"ori_shape": (frame.shape[0], frame.shape[1], 3), "img_shape": (360, 640, 3), "pad_shape": (384, 640, 3)}
            ref = display.render(step_dets[s][b], frame, meta, mode="source")
            assert torch.equal(img, ref), (vid, fid)
            n_drawn += bool(step_dets[s][b] and step_dets[s][b]["box"].shape[0])
    assert n_drawn > 0
