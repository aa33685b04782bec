"""The batched output stage on the MI355X (stm_output_stage_multi_f32, output_utils.OutputStageBatch, VideoBatcher(batched_output=True)).
Every comparison is exact: RLE strings byte for byte against the oracle (mask_resize_threshold -> rle_encode -> rle_to_string), selection and
pixel boxes against output_utils.select_rows / pixel_boxes evaluated by torch on the device, records against postprocess_ytbvis ->
bbox2result_with_id."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from stmask_amd import _lib, eval_utils, ops, output_utils
from stmask_amd.ops import StmError

pytestmark = pytest.mark.gpu

HB, RB = ctypes.sizeof(_lib.OutputHeader), ctypes.sizeof(_lib.OutputRow)
KEPT, RUN_OVER = _lib.ROW_KEPT, _lib.ROW_RUN_OVERFLOW


def read_buffer(out, n):
    """device step buffer -> (header fields, record table int32 [n, 12], arena bytes)"""
    host = out.cpu().numpy()
    hdr = host[:HB].view(np.int32)
    return hdr, host[HB:HB + n * RB].view(np.int32).reshape(n, RB // 4), host[HB + n * RB:]


def row_string(table, arena, r):
    return arena[table[r, 3]:table[r, 3] + table[r, 4]].tobytes()


def embed(mask, mh, mw):
    """a frame's [h, w] mask in the top-left corner of the call's [mh, mw] mask (what lies outside the crop is never read)"""
    big = torch.full((mh, mw), 0.75)
    big[:mask.shape[0], :mask.shape[1]] = mask
    return big


def smooth(g, h, w, cells=4):
    low = torch.randn(1, 1, cells, cells + 2, generator=g) * 3
    return torch.sigmoid(torch.nn.functional.interpolate(low, (h, w), mode="bilinear", align_corners=False)[0, 0])


def alternating(h, w, long, short):
    """column x: ones in its first k rows, k alternating long / short -> in column-major order the one-runs alternate long and short, so every other
    difference against the run two before is negative and needs more than one 5-bit group"""
    m = torch.zeros(h, w)
    for x in range(w):
        m[:(long if x % 2 == 0 else short), x] = 1.0
    return m


def expected_string(mask, crop_h, crop_w, out_h, out_w):
    return oracle.rle_to_string(oracle.rle_encode(oracle.mask_resize_threshold(mask, crop_h, crop_w, out_h, out_w)))


# (mask size, crop, out) of the frames of the mixed call; frame 2 has no rows
FRAMES = [((24, 40), (22, 40), (90, 160)), ((12, 20), (12, 20), (50, 37)), ((12, 20), (12, 20), (33, 21)), ((12, 20), (12, 20), (7, 5)),
          ((12, 20), (12, 20), (64, 64)), ((12, 20), (12, 20), (1, 1)), ((96, 160), (90, 160), (360, 640))]
MH, MW = 96, 160
_case = {}


def mixed_case():
    """The rows of the mixed call (built and run once, shared by the tests that read it): (small masks, frame of row, expected strings, device
    result of ops.output_stage_multi)."""
    if _case:
        return _case
    g = torch.Generator().manual_seed(11)
    rows = []                                       # (frame, small mask)
    for f, ((mh, mw), _, _) in enumerate(FRAMES):
        if f == 2:
            continue
        rows += [(f, torch.zeros(mh, mw)), (f, torch.ones(mh, mw)), (f, torch.sigmoid(torch.randn(mh, mw, generator=g) * 3) if f < 6 else smooth(g, mh, mw)),
                 (f, smooth(g, mh, mw))]
    rows += [(0, alternating(24, 40, 20, 2)), (6, alternating(96, 160, 70, 5)), (1, alternating(12, 20, 11, 1))]
    perm = torch.randperm(len(rows), generator=g).tolist()                 # rows not grouped by frame
    rows = [rows[i] for i in perm]
    frame = [f for f, _ in rows]
    assert frame != sorted(frame)
    want = [expected_string(m, *FRAMES[f][1], *FRAMES[f][2]) for f, m in rows]
    n = len(rows)
    masks = torch.stack([embed(m, MH, MW) for _, m in rows]).cuda()
    frames = [(ch, cw, oh, ow, 1.0, 1.0) for _, (ch, cw), (oh, ow) in FRAMES]
    args = dict(masks=masks, frame_of_row=torch.tensor(frame, dtype=torch.int32).cuda(), score=torch.linspace(0.1, 0.9, n).cuda(),
                cls=torch.arange(1, n + 1).cuda(), box_id=torch.arange(n, dtype=torch.int32).cuda() * 3,
                box=torch.tensor([[0.25, 0.25, 0.5, 0.75]]).repeat(n, 1).cuda(), frames=frames, max_runs=8192, arena_bytes=1 << 18)
    out = ops.output_stage_multi(**args)
    torch.cuda.synchronize()
    _case.update(rows=rows, frame=frame, want=want, args=args, out=out, n=n)
    return _case


def test_mixed_frames_strings_equal_the_oracle():
    c = mixed_case()
    hdr, table, arena = read_buffer(c["out"], c["n"])
    assert hdr[0] == c["n"] and hdr[1] == sum(len(s) for s in c["want"]) and hdr[2] == 1 << 18
    off = 0
    for r, ((f, m), want) in enumerate(zip(c["rows"], c["want"])):
        assert table[r, 0] == f and table[r, 1] == KEPT, r
        assert table[r, 3] == off and table[r, 4] == len(want), (r, f)             # compact, in row order
        assert row_string(table, arena, r) == want, (r, f)
        off += len(want)
        assert table[r, 5] == r + 1 and table[r, 6] == 3 * r
        assert table[r:r + 1, 7].copy().view(np.float32)[0] == c["args"]["score"][r].item()
    # what the rows were built to reach: one run; [0, h*w] with a 4-character count at 360x640; negative multi-group differences; the 64x64 frame
    strings = {(f, i): w for i, ((f, _), w) in enumerate(zip(c["rows"], c["want"]))}
    assert any(len(w) == 1 for w in c["want"])                                   # 1x1, all-zero: "1"
    assert oracle.rle_to_string(torch.tensor([0, 230400])) in [w for (f, _), w in strings.items() if f == 6] and len(oracle.rle_to_string(torch.tensor([230400]))) == 4
    for f, m in c["rows"]:
        if f == 6 and m[:, 0].sum() == 70 and m[:, 1].sum() == 5:
            cnt = oracle.rle_encode(oracle.mask_resize_threshold(m, 90, 160, 360, 640))
            d = cnt[3:] - cnt[1:-2]
            assert int(d.min()) < -32 and int(d.max()) > 32
            break
    else:
        raise AssertionError("the alternating row is missing")
    assert (64 * 64) % 64 == 0 and any(f == 4 for f in c["frame"])


def test_same_submit_twice_is_byte_identical():
    c = mixed_case()
    again = ops.output_stage_multi(**c["args"])
    used = HB + c["n"] * RB + int(read_buffer(c["out"], c["n"])[0][1])
    assert torch.equal(again[:used], c["out"][:used])


def test_run_overflow_marks_that_row_only():
    """checkerboard 24x40 -> 24x40 (hundreds of runs) with max_runs = 16: its record says run overflow and has no string; the rows around it are complete"""
    yy, xx = torch.meshgrid(torch.arange(24), torch.arange(40), indexing="ij")
    masks = [torch.zeros(24, 40), ((yy + xx) % 2).float(), torch.ones(24, 40), (xx < 3).float()]
    frames = [(24, 40, 24, 40, 1.0, 1.0), (24, 40, 48, 80, 1.0, 1.0)]
    frame = [0, 0, 1, 1]
    n = 4
    out = ops.output_stage_multi(torch.stack(masks).cuda(), torch.tensor(frame, dtype=torch.int32).cuda(), torch.ones(n).cuda(), torch.ones(n, dtype=torch.int64).cuda(),
                                 torch.arange(n).cuda(), torch.tensor([[0.1, 0.1, 0.2, 0.2]]).repeat(n, 1).cuda(), frames, max_runs=16)
    hdr, table, arena = read_buffer(out, n)
    want = [expected_string(m, 24, 40, *frames[f][2:4]) for m, f in zip(masks, frame)]
    n_runs = len(oracle.rle_encode(oracle.mask_resize_threshold(masks[1], 24, 40, 24, 40)))
    assert n_runs > 900 and table[1, 1] == KEPT | RUN_OVER and table[1, 4] == 0 and table[1, 2] == n_runs
    for r in (0, 2, 3):
        assert table[r, 1] == KEPT and row_string(table, arena, r) == want[r], r
    assert table[:, 3].tolist() == [0, len(want[0]), len(want[0]), len(want[0]) + len(want[2])]
    assert hdr[1] == len(want[0]) + len(want[2]) + len(want[3])


def test_no_rows_and_seventy_frames():
    dev = "cuda"
    empty = ops.output_stage_multi(torch.zeros(0, 12, 20, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, device=dev),
                                   torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, 4, device=dev), [])
    assert read_buffer(empty, 0)[0][:2].tolist() == [0, 0]
    _lib.call("stm_output_stage_multi_f32", None, 0, 12, 20, None, None, None, 0, None, 0, None, None, None, 0, 0.0, 0.5, 16, None, 0, None, 0, None)
    # 70 frames of their own sizes, one row each, the rows in reverse frame order: three descriptor launches (64 + 6 frames, and frame 69 first)
    g = torch.Generator().manual_seed(5)
    n = 70
    sizes = [(1 + (3 * i) % 11, 1 + (5 * i) % 13) for i in range(n)]
    small = torch.sigmoid(torch.randn(n, 12, 20, generator=g) * 3)
    frame = list(range(n))[::-1]
    out = ops.output_stage_multi(small.cuda(), torch.tensor(frame, dtype=torch.int32).cuda(), torch.ones(n).cuda(), torch.ones(n, dtype=torch.int32).cuda(),
                                 torch.arange(n).cuda(), torch.tensor([[0.1, 0.1, 0.2, 0.2]]).repeat(n, 1).cuda(),
                                 [(12, 20, oh, ow, 1.0, 1.0) for oh, ow in sizes], max_runs=256)
    hdr, table, arena = read_buffer(out, n)
    for r in range(n):
        oh, ow = sizes[frame[r]]
        assert table[r, 0] == frame[r] and table[r, 1] == KEPT, r
        assert row_string(table, arena, r) == expected_string(small[r], 12, 20, oh, ow), (r, oh, ow)
    assert hdr[0] == n and hdr[1] == int(table[:, 4].sum())


def test_many_rows_of_a_large_frame():
    """4700 rows at 720x1280: one workgroup per four words of every row would be a grid of 2^32 threads and more (a served step of 32 clips holds
    this many tracked rows); the rows' workgroups stride instead.  Three tiny masks repeat, the last rows are checked like the first."""
    n = 4700
    assert n * (720 * 1280 // 256) * 256 >= 1 << 32
    xx = torch.arange(4).view(1, 4).expand(4, 4)
    patterns = [torch.zeros(4, 4), torch.ones(4, 4), (xx >= 2).float()]
    want = [expected_string(m, 4, 4, 720, 1280) for m in patterns]
    masks = torch.stack(patterns).repeat(n // 3 + 1, 1, 1)[:n].cuda()
    out = ops.output_stage_multi(masks, torch.zeros(n, dtype=torch.int32).cuda(), torch.ones(n).cuda(), torch.ones(n, dtype=torch.int32).cuda(),
                                 torch.arange(n).cuda(), torch.tensor([[0.1, 0.1, 0.2, 0.2]]).repeat(n, 1).cuda(), [(4, 4, 720, 1280, 1.0, 1.0)], max_runs=16)
    hdr, table, arena = read_buffer(out, n)
    assert (table[:, 1] == KEPT).all() and hdr[1] == sum(len(want[r % 3]) for r in range(n))
    text = arena[:hdr[1]].tobytes()
    assert text == b"".join(want[r % 3] for r in range(n))
    assert row_string(table, arena, n - 1) == want[(n - 1) % 3]


# ---- selection and boxes ----------------------------------------------------------------------------------------------------------------------

METAS = [{"ori_shape": (720, 1280, 3), "img_shape": (360, 640, 3), "pad_shape": (384, 640, 3)},
         {"ori_shape": (375, 625, 3), "img_shape": (340, 600, 3), "pad_shape": (352, 608, 3)},      # neither ratio is an fp32 number
         {"ori_shape": (480, 854, 3), "img_shape": (360, 640, 3), "pad_shape": (384, 640, 3)}]


def near_integer_inputs(s, size):
    """fp32 coordinates b for which trunc((b * (1 / s)) * size) and trunc((b / s) * size) differ (fp32 throughout, searched on the CPU around the
    pre-images of the integers): where a kernel that divides would disagree with torch, which multiplies by the reciprocal."""
    s = np.float32(s)
    inv = np.float32(1.0) / s
    base = (np.arange(1, size, dtype=np.float64) * np.float64(s) / size).astype(np.float32)
    cand = np.unique(np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-1))]).astype(np.float32))
    return cand[np.trunc((cand * inv) * np.float32(size)) != np.trunc((cand / s) * np.float32(size))]


def selection_rows(meta):
    """box [n,4] and score [n] of one frame: random boxes reaching outside [0, 1] (a third with x1 > x2 or y1 > y2), scores on both sides of 0.3 and
    exactly the fp32 value of 0.3, box centres exactly at the fp32 value of s_w / s_h and one ulp above, and every near-integer coordinate of
    this frame's ratios and sizes, as x1 / y1 and as x2 / y2."""
    img_h, img_w = meta["img_shape"][:2]
    pad_h, pad_w = meta["pad_shape"][:2]
    out_h, out_w = meta["ori_shape"][:2]
    s_w, s_h = img_w / pad_w, img_h / pad_h
    g = torch.Generator().manual_seed(out_w)
    box = torch.rand(48, 4, generator=g) * 1.4 - 0.2
    box[::3] = box[::3].flip(1)
    nx, ny = near_integer_inputs(s_w, out_w), near_integer_inputs(s_h, out_h)
    k = max(len(nx), len(ny))
    if k:
        px = torch.from_numpy(np.resize(nx, k)) if len(nx) else torch.full((k,), 0.25)
        py = torch.from_numpy(np.resize(ny, k)) if len(ny) else torch.full((k,), 0.25)
        near = torch.cat([torch.stack([px, py, torch.full((k,), 0.9), torch.full((k,), 0.9)], 1),
                          torch.stack([torch.full((k,), 0.01), torch.full((k,), 0.01), px, py], 1)])
        box = torch.cat([box, near])
    fw, fh = np.float32(s_w), np.float32(s_h)
    up_w, up_h = np.nextafter(fw, np.float32(2)), np.nextafter(fh, np.float32(2))
    edge = torch.tensor([[fw, 0.5, fw, 0.5], [up_w, 0.5, up_w, 0.5], [0.5, fh, 0.5, fh], [0.5, up_h, 0.5, up_h], [fw, fh, fw, fh]], dtype=torch.float32)
    box = torch.cat([box, edge])
    score = torch.rand(box.shape[0], generator=g) * 0.6
    score[::7] = 0.3                                                                # float32(0.3): not above the threshold
    score[1::7] = float(np.nextafter(np.float32(0.3), np.float32(1)))
    return box, score, len(nx), len(ny)


@pytest.mark.parametrize("threshold", [0.3, 0])
def test_selection_and_boxes_equal_torch_on_the_device(threshold):
    per_frame = [selection_rows(m) for m in METAS]
    # the near-integer set: 0 + 421 (frame 0: s_w = 1; 360/384 at 720 rows), 175 + 135 (frame 1), 0 + 303 (frame 2) coordinates, each used twice
    assert [(p[2], p[3]) for p in per_frame] == [(0, 421), (175, 135), (0, 303)]
    mh, mw = 8, 8
    boxes, scores, frame = [], [], []
    for f, (b, s, _, _) in enumerate(per_frame):
        boxes.append(b)
        scores.append(s)
        frame += [f] * b.shape[0]
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(len(frame), generator=g)
    box, score, frame = torch.cat(boxes)[perm].cuda(), torch.cat(scores)[perm].cuda(), torch.tensor(frame, dtype=torch.int32)[perm].cuda()
    n = box.shape[0]
    masks = torch.zeros(n, mh, mw, device="cuda")
    out = ops.output_stage_multi(masks, frame, score, torch.ones(n, dtype=torch.int64, device="cuda"), torch.arange(n, device="cuda"), box,
                                 [output_utils.frame_geometry(m, mh, mw) for m in METAS], score_threshold=threshold, max_runs=16)
    _, table, _ = read_buffer(out, n)
    n_kept = n_rejected = 0
    for f, meta in enumerate(METAS):
        idx = torch.nonzero(frame == f).view(-1)
        det = {"box": box[idx], "score": score[idx], "mask": masks[idx], "row": idx}
        kept, *_ = output_utils.select_rows(det, meta, score_threshold=threshold)
        want_rows = kept["row"].cpu().tolist()
        want_box = output_utils.pixel_boxes(kept["box"], meta).cpu().numpy()
        got_rows = [int(r) for r in idx.cpu().tolist() if table[r, 1] & KEPT]
        assert got_rows == want_rows, f
        assert np.array_equal(table[want_rows, 8:12].astype(np.int64), want_box), f
        assert all(table[r, 1] == 0 and not table[r, 8:12].any() for r in idx.cpu().tolist() if r not in set(want_rows))
        n_kept += len(want_rows)
        n_rejected += idx.numel() - len(want_rows)
    assert n_kept > 500 and n_rejected > 8
    # the five centre rows at the end of every frame's set: a centre exactly at the fp32 value of s_w / s_h is inside, one ulp above is outside
    inv = {int(p): i for i, p in enumerate(perm.tolist())}
    first = 0
    for b in boxes:
        first += b.shape[0]
        at = [inv[first - 5 + j] for j in range(5)]
        score_ok = [threshold == 0 or bool(score[r] > threshold) for r in at]
        assert [bool(table[r, 1] & KEPT) for r in at] == [a and e for a, e in zip(score_ok, [True, False, True, False, True])]


def test_row_keep_and_index_widths():
    n = 6
    keep = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.bool).cuda()
    masks = torch.ones(n, 4, 4).cuda()
    for dt in (torch.int32, torch.int64):
        out = ops.output_stage_multi(masks, torch.zeros(n, dtype=torch.int32).cuda(), torch.ones(n).cuda(), (torch.arange(n) + 7).to(dt).cuda(),
                                     (torch.arange(n) - 2).to(dt).cuda(), torch.tensor([[0.0, 0.0, 1.0, 1.0]]).repeat(n, 1).cuda(), [(4, 4, 3, 5, 1.0, 1.0)],
                                     row_keep=keep, max_runs=8)
        _, table, arena = read_buffer(out, n)
        assert table[:, 1].tolist() == [1, 0, 1, 1, 0, 1] and table[:, 5].tolist() == list(range(7, 13)) and table[:, 6].tolist() == list(range(-2, 4))
        assert all(row_string(table, arena, r) == oracle.rle_to_string(torch.tensor([0, 15])) for r in (0, 2, 3, 5))
        assert table[0, 8:12].tolist() == [0, 0, 5, 3]
    # a frame index that is no frame: the row is marked, not kept, and nothing is read through it
    out = ops.output_stage_multi(masks, torch.tensor([0, 1, -1, 0, 99, 0], dtype=torch.int32).cuda(), torch.ones(n).cuda(), torch.ones(n, dtype=torch.int32).cuda(),
                                 torch.arange(n).cuda(), torch.tensor([[0.0, 0.0, 1.0, 1.0]]).repeat(n, 1).cuda(), [(4, 4, 3, 5, 1.0, 1.0)], max_runs=8)
    assert read_buffer(out, n)[1][:, 1].tolist() == [1, _lib.ROW_BAD_FRAME, _lib.ROW_BAD_FRAME, 1, _lib.ROW_BAD_FRAME, 1]


def test_refusals_come_before_any_launch():
    n = 3
    masks = torch.rand(n, 12, 20).cuda()
    rest = (torch.zeros(n, dtype=torch.int32).cuda(), torch.ones(n).cuda(), torch.ones(n, dtype=torch.int64).cuda(), torch.arange(n).cuda(),
            torch.tensor([[0.1, 0.1, 0.2, 0.2]]).repeat(n, 1).cuda())
    out = torch.full((ops.output_stage_bytes(n, 4096),), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(StmError):
        ops.output_stage_multi(masks, *rest, [(13, 20, 30, 40, 1.0, 1.0)], out=out)                      # crop taller than the mask
    with pytest.raises(StmError):
        ops.output_stage_multi(masks, *rest, [(12, 21, 30, 40, 1.0, 1.0)], out=out)                      # ... wider
    with pytest.raises(StmError):
        ops.output_stage_multi(masks, *rest, [(12, 20, 65536, 32768, 1.0, 1.0)], out=out,                # 2^31 output pixels
                               workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(StmError):
        ops.output_stage_multi(masks, *rest, [(12, 20, 30, 40, 1.0, 1.0)], out=out, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(StmError):
        ops.output_stage_multi(masks, *rest, [(12, 20, 30, 40, 1.0, 1.0)], out=out[:HB + RB])            # no room for the records
    frames = ops.output_frames([(12, 20, 30, 40, 1.0, 1.0)])
    ws = torch.empty(_lib.lib().stm_output_stage_workspace_bytes(n, 1200, 64), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with pytest.raises(StmError) as e:
        _lib.call("stm_output_stage_multi_f32", None, n, 12, 20, p(rest[0]), p(rest[1]), p(rest[2]), 1, p(rest[3]), 1, p(rest[4]), None,
                  ctypes.cast(frames, ctypes.c_void_p), 1, 0.0, 0.5, 64, p(out), out.numel(), p(ws), ws.numel(), None)
    assert "non-NULL" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())                                                  # nothing was launched


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------

CLASSES = ["class_%d" % i for i in range(1, 41)]


def mirror_dets(seed, n=6):
    g = torch.Generator().manual_seed(seed)
    return {"box": torch.rand(n, 4, generator=g).sort(1)[0].cuda(), "score": torch.tensor([.9, .8, .01, .7, .6, .5]).cuda(),
            "class": torch.randint(1, 41, (n,), generator=g).cuda(), "mask": torch.sigmoid(torch.randn(n, 96, 160, generator=g) * 3).cuda(),
            "mask_coeff": torch.randn(n, 32, generator=g).cuda(), "box_ids": torch.arange(n).cuda(), "proto": torch.zeros(96, 160, 32).cuda()}


def flat_rows(dets):
    cat = lambda k: torch.cat([d[k] for d in dets])
    return {"mask": cat("mask"), "box": cat("box"), "score": cat("score"), "class": cat("class"), "box_id": cat("box_ids"),
            "frame": torch.cat([torch.full((d["box"].shape[0],), f, dtype=torch.int32) for f, d in enumerate(dets)]).cuda(),
            "keep": torch.ones(sum(d["box"].shape[0] for d in dets), dtype=torch.bool).cuda()}


def same_frame_record(got, want):
    assert list(got) == list(want) and [type(k) for k in got] == [type(k) for k in want]
    for k in want:
        if not isinstance(want[k], dict):
            assert got[k] == want[k]
            continue
        g, w = got[k], want[k]
        assert list(g) == list(w)
        assert g["bbox"].dtype == w["bbox"].dtype and g["bbox"].tolist() == w["bbox"].tolist()
        assert type(g["score"]) is type(w["score"]) is np.float32 and g["score"] == w["score"]
        assert type(g["label"]) is type(w["label"]) and g["label"] == w["label"] and g["category"] == w["category"]
        assert g["segm"] == w["segm"]


def test_output_stage_batch_equals_postprocess_per_frame():
    metas = [dict(METAS[0], video_id=7, frame_id=2), None, dict(METAS[2], video_id=8, frame_id=0), dict(METAS[0], video_id=9, frame_id=5)]
    busy = [0, 2, 3]
    steps = []
    for s in range(2):
        dets = [mirror_dets(20 + 3 * s + j) for j in range(3)]
        want = [None] * len(metas)
        for d, b in zip(dets, busy):
            post = output_utils.postprocess_ytbvis({"detection": d}, metas[b], score_threshold=0.05)
            want[b] = eval_utils.bbox2result_with_id(post, metas[b], CLASSES)
        rows = flat_rows(dets)
        rows["frame"] = torch.tensor(busy, dtype=torch.int32).cuda()[rows["frame"].long()]
        steps.append((rows, want))
    # room for every run of a 720p noise mask, a small arena and a small copied prefix: the strings come from the device, the arena has to grow
    # and the rest of the strings is fetched behind the prefix
    stage = output_utils.OutputStageBatch(CLASSES, score_threshold=0.05, max_runs=1 << 17, arena_bytes=1 << 16, prefix_bytes=1 << 12)
    tickets = [stage.submit(rows, metas) for rows, _ in steps]             # the second submit before the first collect: both pinned buffers
    for t, (_, want) in zip(tickets, steps):
        got = stage.collect(t)
        assert got[1] is None
        for b in busy:
            assert len(want[b]) > 2
            same_frame_record(got[b], want[b])
    assert stage.resubmits >= 1 and stage.reencoded_rows == 0 and stage.largest_total > 1 << 16
    # with the default 4096 runs these masks overflow: every kept row is encoded again alone, the records are the same
    small = output_utils.OutputStageBatch(CLASSES, score_threshold=0.05)
    got = small.collect(small.submit(steps[0][0], metas))
    for b in busy:
        same_frame_record(got[b], steps[0][1][b])
    assert small.reencoded_rows == sum(len(steps[0][1][b]) - 2 for b in busy)
    # a roomy arena behind a small copied prefix: the strings past the prefix are fetched by a second copy
    roomy = output_utils.OutputStageBatch(CLASSES, score_threshold=0.05, max_runs=1 << 17, arena_bytes=1 << 22, prefix_bytes=1 << 12)
    got = roomy.collect(roomy.submit(steps[1][0], metas))
    for b in busy:
        same_frame_record(got[b], steps[1][1][b])
    assert roomy.tail_copies == 1 and roomy.resubmits == 0 and roomy.reencoded_rows == 0
    assert stage.collect(stage.submit(None, metas)) == [None if m is None else {"video_id": m["video_id"], "frame_id": m["frame_id"]} for m in metas]


def test_video_batcher_batched_output_equals_per_frame_output():
    from scripts.run_video_demo import synthetic_video_u8
    from stmask_amd.serve import VideoBatcher
    from test_gpu_serve import demo_net
    net = demo_net()
    vids = [(50 - i, synthetic_video_u8(1, T, *((720, 1280) if i % 2 == 0 else (480, 854)), seed=60 + i)[0].cuda()) for i, T in enumerate([2, 4, 1, 2])]
    per_frame = VideoBatcher(net, 3).run(vids)                                 # 3 slots, 4 videos: the queue drains with idle slots
    vb = VideoBatcher(net, 3, batched_output=True)
    seen = []
    batched = vb.run(vids, on_frame=lambda v, t, img: seen.append((v, t)))    # (drawing the frames keeps working beside the batched records)
    assert len(per_frame) > 3 and batched == per_frame
    assert len(seen) == 9


@pytest.mark.parametrize("tf", [True, False], ids=["tf", "non_tf"])
def test_tracked_rows_are_the_rows_of_detections(tf):
    """BatchedClipPipeline.tracked_rows() against detections() on the staggered schedule of test_gpu_staggered_clips.py (resets, an idle slot):
    per clip, the rows the keep mask passes are detections()'s rows -- masks, boxes, scores, classes and box ids, bit for bit."""
    import test_gpu_staggered_clips as sc
    from stmask_amd.pipeline import BatchedClipPipeline
    net = sc.net_for("STMask_plus_resnet50_config", tf)
    xs = sc.batches(sc.videos(), sc.SLOTS)
    pipe = BatchedClipPipeline(net, 3)
    n_rows = n_kept = 0
    for t, x in enumerate(xs):
        pipe.step(x, is_first=sc.STAG_FIRST[t], active=sc.STAG_ACTIVE[t])
        rows, dets = pipe.tracked_rows(), pipe.detections()
        for b in range(3):
            want = dets[b]
            if rows is None:
                assert not want or want["box"].shape[0] == 0, (t, b)
                continue
            assert rows["frame"].dtype == torch.int32 and rows["mask"].shape[0] == rows["frame"].shape[0] == rows["keep"].shape[0]
            sel = torch.nonzero((rows["frame"] == b) & rows["keep"]).view(-1)
            if not want:
                assert sel.numel() == 0, (t, b)
                continue
            assert sel.numel() == want["box"].shape[0], (t, b)
            for mine, theirs in (("mask", "mask"), ("box", "box"), ("score", "score"), ("class", "class"), ("box_id", "box_ids")):
                assert torch.equal(rows[mine][sel].to(want[theirs].dtype), want[theirs]), (t, b, mine)
            n_kept += sel.numel()
        n_rows += 0 if rows is None else rows["frame"].shape[0]
    assert n_kept > 10 and n_rows >= n_kept
