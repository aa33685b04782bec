"""The JPEG decoder on the MI355X (stmask_amd/jpeg.py, csrc/jpeg_decode.hip) against PIL's pixels: every fixture of tests/golden/jpeg_cases.npz
and of tests/golden/jpeg_edge_cases.npz bit for bit, singly and in one mixed batch, both channel orders; the host fallback; damaged files beside sound ones; no host wait in deferred
mode; the launch and upload counts; and the places it plugs into (collate_device, serve.device_prep) against the host-decoded path."""
import io
import random

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import train_data_cases as C
from stmask_amd import datasets, jpeg, serve

pytestmark = pytest.mark.gpu
GRID, UNSUPPORTED, DAMAGED = JC.load()
EDGE = JC.load_edge()


def _want(c, order):
    return torch.from_numpy(np.ascontiguousarray(c.rgb if order == "rgb" else c.rgb[:, :, ::-1]))


def _assert_frames(frames, cases, order):
    assert len(frames) == len(cases)
    for f, c in zip(frames, cases):
        assert f.dtype == torch.uint8 and f.is_cuda and tuple(f.shape) == c.rgb.shape and f.is_contiguous(), c.name
        assert torch.equal(f.cpu(), _want(c, order)), c.name


def test_every_fixture_singly():
    jpeg.reset_counters()
    for c in GRID:
        _assert_frames(jpeg.decode_batch([c.data], order="rgb", names=[c.name]), [c], "rgb")
    assert jpeg.COUNTERS["host_fallback"] == 0 and jpeg.COUNTERS["uploads"] == len(GRID) and jpeg.COUNTERS["launches"] == 3 * len(GRID)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_all_fixtures_in_one_mixed_batch(order):
    jpeg.reset_counters()
    frames = jpeg.decode_batch([c.data for c in GRID], order=order)
    _assert_frames(frames, GRID, order)
    assert jpeg.COUNTERS == {"launches": 3, "uploads": 1, "h2d_bytes": jpeg.COUNTERS["h2d_bytes"], "host_fallback": 0}
    assert 0 < jpeg.COUNTERS["h2d_bytes"] < 4 * sum(len(c.data) for c in GRID)
    base = frames[0].untyped_storage().data_ptr()
    assert all(f.untyped_storage().data_ptr() == base for f in frames)                 # views of ONE buffer


def test_every_edge_fixture_singly():
    """Narrow chroma planes, header layouts, table selections, the largest magnitudes, the staging window's offsets, 8192-pixel sides: each file
    alone, so that a failure names it."""
    jpeg.reset_counters()
    for c in EDGE:
        _assert_frames(jpeg.decode_batch([c.data], order="rgb", names=[c.name]), [c], "rgb")
    assert jpeg.COUNTERS["host_fallback"] == 0 and jpeg.COUNTERS["uploads"] == len(EDGE) and jpeg.COUNTERS["launches"] == 3 * len(EDGE)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("first", ["grid", "edge"])
def test_edge_fixtures_and_the_grid_in_one_batch(order, first):
    cases = GRID + EDGE if first == "grid" else EDGE + GRID
    jpeg.reset_counters()
    _assert_frames(jpeg.decode_batch([c.data for c in cases], order=order), cases, order)
    assert jpeg.COUNTERS == {"launches": 3, "uploads": 1, "h2d_bytes": jpeg.COUNTERS["h2d_bytes"], "host_fallback": 0}


def test_a_1024_segment_file_between_two_one_pixel_frames():
    """One wave a restart interval: 1024 workgroups of one image between images of one block, and the restart counter wraps 128 times."""
    long = next(c for c in EDGE if c.name.endswith("_grey_rst1"))
    assert len(jpeg.parse(long.data).segments) == 1024
    cases = [JC.by_name("1x1_420_q90"), long, JC.by_name("1x1_grey_q30opt")]
    for order in ("rgb", "bgr"):
        jpeg.reset_counters()
        _assert_frames(jpeg.decode_batch([c.data for c in cases], order=order), cases, order)
        assert jpeg.COUNTERS["launches"] == 3 and jpeg.COUNTERS["uploads"] == 1 and jpeg.COUNTERS["host_fallback"] == 0


def test_host_decoded_frames_first_last_and_side_by_side():
    """Images without blocks or segments share their first block index with the image behind them: the lookups must pass over them wherever
    they stand."""
    pytest.importorskip("PIL.Image")
    u, v = UNSUPPORTED
    a, b, c = JC.edge_by_name("narrow_3x9_420"), JC.by_name("33x31_422_q75rst3"), JC.edge_by_name("tables_three_selections")
    for cases in ([u, a, b, c], [a, b, c, u], [a, u, v, b, c], [u, v, a, b, v, u, c, u, v], [v, u, u, a]):
        jpeg.reset_counters()
        _assert_frames(jpeg.decode_batch([x.data for x in cases], order="rgb"), cases, "rgb")
        assert jpeg.COUNTERS["host_fallback"] == sum(x in UNSUPPORTED for x in cases) and jpeg.COUNTERS["uploads"] == 1 and jpeg.COUNTERS["launches"] == 3


def test_sixty_five_tiny_frames_in_one_batch():
    """More frames than any descriptor table in kernel arguments could hold, and a lookup over more than 64 images."""
    tiny = [c for c in GRID if c.rgb.shape[0] * c.rgb.shape[1] <= 64]
    cases = (tiny * 3)[:65]
    assert len(cases) == 65
    jpeg.reset_counters()
    _assert_frames(jpeg.decode_batch([c.data for c in cases], order="bgr"), cases, "bgr")
    assert jpeg.COUNTERS["launches"] == 3 and jpeg.COUNTERS["uploads"] == 1


def test_two_runs_give_the_same_bytes():
    datas = [c.data for c in GRID[::3]]
    a = jpeg.decode_batch(datas)
    b = jpeg.decode_batch(datas)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_unsupported_files_take_the_host_fallback_in_the_same_batch():
    pytest.importorskip("PIL.Image")
    cases = [GRID[40], UNSUPPORTED[0], GRID[77], UNSUPPORTED[1]]
    for order in ("rgb", "bgr"):
        jpeg.reset_counters()
        _assert_frames(jpeg.decode_batch([c.data for c in cases], order=order), cases, order)
        assert jpeg.COUNTERS["host_fallback"] == 2 and jpeg.COUNTERS["uploads"] == 1 and jpeg.COUNTERS["launches"] == 3
    jpeg.reset_counters()
    _assert_frames(jpeg.decode_batch([c.data for c in UNSUPPORTED], order="rgb"), UNSUPPORTED, "rgb")       # nothing but copies: one launch
    assert jpeg.COUNTERS["host_fallback"] == 2 and jpeg.COUNTERS["launches"] == 1


def test_damaged_files_are_flagged_by_name_and_their_neighbours_are_bit_equal():
    """The damaged files the host program passed under the sanitizers (the verdicts stored with the fixtures; tests/test_jpeg_cpu.py repeats
    that run and compares): what it flagged, the device flags with the same status word; what it decoded, the device decodes alike."""
    dev = JC.device_damaged()
    assert all(c.verdict.startswith("flagged") or c.verdict == "equal" for c in dev)
    flagged = [c for c in dev if c.verdict.startswith("flagged")]
    assert len(flagged) >= 7 and all(c in flagged for c in dev if "_cut" in c.name)
    sound = [JC.by_name("17x9_422_q90"), JC.by_name("48x40_420_q75rst3"), JC.by_name("64x50_444_q100noise")]
    cases = [sound[0]] + dev[:5] + [sound[1]] + dev[5:] + [sound[2]]
    names = [f"file {c.name}" for c in cases]
    frames, status = jpeg.decode_batch([c.data for c in cases], order="rgb", names=names, check="deferred")
    got = status.flagged()
    assert sorted(got) == [i for i, c in enumerate(cases) if c in flagged]                    # what the host program flags, the device flags
    for i, c in enumerate(cases):
        if c in flagged:
            assert got[i] == int(c.verdict.split()[1]), c.name                 # ... with the same status word
        elif c.rgb is not None:
            assert torch.equal(frames[i].cpu(), _want(c, "rgb")), c.name                      # sound neighbours, and damaged streams that are valid
    with pytest.raises(ValueError, match=f"file {cases[min(got)].name}: the JPEG data is damaged"):
        status.raise_if_bad()
    for c in flagged[:3]:                                                                     # check="raise" names the file
        with pytest.raises(ValueError, match=f"file {c.name}: the JPEG data is damaged"):
            jpeg.decode_batch([sound[0].data, c.data, sound[1].data], names=["a", f"file {c.name}", "b"])
    clean, status = jpeg.decode_batch([c.data for c in sound], check="deferred")
    status.raise_if_bad()
    assert status.flagged() == {}


def test_deferred_mode_never_waits_for_the_device():
    datas = [c.data for c in GRID[5::11]] + [UNSUPPORTED[0].data]
    jpeg.decode_batch(datas[:2])                                                              # the library is loaded and bound
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames, status = jpeg.decode_batch(datas, order="bgr", check="deferred")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    status.raise_if_bad()
    _assert_frames(frames, GRID[5::11] + [UNSUPPORTED[0]], "bgr")


# ---------------------------------------------------------------------------------------------------------------- where it plugs in
EXTRA_AUG = dict(photo_metric_distortion=dict(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18),
                 expand=dict(mean=C.MEAN, to_rgb=True, ratio_range=(1, 2)), random_crop=dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3))


def _batch(mode, aug, check="raise"):
    ann, host, device, _ = JC.sources()
    ds = datasets.YTVISTrainSet(ann, frame_reader=device if mode == "device" else host, img_scale=C.SIZE, size_divisor=C.DIVISOR, extra_aug=aug, decode=mode)
    random.seed(3)
    np.random.seed(3)
    records = [ds[i] for i in range(len(ds))]
    assert {r["size"] for r in records} == {(31, 33), (160, 96)}
    datasets.reset_counters()
    jpeg.reset_counters()
    return records, datasets.collate_device(records, check=check)


@pytest.mark.parametrize("aug", [None, EXTRA_AUG], ids=["plain", "extra_aug"])
def test_collate_device_on_compressed_records_equals_collate_device_on_host_decoded_frames(aug):
    h_records, (h_images, *h_gt, h_meta) = _batch("host", aug)
    h_counts = dict(datasets.COUNTERS)
    d_records, (d_images, *d_gt, d_meta) = _batch("device", aug)
    assert torch.equal(h_images, d_images) and h_images.shape[0] == len(h_records) == 7
    for what, a, b in zip(("boxes", "labels", "masks", "ids"), h_gt, d_gt):
        assert len(a) == len(b) == 7
        for ca, cb in zip(a, b):
            assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(ca, cb)), what
    assert len(h_meta) == len(d_meta) and all(str(x) == str(y) for x, y in zip(h_meta, d_meta))
    # the decode took the place of the frames' upload: one upload either way, three more launches, nothing else moved
    assert datasets.COUNTERS["launches"] == h_counts["launches"] and datasets.COUNTERS["uploads"] == h_counts["uploads"] - 1
    assert jpeg.COUNTERS["launches"] == 3 and jpeg.COUNTERS["uploads"] == 1 and jpeg.COUNTERS["host_fallback"] == 0


def test_collate_device_joins_the_decode_status_and_refuses_mixed_batches():
    records, out = _batch("device", None, check="deferred")
    assert len(out) == 7
    out[-1].raise_if_bad()
    h_records, _ = _batch("host", None)
    with pytest.raises(datasets.StmError, match="compressed and decoded"):
        datasets.collate_device([records[0], h_records[1]])
    cut = next(c for c in JC.device_damaged() if c.name == "33x31_420_q90_cut50")
    bad = dict(records[0], frames=[records[0]["frames"][0], jpeg.CompressedFrame(cut.data, name="cut.jpg")])
    with pytest.raises(ValueError, match=r"video 1, frame \d \(cut.jpg\): the JPEG data is damaged"):
        datasets.collate_device([records[1], bad])
    *_, status = datasets.collate_device([records[1], bad], check="deferred")
    with pytest.raises(ValueError, match="cut.jpg"):
        status.raise_if_bad()


def test_compressed_prep_equals_device_prep_on_host_decoded_frames():
    cases = [JC.by_name("64x50_420_q90"), None, JC.by_name("64x50_444_q30opt"), JC.by_name("96x160_420_rstrows1"), JC.by_name("64x50_grey_q75rst3")]
    ids = [0, None, 3, 1, 7]
    host = [None if c is None else torch.from_numpy(np.ascontiguousarray(c.rgb[:, :, ::-1])).pin_memory() for c in cases]
    comp = [None if c is None else jpeg.CompressedFrame(c.data, name=c.name) for c in cases]
    for size, cl in (((640, 360), True), ((96, 64), False)):
        want, want_meta = serve.device_prep(host, ids, size=size, channels_last=cl)
        jpeg.reset_counters()
        got, got_meta = jpeg.compressed_prep(size=size, channels_last=cl)(comp, ids)
        assert got.shape == want.shape and got.stride() == want.stride() and torch.equal(got, want)
        assert str(got_meta) == str(want_meta)
        assert jpeg.COUNTERS["launches"] == 3 and jpeg.COUNTERS["uploads"] == 1                 # the busy slots of a step: ONE decode_batch
    idle = jpeg.compressed_prep()([None, None], [None, None])
    assert idle[1] == [None, None] and not idle[0].any()
    with pytest.raises(jpeg.StmError, match="CompressedFrames"):
        jpeg.compressed_prep()(host, ids)


def test_a_360_by_640_file_against_live_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:360, 0:640]
    a = np.clip(np.stack([127 + 120 * np.sin(xx / (31.0 + 9 * c)) * np.cos(yy / 23.0) for c in range(3)], -1) + rng.normal(0, 12, (360, 640, 3)), 0, 255)
    bio = io.BytesIO()
    Image.fromarray(a.astype(np.uint8)).save(bio, "JPEG", quality=90, subsampling=2)
    ref = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))
    got = jpeg.decode_batch([bio.getvalue()], order="rgb")[0]
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
