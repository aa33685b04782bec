"""The split entropy decode on the MI355X (stmask_amd/jpeg.py split=, csrc/jpeg_split.hip): the stored fixtures and the files of
tests/jpeg_split_cases.py through decode_batch(split="all" | "auto"), byte for byte against the expected pixels and against the serial path on the
same card; the launch and upload counts; status words and redone() sets against the host model (tests/jpeg_split_host_main.cpp), image for
image, on sound and on damaged files; and the places the option travels through (collate_device, compressed_prep)."""
import random

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import jpeg_split_cases as SC
import jpeg_write as JW
import train_data_cases as C
from stmask_amd import _lib, datasets, jpeg

pytestmark = pytest.mark.gpu
GRID, UNSUPPORTED, _ = JC.load()
EDGE = JC.load_edge()
SPLIT_TOTAL = jpeg.SPLIT_LAUNCHES + 2


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """cases, split -> {image: (verdict, mode)} of the host model"""
    d = tmp_path_factory.mktemp("jpeg_split_model")
    exe = SC.build_host_program(d, sanitize=False)

    def run(cases, split, lenient=0):
        SC.write_job(d / "job", cases, [lenient] * len(cases), split)
        rc, lines, text = SC.run_host_program(exe, d / "job")
        assert rc in (0, 1) and len(lines) == len(cases), text[-2000:]
        return lines
    return run


def _want(c, order):
    return torch.from_numpy(np.ascontiguousarray(c.rgb if order == "rgb" else c.rgb[:, :, ::-1]))


def _decode(cases, split, order="rgb"):
    """-> (frames, DecodeStatus, the counters of the call, the indices pack_batch split)"""
    jpeg.reset_counters()
    frames, status = jpeg.decode_batch([c.data for c in cases], order=order, names=[c.name for c in cases], check="deferred", split=split)
    counts = dict(jpeg.COUNTERS)
    assert jpeg.SPLIT_COUNTERS["redone"] == 0
    return frames, status, counts, jpeg.SPLIT_COUNTERS["images"]


def _assert_sound(cases, split, model, order="rgb", n_split=None):
    """Every file equal to its expected pixels and to the serial path's frame, none flagged, none redone; the modes are the model's."""
    frames, status, counts, images = _decode(cases, split, order)
    serial, s_status, s_counts, s_images = _decode(cases, None, order)
    modes = model(cases, split)
    assert status.flagged() == {} and s_status.flagged() == {}
    assert status.redone() == set() == {i for i, v in modes.items() if v[1] == "redone"}
    assert images == sum(v[1] == "split" for v in modes.values()) and s_images == 0
    if n_split is not None:
        assert images == n_split
    for i, c in enumerate(cases):
        assert modes[i][0] == "equal", (c.name, modes[i])
        assert torch.equal(frames[i], serial[i]), c.name
        assert torch.equal(frames[i].cpu(), _want(c, order)), c.name
    assert counts["uploads"] == 1 and counts["launches"] == (SPLIT_TOTAL if images else 3) and s_counts["launches"] == 3
    assert counts["h2d_bytes"] == s_counts["h2d_bytes"]
    return frames


def test_the_keyword_and_its_constants():
    assert jpeg.SPLIT_LAUNCHES == _lib.JPEG_SPLIT_ROUNDS + 4 and jpeg.SPLIT_MIN_BYTES == SC.GROUP_BYTES
    with pytest.raises(ValueError, match="split="):
        jpeg.decode_batch([GRID[0].data], split="some")


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_every_stored_fixture_in_one_batch_split_all(order, model):
    """16-bit codes, DC size 11, ZRL runs, crossed tables, stuffed bytes, fill bytes in front of the end marker: whatever has one segment of more
    than one sub-sequence is split, beside restart-marker files and files of a few bytes."""
    cases = GRID + EDGE
    _assert_sound(cases, "all", model, order)
    batch = jpeg.pack_batch([c.data for c in cases], split="all")
    assert len(batch.split_images) >= 70
    assert sum(c.name.split("_")[0] in JC.EDGE_GROUPS for c in [cases[i] for i in batch.split_images]) >= 20


def test_sub_sequence_and_group_boundaries(model):
    cases = SC.boundary_lengths() + SC.boundary_straddles()
    _assert_sound(cases, "all", model, n_split=len(cases) - 1)          # data of exactly one sub-sequence stays serial
    for c in cases:                                                      # ... and each alone, so that a failure names it
        _assert_sound([c], "all", model)


@pytest.mark.parametrize("split", ["all", "auto"])
def test_files_of_more_groups_than_rounds(split, model):
    cases = SC.multi_group()
    _assert_sound(cases, split, model, n_split=4)
    _assert_sound(cases[::-1] + [JC.by_name("1x1_420_q90")], split, model, "bgr", n_split=4)


def test_a_file_past_two_scan_tiles(model):
    _assert_sound([JC.by_name("33x31_444_q90"), SC.past_a_scan_tile(), SC.multi_group()[2]], "all", model, n_split=3)


def test_auto_leaves_short_segments_serial(model):
    short = [c for c in SC.boundary_straddles() if len(c.data) < SC.GROUP_BYTES] + [JC.by_name("96x160_420_rstrows1")]
    frames, status, counts, images = _decode(short, "auto")
    assert images == 0 and counts["launches"] == 3 and status.redone() == set()
    for f, c in zip(frames, short):
        assert torch.equal(f.cpu(), _want(c, "rgb")), c.name
    # files that cannot be split at all: restart markers, a few bytes
    none = [JC.by_name("96x160_420_rstrows1"), JC.by_name("1x1_grey_q30opt"), JC.by_name("48x40_420_q75rst3")]
    assert _decode(none, "all")[2]["launches"] == 3


def test_a_mixed_batch(model):
    """Split files beside restart-marker files, a 1 x 1 frame, an image whose records do not fit and (where PIL is there to decode it) a file
    the device does not decode, in several orders: images without groups share their first group with the image behind them."""
    tiny = SC.boundary_lengths()[0]
    long_tail = SC.Case("records_do_not_fit", JW.with_fill(JC.by_name("1x1_grey_q30opt").data, end=300), JC.by_name("1x1_grey_q30opt").rgb)
    b, e = SC.ecs_of(long_tail.data)
    assert e - b > 256 * 1 and jpeg.split_fits(e - b, 1) is False
    a, g, r, one = SC.boundary_straddles()[0], SC.multi_group()[3], JC.by_name("96x160_420_rstrows1"), JC.by_name("1x1_420_q90")
    try:
        import PIL.Image  # noqa: F401
        raw = [UNSUPPORTED[0]]
    except ImportError:
        raw = []
    for cases in ([a, r, g, one, long_tail, tiny] + raw, raw + [one, long_tail, a, r, r, g], [long_tail, g] + raw + [tiny, a, one]):
        _assert_sound(cases, "all", model, n_split=2)
        assert jpeg.pack_batch([c.data for c in cases], split="all").images[cases.index(long_tail)].split & 1 == 0


def test_damaged_files_have_the_serial_path_s_pixels_and_status(model):
    """Cuts and inverted bytes of the multi-group files: what the model flags the device flags, with the same status word; what the model
    redoes the device redoes; every frame is the serial path's, byte for byte; every cut is redone."""
    sound = SC.multi_group()
    cases = []
    for k, c in enumerate(sound):
        for d in SC.damaged_variants(c, 50 + k):
            try:
                jpeg.parse(d.data)
            except ValueError:
                continue
            cases.append(d)
    cases = cases[:7] + [sound[1]] + cases[7:]
    assert sum("_cut" in c.name for c in cases) == 12 and len(cases) >= 26
    verdicts = model(cases, "all", lenient=1)
    frames, status, counts, images = _decode(cases, "all")
    serial, s_status, _, _ = _decode(cases, None)
    assert counts["launches"] == SPLIT_TOTAL and images == len(cases)
    want_flag = {i: int(v[0].split()[1]) for i, v in verdicts.items() if v[0].startswith("flagged")}
    assert status.flagged() == want_flag == s_status.flagged()
    redone = status.redone()
    assert redone == {i for i, v in verdicts.items() if v[1] == "redone"} and s_status.redone() == set()
    assert all(i in redone for i, c in enumerate(cases) if "_cut" in c.name) and cases.index(sound[1]) not in redone
    assert set(want_flag) <= redone
    for i, c in enumerate(cases):
        assert torch.equal(frames[i], serial[i]), c.name
    with pytest.raises(ValueError, match=f"{cases[min(want_flag)].name}: the JPEG data is damaged"):
        status.raise_if_bad()


def test_two_runs_give_the_same_bytes_and_deferred_mode_never_waits():
    cases = SC.multi_group()[:2] + SC.boundary_straddles()[:2] + [JC.by_name("96x160_420_rstrows1")]
    datas = [c.data for c in cases]
    a = jpeg.decode_batch(datas, split="all")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b, status = jpeg.decode_batch(datas, split="all", check="deferred")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    status.raise_if_bad()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _batch(decode_split):
    ann, host, device, _ = JC.sources()
    ds = datasets.YTVISTrainSet(ann, frame_reader=device, img_scale=C.SIZE, size_divisor=C.DIVISOR, decode="device", decode_split=decode_split)
    random.seed(3)
    np.random.seed(3)
    records = [ds[i] for i in range(len(ds))]
    datasets.reset_counters()
    jpeg.reset_counters()
    return records, datasets.collate_device(records)


def test_collate_device_with_decode_split_equals_the_unsplit_batch():
    _, (want, *want_gt, want_meta) = _batch(None)
    assert jpeg.COUNTERS["launches"] == 3 and jpeg.SPLIT_COUNTERS["images"] == 0
    records, (got, *got_gt, got_meta) = _batch("all")
    assert jpeg.COUNTERS["launches"] == SPLIT_TOTAL and jpeg.COUNTERS["uploads"] == 1 and jpeg.SPLIT_COUNTERS["images"] >= 1
    assert all(r["decode_split"] == "all" for r in records)
    assert torch.equal(want, got) and str(want_meta) == str(got_meta)
    for a, b in zip(want_gt, got_gt):
        for ca, cb in zip(a, b):
            assert all(torch.equal(x, y) for x, y in zip(ca, cb))
    jpeg.reset_counters()
    plain = [{k: v for k, v in r.items() if k != "decode_split"} for r in records]
    assert torch.equal(datasets.collate_device(plain, decode_split="all")[0], want) and jpeg.COUNTERS["launches"] == SPLIT_TOTAL
    with pytest.raises(ValueError, match="decode_split"):
        datasets.YTVISTrainSet(JC.sources()[0], decode="host", decode_split="all")


def test_compressed_prep_with_split_equals_the_unsplit_prep():
    cases = [JC.by_name("64x50_420_q90"), None, JC.by_name("64x50_444_q30opt"), JC.by_name("96x160_420_rstrows1"), SC.multi_group()[3]]
    ids = [0, None, 3, 1, 7]
    comp = [None if c is None else jpeg.CompressedFrame(c.data, name=c.name) for c in cases]
    want, want_meta = jpeg.compressed_prep(size=(96, 64), channels_last=False)(comp, ids)
    for split, launches in (("all", SPLIT_TOTAL), ("auto", SPLIT_TOTAL)):
        jpeg.reset_counters()
        got, got_meta = jpeg.compressed_prep(size=(96, 64), channels_last=False, split=split)(comp, ids)
        assert torch.equal(got, want) and str(got_meta) == str(want_meta)
        assert jpeg.COUNTERS["launches"] == launches and jpeg.COUNTERS["uploads"] == 1
