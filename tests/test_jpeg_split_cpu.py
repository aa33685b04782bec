"""The split entropy decode without a GPU: the arithmetic of csrc/jpeg_split_core.h in the host model (tests/jpeg_split_host_main.cpp, built with
AddressSanitizer and UBSan and run as a process of its own) over the stored fixtures and the files of tests/jpeg_split_cases.py; the layout
pack_batch(split=...) writes and what the entry point refuses of it; the constants and the kernels' resources.

The model says which segments converge with R = STM_JPEG_SPLIT_ROUNDS rounds behind round 0.  No sound file named here may be redone: REDONE_EDGE
is the list of stored edge fixtures that are (asserted equal to the model's; it is empty), and a generated file that did not converge would be
replaced in tests/jpeg_split_cases.py, not listed."""
import ctypes
import os
import re

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_split_cases as SC
import jpeg_write as JW
from kernel_resources import kernel_resources
from stmask_amd import _lib, jpeg

GRID, UNSUPPORTED, _ = JC.load()
EDGE = JC.load_edge()
SUB, GROUP, ROUNDS = SC.SUB, SC.GROUP, SC.ROUNDS
REDONE_EDGE = []
EINVAL = -1


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_split_host")
    return d, SC.build_host_program(d), JC.build_host_program(d)


def _model(programs, cases, split, lenient=0, frames=None):
    d, exe, _ = programs
    batch = SC.write_job(d / "job", cases, [lenient] * len(cases), split)
    rc, lines, text = SC.run_host_program(exe, d / "job", frames)
    assert rc in (0, 1) and len(lines) == len(cases), text[-3000:]
    assert "ERROR" not in text and "runtime error" not in text, text[-3000:]
    return batch, rc, lines


def _all_equal_and_split(programs, cases, split="all", n_split=None):
    batch, rc, lines = _model(programs, cases, split)
    assert rc == 0
    for i, c in enumerate(cases):
        assert lines[i] == ("equal", "split" if i in batch.split_images else "serial"), (c.name, lines[i])
    if n_split is not None:
        assert len(batch.split_images) == n_split
    return batch


def _data_bytes(c):
    b, e = SC.ecs_of(c.data)
    return e - b


# ---------------------------------------------------------------------------------------------------------------- the constants
def test_the_defines_equal_their_mirrors():
    text = open(os.path.join(JC.ROOT, "stmask_amd", "csrc", "jpeg.h")).read()
    define = lambda name: re.search(r"#define " + name + r" (\([^\n]*?\)|\S+)", text).group(1)                            # noqa: E731
    assert int(define("STM_JPEG_SUB_BYTES")) == _lib.JPEG_SUB_BYTES == 128 and int(define("STM_JPEG_SUB_GROUP")) == _lib.JPEG_SUB_GROUP
    assert int(define("STM_JPEG_SPLIT_ROUNDS")) == _lib.JPEG_SPLIT_ROUNDS
    assert define("STM_JPEG_SPLIT_LAUNCHES") == "(STM_JPEG_SPLIT_ROUNDS + 4)" and jpeg.SPLIT_LAUNCHES == _lib.JPEG_SPLIT_LAUNCHES == _lib.JPEG_SPLIT_ROUNDS + 4
    assert define("STM_JPEG_REDONE") == "(1 << 8)" and _lib.JPEG_REDONE == 1 << 8
    assert define("STM_JPEG_SPLIT_MAX_BYTES") == "(1 << 30)" and _lib.JPEG_SPLIT_MAX_BYTES == 1 << 30
    assert jpeg.SPLIT_MIN_BYTES == SUB * GROUP and jpeg.SPLIT_COUNTERS.keys() == {"images", "redone"}
    assert all(_lib.JPEG_REDONE & s == 0 for s in jpeg.STATUS_TEXT)
    assert ctypes.sizeof(_lib.JpegImage) == 96 and _lib.JpegImage.split.offset == 92


def test_decode_status_masks_the_redone_bit():
    class Ready:
        def synchronize(self):
            pass
    import torch
    st = jpeg.DecodeStatus(None, np.array([0, 1, 1, 2, 3]), list("abcd"))
    st.host, st.event = torch.tensor([0, _lib.JPEG_REDONE, 0, _lib.JPEG_REDONE | _lib.JPEG_ETRUNCATED, _lib.JPEG_EINDEX], dtype=torch.int32), Ready()
    assert st.flagged() == {2: _lib.JPEG_ETRUNCATED, 3: _lib.JPEG_EINDEX} and st.redone() == {1, 2}
    with pytest.raises(ValueError, match="c: the JPEG data is damaged \\(the entropy-coded data ends"):
        st.raise_if_bad()
    assert jpeg.DecodeStatus(None, np.zeros(0), []).redone() == set()


# ---------------------------------------------------------------------------------------------------------------- the model over sound files
def test_every_stored_fixture_is_equal_under_split_all(programs):
    """Most edge fixtures exceed one sub-sequence and so split: 16-bit codes, DC size 11, ZRL runs, crossed tables, stuffed bytes, fill bytes."""
    cases = GRID + EDGE
    batch, rc, lines = _model(programs, cases, "all")
    assert rc == 0 and all(v[0] == "equal" for v in lines.values()), [(cases[i].name, v) for i, v in lines.items() if v[0] != "equal"]
    redone = [cases[i].name for i, v in lines.items() if v[1] == "redone"]
    assert redone == REDONE_EDGE and len(REDONE_EDGE) < 0.05 * len(EDGE)
    split = [cases[i] for i, v in lines.items() if v[1] == "split"]
    assert sorted(i for i, v in lines.items() if v[1] != "serial") == batch.split_images
    assert sum(c in EDGE for c in split) >= 20 and sum(c in GRID for c in split) >= 50
    for c in cases:                                                     # what is split is what can be
        h = jpeg.parse(c.data)
        blocks = h.mcu_w * h.mcu_h * (h.hs * h.vs + h.ncomp - 1)
        assert (c in split) == (len(h.segments) == 1 and _data_bytes(c) > SUB and 32 * -(-_data_bytes(c) // SUB) <= 64 * blocks), c.name


def test_sub_sequence_boundaries(programs):
    lengths = SC.boundary_lengths()
    assert [_data_bytes(c) for c in lengths] == [SUB, SUB + 1, 2 * SUB - 1, 2 * SUB]
    straddles = SC.boundary_straddles()
    data = {c.name: c.data[slice(*SC.ecs_of(c.data))] for c in straddles}
    at = lambda name, pair: any(data[name][b + pair[0]] == 0xFF and data[name][b + pair[0] + 1] == 0 for b in range(SUB, len(data[name]) - 1, SUB))   # noqa: E731
    assert at("stuffed_ff_then_boundary", (-1,)) and at("stuffed_pair_then_boundary", (-2,)) and at("boundary_then_stuffed", (0,))
    g = data["stuffed_at_group_boundary"]
    assert g[SUB * GROUP - 1] == 0xFF and g[SUB * GROUP] == 0 and len(g) > SUB * GROUP + SUB
    _all_equal_and_split(programs, lengths + straddles, n_split=len(lengths) + len(straddles) - 1)
    for c in lengths + straddles:
        _all_equal_and_split(programs, [c])


def test_files_of_more_groups_than_rounds_and_past_a_scan_tile(programs):
    multi = SC.multi_group()
    assert [jpeg.parse(c.data).hs * jpeg.parse(c.data).vs + jpeg.parse(c.data).ncomp - 1 for c in multi] == [1, 3, 4, 6]
    assert all(_data_bytes(c) > (ROUNDS + 2) * GROUP * SUB for c in multi)
    tile = SC.past_a_scan_tile()
    assert _data_bytes(tile) > 2 * 256 * SUB
    for split in ("all", "auto"):
        _all_equal_and_split(programs, multi + [tile], split, n_split=5)
    b = _all_equal_and_split(programs, SC.boundary_straddles()[:3] + multi[:1], "auto", n_split=1)      # auto: SPLIT_MIN_BYTES or more
    assert b.split_images == [3]


def _long_tail():
    one = JC.by_name("1x1_grey_q30opt")
    c = SC.Case("records_do_not_fit", JW.with_fill(one.data, end=300), one.rgb)
    assert _data_bytes(c) > 256 * 1 and not jpeg.split_fits(_data_bytes(c), 1)
    return c


def test_a_mixed_batch_and_its_layout(programs):
    a, g, r, one, tiny = SC.boundary_straddles()[0], SC.multi_group()[3], JC.by_name("96x160_420_rstrows1"), JC.by_name("1x1_420_q90"), SC.boundary_lengths()[0]
    long_tail = _long_tail()
    raw = []
    try:
        import PIL.Image  # noqa: F401
        raw = [UNSUPPORTED[0]]
    except ImportError:
        pass
    groups = lambda c: -(-(-(-_data_bytes(c) // SUB)) // GROUP)                                                              # noqa: E731
    for cases in ([a, r, g, one, long_tail, tiny] + raw, raw + [one, long_tail, a, r, r, g], [long_tail, g] + raw + [tiny, a, one]):
        batch = _all_equal_and_split(programs, cases, n_split=2)
        assert batch.split_images == sorted([cases.index(a), cases.index(g)]) and batch.total_groups == groups(a) + groups(g) == 1 + groups(g)
        before = 0
        for i, c in enumerate(cases):                                    # the prefix: groups before the image, doubled, and the image's own flag
            assert batch.images[i].split == 2 * before + (c in (a, g)), (i, c.name)
            before += groups(c) if c in (a, g) else 0
        # the same files unsplit: every other byte of the descriptors, the blob's size, the workspace
        plain = jpeg.pack_batch([c.data for c in cases], "rgb")
        assert plain.workspace_bytes == batch.workspace_bytes == _lib.private_fn("stm_jpeg_workspace_bytes")(batch.images, batch.n_images)
        assert plain.blob_bytes == batch.blob_bytes and bytes(plain.segments) == bytes(batch.segments)
        images = (_lib.JpegImage * batch.n_images)()
        ctypes.memmove(images, batch.images, ctypes.sizeof(images))
        for im in images:
            im.split = 0
        assert bytes(images) == bytes(plain.images)[:ctypes.sizeof(images)]
        assert all(im.split == 0 for im in plain.images) and plain.split_images == [] and plain.total_groups == 0


def test_unsplit_descriptors_are_what_they_were():
    """split=None, and a split option that finds nothing to split, write the bytes the parent's pack_batch wrote: the field is zero."""
    cases = [JC.by_name("96x160_420_rstrows1"), JC.by_name("1x1_grey_q30opt"), SC.boundary_lengths()[0]]
    base = jpeg.pack_batch([c.data for c in cases])
    for split in ("all", "auto"):
        b = jpeg.pack_batch([c.data for c in cases], split=split)
        assert bytes(b.images) == bytes(base.images) and bytes(b.segments) == bytes(base.segments) and b.split_images == [] and b.blob_bytes == base.blob_bytes
    a = np.frombuffer(bytes(base.images), dtype=np.int32).reshape(-1, 24)
    assert not a[:, 23].any()
    with pytest.raises(ValueError, match="split="):
        jpeg.pack_batch([cases[0].data], split="yes")
    with pytest.raises(TypeError):
        jpeg.pack_batch([cases[0].data], "bgr", None, None, None)


# ---------------------------------------------------------------------------------------------------------------- damaged files
def test_damaged_multi_group_files_end_as_the_serial_decoder_ends_them(programs):
    """Verdict and status word are tests/jpeg_host_main.cpp's on the same bytes; the pixels are those of the model run over the unsplit batch,
    which is that program's decode; every cut is redone, and so is whatever is flagged."""
    d, exe, serial_exe = programs
    sound = SC.multi_group()
    cases = []
    for k, c in enumerate(sound):
        for v in SC.damaged_variants(c, 50 + k):
            try:
                jpeg.parse(v.data)
            except ValueError:
                continue
            cases.append(v)
    assert sum("_cut" in c.name for c in cases) == 12 and sum("_flip" in c.name for c in cases) >= 15
    batch, rc, lines = _model(programs, cases, "all", lenient=1, frames=d / "split.frames")
    assert len(batch.split_images) == len(cases)
    _, _, plain = _model(programs, cases, None, lenient=1, frames=d / "serial.frames")
    JC.write_job(d / "job_serial", cases, [1] * len(cases))
    _, ref, text = JC.run_host_program(serial_exe, d / "job_serial")
    assert len(ref) == len(cases), text[-2000:]
    for i, c in enumerate(cases):
        assert lines[i][0] == plain[i][0] == ref[i] and plain[i][1] == "serial", (c.name, lines[i], plain[i], ref[i])
        assert lines[i][1] == "redone" or not ref[i].startswith("flagged"), (c.name, lines[i])
        if "_cut" in c.name:
            assert lines[i] == (f"flagged {_lib.JPEG_ETRUNCATED}", "redone"), (c.name, lines[i])
    assert (d / "split.frames").read_bytes() == (d / "serial.frames").read_bytes()
    assert sum(v[1] == "split" for v in lines.values()) >= 5           # an inverted byte often leaves a stream that decodes: split, and equal


# ---------------------------------------------------------------------------------------------------------------- refusals
def _call(batch, **over):
    """stm_jpeg_decode_u8 over a packed batch with fake (never dereferenced) device pointers -> the return code"""
    a = dict(images=batch.images, n_images=batch.n_images, segments=batch.segments, n_segments=batch.n_segments, blob=0x1000, blob_bytes=batch.blob_bytes,
             images_off=batch.images_off, segments_off=batch.segments_off, out=0x2000, out_bytes=batch.out_bytes, status=0x3000, workspace=0x4000,
             workspace_bytes=batch.workspace_bytes, bgr=1, stages=7, stream=None)
    a.update(over)
    return _lib.private_fn("stm_jpeg_decode_u8")(*a.values())


def test_the_entry_point_refuses_a_split_field_that_disagrees():
    g, r, a = SC.multi_group()[0], JC.by_name("96x160_420_rstrows1"), SC.boundary_straddles()[0]
    b = jpeg.pack_batch([a.data, r.data, g.data, _long_tail().data, a.data], split="all")
    assert [im.split for im in b.images] == [1, 2, 3, 2 * (1 + b.total_groups - 2) , 2 * (b.total_groups - 1) + 1]

    def broken(i, value):
        images = (_lib.JpegImage * b.n_images)()
        ctypes.memmove(images, b.images, ctypes.sizeof(images))
        images[i].split = value
        rc = _call(b, images=images)
        assert rc != 0                                                   # (a call that passed would launch on the fake pointers)
        return rc
    assert broken(1, 3) == EINVAL                                        # more than one segment
    assert broken(3, b.images[3].split | 1) == EINVAL                    # records that do not fit
    assert broken(2, 5) == EINVAL and broken(2, 1) == EINVAL             # a prefix that is not the groups before: too many, too few
    assert broken(4, b.images[4].split + 2) == EINVAL and broken(4, b.images[4].split - 2) == EINVAL     # ... the group count of image 2
    assert broken(0, 0) == EINVAL and broken(0, -1) == EINVAL            # image 1's prefix no longer continues it; a negative field
    assert broken(1, 0) == EINVAL
    assert "split field" in _lib.lib().stm_last_error_string().decode()
    assert _call(b, workspace_bytes=b.workspace_bytes - 1) == -4         # the workspace is the unsplit batch's, to the byte
    tiny = jpeg.pack_batch([SC.boundary_lengths()[0].data], split="all")   # one sub-sequence: no split
    images = (_lib.JpegImage * 1)()
    ctypes.memmove(images, tiny.images, ctypes.sizeof(images))
    images[0].split = 1
    assert _call(tiny, images=images) == EINVAL


# ---------------------------------------------------------------------------------------------------------------- the kernels
def test_split_kernels_use_no_scratch():
    """The lanes of the sync and write kernels each walk a bit stream of their own; an indexed local array (a table, a copy of a descriptor) would
    put that walk into scratch memory.  The report, for the record: registers, LDS (the group's bytes, skewed, and four Huffman tables)."""
    seen = {}
    for name, r in kernel_resources("jpeg_split.hip").items():
        kernel = next((k for k in ("jpeg_split_sync_kernel", "jpeg_split_scan_kernel", "jpeg_split_write_kernel") if k in name), None)
        assert kernel is not None and not any(k in name for k in ("jpeg_entropy_kernel", "jpeg_idct_kernel", "jpeg_colour_kernel")), name
        print(kernel, r, r.spills)
        assert r.scratch == 0 and r.spills == (0, 0), (kernel, r, r.spills)
        seen[kernel] = r
    assert sorted(seen) == ["jpeg_split_scan_kernel", "jpeg_split_sync_kernel", "jpeg_split_write_kernel"]
    staged = GROUP * SUB + 32
    assert staged + 4 * ctypes.sizeof(_lib.JpegHuff) <= seen["jpeg_split_write_kernel"].lds <= seen["jpeg_split_sync_kernel"].lds <= 16384
    assert seen["jpeg_split_scan_kernel"].lds == 4 * 4 * 256
