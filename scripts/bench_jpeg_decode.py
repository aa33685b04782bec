#!/usr/bin/env python3
"""What decoding JPEG frames on the MI355X (stmask_amd.jpeg, csrc/jpeg_decode.hip) is worth against the unchanged host path, in one job.  A
measuring tool, not a test.  Files: seeded synthetic 720 x 1280 frames (a smooth field plus noise), quality 90, 4:2:0, encoded with PIL here.

1. Batches of 4, 16, 32 and 64 frames, --rounds rounds alternating:
     host 1 thread    PIL decode of every file, one after the other, then datasets.upload_frames
     host 8 threads   the same decodes on a pool of 8 threads (PIL releases the GIL while it decodes), then datasets.upload_frames
     device           jpeg.decode_batch(check="deferred") end to end (parse, pinned blob, one copy, three launches), wall clock around a device
                      synchronise; and each launch alone from device events over a blob already uploaded
   plus the bytes copied to the device on both sides.
2. datasets.collate_device end to end both ways at 2, 8 and 16 clips: records that hold decoded frames (the decode with PIL on 1 thread is
   timed in front of it, as a loader without workers pays it) against records of CompressedFrames.
3. serve.VideoBatcher at --slots slots over datasets.YTVISValSet with a frame_reader that serves the files' bytes from memory: host decode with
   read_ahead 0 and 8 against decode="device" (R50 FCA, batched output, warm batchers).
4. Part 1's device rows over the same frames re-encoded with one restart interval per MCU row: what parallelism inside an image is worth to the
   entropy launch, which otherwise has one wavefront per frame.

5. --split all|auto: a third contestant in parts 1 to 3, in the same alternating rounds -- decode_batch(split=...), which decodes a file without
   restart markers at many places at once (csrc/jpeg_split.hip) -- beside the serial device path and PIL, which stay the baselines.  Part 4 is
   left out, and the default --out is profiles/bench_jpeg_split.txt.  Part 6 then looks for the crossover: the launches of the entropy stage alone,
   serial against split="all", over ONE noise file of growing size (from two sub-sequences to a few groups), which is what jpeg.SPLIT_MIN_BYTES
   should be set from.

usage: python scripts/bench_jpeg_decode.py [--frames 4 16 32 64] [--clips 2 8 16] [--rounds 5] [--skip-serving] [--split all|auto]
                                           [--out profiles/bench_jpeg_decode.txt]"""
import argparse
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from stmask_amd import _lib, datasets, jpeg, synthetic  # noqa: E402
from stmask_amd.preprocess import MEANS, STD  # noqa: E402

H0, W0, SIZE, DIVISOR = 720, 1280, (640, 360), 32
DEV = "cuda:0"


def make_files(n, seed, **kw):
    """n distinct JPEG files of H0 x W0 -> [bytes]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H0, 0:W0]
    out = []
    for i in range(n):
        a = np.stack([127 + 100 * np.sin(xx / (40.0 + 7 * c + i)) * np.cos(yy / (50.0 + 3 * i)) for c in range(3)], -1) + rng.normal(0, 12, (H0, W0, 3))
        bio = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(bio, "JPEG", quality=90, subsampling=2, **kw)
        out.append(bio.getvalue())
    return out


def pil_bgr(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(xs):
    return f"{statistics.median(xs):9.2f} ms   (min {min(xs):8.2f}, max {max(xs):8.2f})"


def decode_rows(files, n, rounds, pool, out, host=True, split=None):
    """part 1 (and 4 with host=False) for the first n files"""
    datas = [files[i % len(files)] for i in range(n)]
    t = {k: [] for k in ("host1", "host8", "device", "entropy", "idct", "colour", "split", "split_entropy")}
    jpeg.decode_batch(datas)                                                    # warm-up
    if split:
        jpeg.decode_batch(datas, split=split)
    if host:
        datasets.upload_frames([pil_bgr(d) for d in datas[:2]], DEV)
    for _ in range(rounds):
        if host:
            t["host1"].append(wall_ms(lambda: datasets.upload_frames([pil_bgr(d) for d in datas], DEV))[0])
            t["host8"].append(wall_ms(lambda: datasets.upload_frames(list(pool.map(pil_bgr, datas)), DEV))[0])
        jpeg.reset_counters()
        ms, (frames, status) = wall_ms(lambda: jpeg.decode_batch(datas, DEV, check="deferred"))
        t["device"].append(ms)
        counters = dict(jpeg.COUNTERS)
        status.raise_if_bad()
        if split:
            jpeg.reset_counters()
            ms, (s_frames, s_status) = wall_ms(lambda: jpeg.decode_batch(datas, DEV, check="deferred", split=split))
            t["split"].append(ms)
            s_counters, s_images = dict(jpeg.COUNTERS), jpeg.SPLIT_COUNTERS["images"]
            s_status.raise_if_bad()
            s_redone = len(s_status.redone())
        # the launches alone, one at a time, over a blob already on the device
        batch = jpeg.pack_batch(datas)
        stage = torch.empty(batch.blob_bytes, dtype=torch.uint8, pin_memory=True)
        batch.fill(stage.numpy())
        blob = stage.to(DEV)
        bufs = [torch.empty(k, dtype=d, device=DEV) for k, d in ((batch.out_bytes, torch.uint8), (batch.n_segments, torch.int32), (batch.workspace_bytes, torch.uint8))]
        torch.cuda.synchronize()
        for name, stage_bit in (("entropy", _lib.JPEG_STAGE_ENTROPY), ("idct", _lib.JPEG_STAGE_IDCT), ("colour", _lib.JPEG_STAGE_COLOUR)):
            t[name].append(events_ms(lambda: jpeg.launch_batch(batch, blob, *bufs, "bgr", stage_bit)))
        if split:                                                               # the launches that take the entropy launch's place
            s_batch = jpeg.pack_batch(datas, split=split)
            s_batch.fill(stage.numpy())
            blob = stage.to(DEV)
            torch.cuda.synchronize()
            t["split_entropy"].append(events_ms(lambda: jpeg.launch_batch(s_batch, blob, *bufs, "bgr", _lib.JPEG_STAGE_ENTROPY)))
    same = all(torch.equal(f.cpu(), torch.from_numpy(pil_bgr(d))) for f, d in zip(frames[:2], datas[:2]))
    out(f" {n} frames ({sum(len(d) for d in datas)} file bytes, {batch.n_segments} segments):")
    if host:
        out(f"  host, PIL on 1 thread + upload_frames:       {med(t['host1'])}   {n * H0 * W0 * 3} bytes to the device")
        out(f"  host, PIL on 8 threads + upload_frames:      {med(t['host8'])}")
    out(f"  device, decode_batch end to end:             {med(t['device'])}   {counters['h2d_bytes']} bytes to the device, "
        f"{counters['launches']} launches, {counters['uploads']} upload")
    out(f"    entropy launch, device events:             {med(t['entropy'])}")
    out(f"    idct launch, device events:                {med(t['idct'])}")
    out(f"    upsample + colour launch, device events:   {med(t['colour'])}")
    out(f"  the first two frames equal PIL's bit for bit: {same}")
    if split:
        out(f"  device, decode_batch(split={split!r}) end to end: {med(t['split'])}   {s_counters['h2d_bytes']} bytes to the device, "
            f"{s_counters['launches']} launches, {s_counters['uploads']} upload; {s_images} images split, {s_redone} redone")
        out(f"    the {jpeg.SPLIT_LAUNCHES} launches in the entropy launch's place, device events: {med(t['split_entropy'])}")
        out(f"  every split frame equals the serial path's: {all(torch.equal(x, y) for x, y in zip(s_frames, frames))}")
        out(f"  split / serial device: {statistics.median(t['split']) / statistics.median(t['device']):.3f}   "
            f"entropy launches, split / serial: {statistics.median(t['split_entropy']) / statistics.median(t['entropy']):.3f}" +
            (f"   split / host 1 thread: {statistics.median(t['split']) / statistics.median(t['host1']):.3f}   "
             f"split / host 8 threads: {statistics.median(t['split']) / statistics.median(t['host8']):.3f}" if host else ""))
    if host:
        out(f"  device / host 1 thread: {statistics.median(t['device']) / statistics.median(t['host1']):.3f}   "
            f"device / host 8 threads: {statistics.median(t['device']) / statistics.median(t['host8']):.3f}")


def crossover_rows(rounds, out):
    """part 6: one file alone, its entropy stage serial and split, device events"""
    rng = np.random.default_rng(5)
    out(" data bytes   sub-sequences   serial entropy launch        split, its launches        split / serial")
    for side in (8, 16, 24, 32, 48, 64, 96, 128, 192, 256):
        bio = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8)).save(bio, "JPEG", quality=90, subsampling=2)
        data = bio.getvalue()
        plain, batch = jpeg.pack_batch([data]), jpeg.pack_batch([data], split="all")
        nbytes = int(batch.segments[0].nbytes)
        if not batch.split_images:
            out(f" {nbytes:10d}   not split (one sub-sequence, or the records do not fit)")
            continue
        stage = torch.empty(batch.blob_bytes, dtype=torch.uint8, pin_memory=True)
        bufs = [torch.empty(k, dtype=d, device=DEV) for k, d in ((batch.out_bytes, torch.uint8), (batch.n_segments, torch.int32), (batch.workspace_bytes, torch.uint8))]
        t = {"serial": [], "split": []}
        for r in range(rounds + 1):                                              # the first round warms up
            for name, b in (("serial", plain), ("split", batch)):
                b.fill(stage.numpy())
                blob = stage.to(DEV)
                torch.cuda.synchronize()
                ms = events_ms(lambda: jpeg.launch_batch(b, blob, *bufs, "bgr", _lib.JPEG_STAGE_ENTROPY))
                if r:
                    t[name].append(ms)
        a, b = statistics.median(t["serial"]), statistics.median(t["split"])
        out(f" {nbytes:10d}   {-(-nbytes // _lib.JPEG_SUB_BYTES):13d}   {a:8.3f} ms (max {max(t['serial']):7.3f})   {b:8.3f} ms (max {max(t['split']):7.3f})   {b / a:6.3f}")


def make_records(files, bs, seed, compressed):
    """bs records in YTVISTrainSet's layout over the files; two rectangles per frame"""
    rng = np.random.default_rng(seed)
    h, w, Hp, Wp = datasets.padded_size(SIZE, DIVISOR)
    recs = []
    for c in range(bs):
        flip = bool(rng.random() < 0.5)
        segs, boxes = [], []
        for t in range(2):
            s, b = [], []
            for k in range(2):
                cy, cx = rng.uniform(0.3, 0.7) * H0, rng.uniform(0.3, 0.7) * W0
                m = synthetic._shape_mask(k % 2, cy, cx, 0.15 * H0, 0.12 * W0, H0, W0).numpy()
                ys, xs = np.nonzero(m)
                flat = m.astype(bool).reshape(-1, order="F")
                edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
                cnts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
                s.append({"size": [H0, W0], "counts": ([0] + cnts) if flat[0] else cnts})
                b.append([xs.min(), ys.min(), xs.max(), ys.max()])
            segs.append(s)
            boxes.append(np.array(b, dtype=np.float32))
        data = [files[(2 * c + t) % len(files)] for t in range(2)]
        frames = [jpeg.CompressedFrame(d, name=f"clip {c} frame {t}") for t, d in enumerate(data)] if compressed else data
        recs.append(dict(frames=frames, size=(H0, W0), flip=flip, video_id=c, frame_ids=[0, 1], bboxes=boxes, labels=[np.arange(1, 3, dtype=np.int64)] * 2,
                         obj_ids=[[10 * c, 10 * c + 1]] * 2, segms=segs,
                         img_meta=dict(ori_shape=(H0, W0, 3), img_shape=(h, w, 3), pad_shape=(Hp, Wp, 3), video_id=c, frame_id=1, is_first=False, flip=flip),
                         img_scale=SIZE, size_divisor=DIVISOR, to_rgb=True, mean=MEANS, std=STD))
    return recs


def collate_rows(files, bs, rounds, out, split=None):
    host_recs, dev_recs = make_records(files, bs, bs, False), make_records(files, bs, bs, True)

    def host_side():
        decoded = [dict(r, frames=[pil_bgr(d) for d in r["frames"]]) for r in host_recs]          # what frame_reader=read_frame does per record
        *batch, status = datasets.collate_device(decoded, DEV, check="deferred")
        return batch, status

    def device_side():
        *batch, status = datasets.collate_device(dev_recs, DEV, check="deferred")
        return batch, status
    def split_side():
        *batch, status = datasets.collate_device(dev_recs, DEV, check="deferred", decode_split=split)
        return batch, status
    host_side(), device_side()
    if split:
        split_side()
    t_host, t_dev, t_split = [], [], []
    for _ in range(rounds):
        ms, (hb, st) = wall_ms(host_side)
        t_host.append(ms)
        st.raise_if_bad()
        ms, (db, st) = wall_ms(device_side)
        t_dev.append(ms)
        st.raise_if_bad()
        if split:
            ms, (sb, st) = wall_ms(split_side)
            t_split.append(ms)
            st.raise_if_bad()
    same = torch.equal(hb[0], db[0]) and all(torch.equal(x, y) for a, b in zip(hb[3], db[3]) for x, y in zip(a, b))
    out(f" {bs} clips ({2 * bs} frames):")
    out(f"  host: PIL on 1 thread + collate_device:      {med(t_host)}")
    out(f"  device: collate_device on CompressedFrames:  {med(t_dev)}")
    out(f"  images and masks of the two sides are the same bytes: {same}   device / host: {statistics.median(t_dev) / statistics.median(t_host):.3f}")
    if split:
        out(f"  device: collate_device(decode_split={split!r}):   {med(t_split)}")
        out(f"  its images are the same bytes: {torch.equal(sb[0], db[0])}   split / device: {statistics.median(t_split) / statistics.median(t_dev):.3f}   "
            f"split / host: {statistics.median(t_split) / statistics.median(t_host):.3f}")


def serving_rows(files, a, out):
    from stmask_amd import validate
    from stmask_amd.config import get_cfg
    from stmask_amd.model import STMask
    net = STMask(get_cfg("STMask_plus_resnet50_config"))
    synthetic.fill_state_dict(net, seed=0, bg_bias=4.7)
    net = net.to(DEV).train()
    rng = np.random.default_rng(0)
    lengths = rng.integers(a.min_frames, a.max_frames + 1, a.videos).tolist()
    by_name, videos = {}, []
    for i, T in enumerate(lengths):
        names = [f"v{i}/{t:05d}.jpg" for t in range(T)]
        by_name.update({n: files[(i + t) % len(files)] for t, n in enumerate(names)})
        videos.append(dict(id=i, height=H0, width=W0, length=T, file_names=names))
    ann = dict(videos=videos, categories=[dict(id=c, name=str(c)) for c in range(1, 41)])
    n_frames = sum(lengths)
    twin = validate.InferenceTwin(net)
    twin.refresh()
    host_reader = lambda n: pil_bgr(by_name[n])                                               # noqa: E731
    sets = {"host decode, read_ahead=0": datasets.YTVISValSet(ann, frame_reader=host_reader, read_ahead=0),
            "host decode, read_ahead=8": datasets.YTVISValSet(ann, frame_reader=host_reader, read_ahead=8),
            "device decode": datasets.YTVISValSet(ann, frame_reader=lambda n: jpeg.CompressedFrame(by_name[n], name=n), decode="device")}
    preps = {"device decode": jpeg.compressed_prep()}
    if a.split:
        name = f"device decode, split={a.split}"
        sets[name] = datasets.YTVISValSet(ann, frame_reader=lambda n: jpeg.CompressedFrame(by_name[n], name=n), decode="device", decode_split=a.split)
        preps[name] = jpeg.compressed_prep(split=a.split)
    batchers = {m: twin.batcher(a.slots, **({"prep": preps[m]} if m in preps else {})) for m in sets}
    results = {}
    for m in sets:                                                                            # warm-up: graph capture, workspaces
        results[m] = twin.run(batchers[m], sets[m].videos())
    torch.cuda.synchronize()
    fps = {m: [] for m in sets}
    for _ in range(a.rounds):
        for m in sets:
            t0 = time.perf_counter()
            twin.run(batchers[m], sets[m].videos())
            torch.cuda.synchronize()
            fps[m].append(n_frames / (time.perf_counter() - t0))
    out(f" {a.videos} videos, {n_frames} frames of {H0} x {W0}, {a.slots} slots, R50 FCA, warm batchers, {a.rounds} alternating rounds (frames/s)")
    for m in sets:
        out(f"  {m:28s} median {statistics.median(fps[m]):8.1f}   min {min(fps[m]):8.1f}   max {max(fps[m]):8.1f}")
    out(f"  records of device decode equal those of host decode: {str(results['device decode']) == str(results['host decode, read_ahead=0'])}")
    if a.split:
        out(f"  records of the split decode equal those of host decode: {str(results[name]) == str(results['host decode, read_ahead=0'])}")
    for s in sets.values():
        s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[4, 16, 32, 64])
    ap.add_argument("--clips", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="distinct files; batches cycle through them")
    ap.add_argument("--videos", type=int, default=12)
    ap.add_argument("--min-frames", type=int, default=8)
    ap.add_argument("--max-frames", type=int, default=16)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--skip-serving", action="store_true")
    ap.add_argument("--only-crossover", action="store_true", help="with --split: part 6 alone")
    ap.add_argument("--split", choices=["all", "auto"], default=None, help="a third contestant: decode_batch(split=...)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "bench_jpeg_split.txt" if a.split else "bench_jpeg_decode.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py measures on the MI355X: no GPU, no numbers")
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out(f"scripts/bench_jpeg_decode.py on {torch.cuda.get_device_name(0)}: {H0} x {W0} quality-90 4:2:0 files ({a.distinct} distinct, seeded), "
        f"{a.rounds} rounds alternating host / device; wall clock around device-synchronised runs unless it says device events; "
        f"{os.cpu_count()} CPUs visible, thread pool of 8" +
        (f"; split={a.split!r}: sub-sequences of {_lib.JPEG_SUB_BYTES} bytes, {_lib.JPEG_SUB_GROUP} a group, {_lib.JPEG_SPLIT_ROUNDS} rounds behind round 0, "
         f"SPLIT_MIN_BYTES {jpeg.SPLIT_MIN_BYTES}" if a.split else ""))
    files = make_files(a.distinct, 0)
    out(f"file sizes: {min(map(len, files))} .. {max(map(len, files))} bytes; a decoded frame is {H0 * W0 * 3} bytes")
    if a.only_crossover:
        out("== 6. the entropy stage of one file alone, serial against split='all', by size (device events)")
        crossover_rows(a.rounds, out)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        raise SystemExit(0)
    with ThreadPoolExecutor(max_workers=8) as pool:
        out("== 1. decode_batch against PIL + upload_frames")
        for n in a.frames:
            decode_rows(files, n, a.rounds, pool, out, split=a.split)
        out("== 2. collate_device end to end")
        for bs in a.clips:
            collate_rows(files, bs, a.rounds, out, split=a.split)
        if not a.skip_serving:
            out("== 3. VideoBatcher over YTVISValSet, files served from memory")
            serving_rows(files, a, out)
        if a.split:
            out("== 6. the entropy stage of one file alone, serial against split='all', by size (device events)")
            crossover_rows(a.rounds, out)
        else:
            out("== 4. the same frames with one restart interval per MCU row (45 segments a frame)")
            rst = make_files(a.distinct, 0, restart_marker_rows=1)
            for n in a.frames:
                decode_rows(rst, n, a.rounds, pool, out, host=False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
