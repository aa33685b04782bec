"""Inputs of the training-batch tests, made with numpy at test time: run lists for every source size (the edge cases of the RLE -> target-size
rendering), seeded uint8 frames, boxes that touch the clip, and a small hand-built YouTube-VIS annotation dict that walks every branch of the
dataset's parse.  Not a test module: imported by the training-batch tests."""
import numpy as np

from stmask_amd.output_utils import rle_counts_to_string

SIZE, DIVISOR = (40, 24), 32                                   # (w, h) -> Hp, Wp = 32, 64: padding in both directions
SOURCES = [(24, 40), (48, 80), (37, 53), (15, 22), (50, 30)]   # identity, factor 2, non-integer shrinking, enlarging, portrait
REAL_SOURCE, REAL_SIZE = (720, 1280), (640, 360)              # the reference's own shapes: padded to 384 x 640
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def counts_of_mask(mask):
    """Run lengths of a [h, w] mask, column-major, starting with a run of zeros (possibly of length 0)."""
    flat = np.asarray(mask, dtype=bool).reshape(-1, order="F")
    edges = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
    cnts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return ([0] + cnts) if flat.size and flat[0] else cnts


def blob(H0, W0, rng, k=3):
    """The union of k random ellipses."""
    ys, xs = np.mgrid[0:H0, 0:W0]
    m = np.zeros((H0, W0), dtype=bool)
    for _ in range(k):
        cy, cx = rng.uniform(0, H0), rng.uniform(0, W0)
        ry, rx = rng.uniform(0.08, 0.35) * H0 + 1, rng.uniform(0.08, 0.35) * W0 + 1
        m |= ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
    return m


def run_lists(H0, W0, seed=0):
    """{name: list of run lengths} for one source size."""
    rng = np.random.default_rng(1000 * H0 + W0 + seed)
    n = H0 * W0
    out = {"empty": [n], "full": [0, n], "last_pixel": [n - 1, 1],
           # zero-length runs in the middle (of ones, then of zeros and ones together) and at the end
           "zero_runs": [7, 0, 5, 9, 0, 0, 4, 11, n - 36, 0],
           "blob_a": counts_of_mask(blob(H0, W0, rng)), "blob_b": counts_of_mask(blob(H0, W0, rng, 5)),
           "noise": counts_of_mask(rng.random((H0, W0)) < 0.5)}
    if (H0, W0) == (48, 80):
        out["stripes_1px"] = [1] * n                                                              # 3840 runs: 60 scan chunks, 12-step searches
        out["checker_1px"] = counts_of_mask((np.add.outer(np.arange(H0), np.arange(W0)) & 1) == 1)
    for name, c in out.items():
        assert sum(c) == n and min(c) >= 0, name
    return out


def rle(counts, H0, W0, compressed=False):
    return {"size": [H0, W0], "counts": rle_counts_to_string([int(c) for c in counts]).decode() if compressed else [int(c) for c in counts]}


def frame(H0, W0, seed=0):
    """A seeded uint8 [H0, W0, 3] frame: smooth gradients plus noise, so that the bilinear taps and the flip both matter."""
    rng = np.random.default_rng(77 * H0 + W0 + seed)
    ys, xs = np.mgrid[0:H0, 0:W0]
    base = np.stack([255.0 * xs / max(W0 - 1, 1), 255.0 * ys / max(H0 - 1, 1), 127.0 + 0 * xs], -1)
    return np.clip(base + rng.normal(0, 40, (H0, W0, 3)), 0, 255).astype(np.uint8)


def boxes_for(H0, W0):
    """float32 [G, 4] (x1, y1, x2, y2) source-pixel boxes: inside, touching every clip bound, and at x = 0 and x = W0 - 1 (the flip's ends)."""
    return np.array([[3.3, 2.7, W0 * 0.6 + 0.4, H0 * 0.7 + 0.2],
                     [-4.5, -2.25, W0 * 0.5, H0 * 0.5],                  # clipped at 0
                     [W0 * 0.4, H0 * 0.3, W0 + 6.5, H0 + 3.75],          # clipped at w / h
                     [0.0, 0.0, W0 - 1.0, H0 - 1.0],                     # the whole frame
                     [0.0, 1.0, 0.0, 2.0],                               # a box at x = 0
                     [W0 - 1.0, 1.0, W0 - 1.0, 2.0],                     # a box at x = W0 - 1
                     [1 / 3, 2 / 3, W0 / 3, H0 / 7]], dtype=np.float32)


# ---------------------------------------------------------------------------------------------- a hand-built YouTube-VIS annotation dict
VIDEOS = [(10, 37, 53, 5), (20, 48, 80, 3), (30, 50, 30, 1)]       # id, height, width, frames
CAT_IDS = [7, 3, 12]                                                # labels 1, 2, 3 in this order


def _rect(H0, W0, x, y, bw, bh):
    m = np.zeros((H0, W0), dtype=bool)
    m[int(y):int(y + bh), int(x):int(x + bw)] = True
    return m


def _track(aid, vid, cat, H0, W0, per_frame, crowd=0, compressed=False):
    """per_frame: None, or (x, y, w, h) (floats), or ((x, y, w, h), area) to force an area."""
    bboxes, areas, segs = [], [], []
    for f in per_frame:
        if f is None:
            bboxes.append(None), areas.append(None), segs.append(None)
            continue
        box, area = f if isinstance(f[0], tuple) else (f, None)
        m = _rect(H0, W0, *box)
        bboxes.append([float(v) for v in box])
        areas.append(int(m.sum()) if area is None else area)
        segs.append(rle(counts_of_mask(m), H0, W0, compressed))
    return {"id": aid, "video_id": vid, "category_id": cat, "iscrowd": crowd, "bboxes": bboxes, "areas": areas, "segmentations": segs}


def annotations():
    """3 videos of different sizes.  Video 10: frame 2 has no objects (track 101 has bbox None there, track 102 has left); track 103 has area 0 in
    frame 3.  Video 20 carries a crowd track next to a plain one, the plain one as compressed strings.  Video 30 has a single frame."""
    vids = [{"id": v, "height": h, "width": w, "length": n, "file_names": [f"v{v}/{f:05d}.jpg" for f in range(n)]} for v, h, w, n in VIDEOS]
    anns = [
        _track(101, 10, 3, 37, 53, [(3.3, 2.2, 10.7, 8.1), (4.1, 2.9, 10.2, 8.4), None, (6.0, 4.0, 11.0, 9.0), (7.5, 4.5, 11.25, 9.5)]),
        _track(102, 10, 7, 37, 53, [(30.0, 20.0, 12.5, 9.0), (31.0, 21.0, 12.0, 8.0), None, None, None]),
        _track(103, 10, 12, 37, 53, [None, None, None, ((20.0, 5.0, 6.0, 6.0), 0), (21.0, 6.0, 6.0, 6.0)]),
        _track(201, 20, 7, 48, 80, [(10.0, 8.0, 30.0, 20.0), (12.0, 9.0, 30.0, 21.0), (14.0, 10.0, 31.0, 22.0)], compressed=True),
        _track(202, 20, 3, 48, 80, [(50.0, 5.0, 20.0, 30.0)] * 3, crowd=1),
        _track(301, 30, 12, 50, 30, [(5.0, 10.0, 12.0, 25.0)]),
    ]
    return {"videos": vids, "categories": [{"id": c, "name": f"c{c}"} for c in CAT_IDS], "annotations": anns}


def frame_reader():
    """path -> the seeded frame of that video and index (what tests hand to YTVISTrainSet instead of a decoder)."""
    frames = {f"v{v}/{f:05d}.jpg": frame(h, w, seed=100 * v + f) for v, h, w, n in VIDEOS for f in range(n)}
    return frames.__getitem__
