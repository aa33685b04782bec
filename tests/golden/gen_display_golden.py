#!/usr/bin/env python3
"""Display-mode fixtures: the reference's own eval.prep_display on the inputs of display_cases.py (build container only).

    python tests/golden/gen_display_golden.py        # writes tests/golden/display_cases.npz

prep_display runs on this CPU with gen_golden.install_stubs(), a stub torch.utils.tensorboard, torch.Tensor.cuda and
torch.cuda.synchronize as no-ops and get_color's on_gpu=None read as "cpu".  Boxes and text are off
(--display_bboxes=False --display_text=False): they are cv2 drawing, which is not pinned here.  Per case the file holds the
detections, and either the whole output (small frames) or one CRC32 per output row plus 4096 sampled pixels.
"""
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import display_cases  # noqa: E402
import gen_golden  # noqa: E402

N_SAMPLES = 4096


def row_crcs(img):
    return np.array([zlib.crc32(np.ascontiguousarray(img[y]).tobytes()) for y in range(img.shape[0])], dtype=np.uint32)


def sample_index(shape, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, shape[0], N_SAMPLES), rng.integers(0, shape[1], N_SAMPLES)], 1).astype(np.int32)


def load_reference():
    gen_golden.install_stubs()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.synchronize = lambda *a, **k: None
    from datasets.config import cfg, set_cfg
    set_cfg("STMask_plus_resnet50_config")
    import eval as ref_eval
    ref_eval.parse_args(["--display_bboxes=False", "--display_text=False"])
    get_color = ref_eval.get_color

    def get_color_cpu(j, color_type, on_gpu=None, undo_transform=True):
        return get_color(j, color_type, on_gpu="cpu" if on_gpu is None else on_gpu, undo_transform=undo_transform)

    ref_eval.get_color = get_color_cpu
    return cfg, ref_eval


def main():
    cfg, ref_eval = load_reference()
    out = {"COLORS": np.array(cfg.COLORS, dtype=np.uint8), "eval_conf_thresh": np.float64(cfg.eval_conf_thresh),
           "top_k": np.int64(ref_eval.args.top_k), "score_threshold": np.float64(ref_eval.args.score_threshold)}
    for name, spec in display_cases.CASES.items():
        mode = spec[0]
        d = display_cases.detections(spec)
        meta = display_cases.meta(spec)
        det = {"box": torch.from_numpy(d["box"]), "score": torch.from_numpy(d["score"]), "class": torch.from_numpy(d["class"]),
               "box_ids": torch.from_numpy(d["box_ids"]), "mask": torch.from_numpy(d["mask_u8"]).float() / 256.0,
               "mask_coeff": torch.zeros(len(d["score"]), 32), "proto": torch.zeros(1)}
        cfg.preserve_aspect_ratio = mode == "source"
        ref_eval.color_cache.clear()
        if mode == "source":
            img = torch.from_numpy(display_cases.source_frame(spec))
        else:
            img = torch.from_numpy(display_cases.network_input(spec))
        res = ref_eval.prep_display({"detection": det, "net": None}, img, img_meta=dict(meta), undo_transform=mode == "reference")
        res = np.ascontiguousarray(res)
        for k in ("box", "score", "class", "box_ids", "mask_u8"):
            out[f"{name}/{k}"] = d[k]
        out[f"{name}/shape"] = np.array(res.shape, dtype=np.int32)
        if spec[6]:
            out[f"{name}/out"] = res
        else:
            idx = sample_index(res.shape, spec[5])
            out[f"{name}/row_crc"] = row_crcs(res)
            out[f"{name}/sample_yx"] = idx
            out[f"{name}/sample_px"] = res[idx[:, 0], idx[:, 1]]
        print(f"{name}: {mode} {res.shape} rows={len(d['score'])}")
    path = os.path.join(HERE, "display_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote display_cases.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
