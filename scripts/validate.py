#!/usr/bin/env python3
"""Validate a saved checkpoint: what scripts/train_ytvis.py does every --validation_interval iterations, for a file on disk.  The weights are
loaded into an STMask, an stmask_amd.validate.InferenceTwin of it serves the split (stmask_amd.datasets.YTVISValSet: frames are read when the
batcher asks for them), and the results JSON is written to the checkpoint's path with .pth replaced by .json (or --out).  When the annotation
file has annotations the results are scored (eval_utils.calc_metrics: video mask AP on the device) and the mAP file is written beside it as
.txt; the official valid split has none and only the JSON is written (eval.py:566-573).
    python scripts/validate.py CKPT ANN IMG_PREFIX [--config STMask_plus_resnet50_config] [--slots 8] [--planes fp16x2] [--out results.json]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("ckpt")
    ap.add_argument("ann")
    ap.add_argument("img_prefix")
    ap.add_argument("--config", default="STMask_plus_resnet50_config")
    ap.add_argument("--slots", type=int, default=8, help="videos in flight")
    ap.add_argument("--planes", choices=["fp16x2", "bf16x3", "fp16x1"], default="fp16x2", help="plane format of the inference graph")
    ap.add_argument("--decode", choices=["host", "device"], default="host",
                    help="where the frames' JPEG files are decoded: PIL on the host, or the MI355X (stmask_amd.jpeg)")
    ap.add_argument("--decode-split", dest="decode_split", choices=["auto", "all"], default=None,
                    help="with --decode device: decode a file without restart markers at many places at once (stmask_amd.jpeg split=): every such "
                         "file, or those of jpeg.SPLIT_MIN_BYTES or more; default: one wavefront a file")
    ap.add_argument("--out", default=None, help="the results JSON (default: CKPT with .pth replaced by .json); the mAP file lies beside it")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    from stmask_amd import datasets, validate
    from stmask_amd.config import get_cfg
    from stmask_amd.model import STMask
    net = STMask(get_cfg(args.config))
    net.load_weights(args.ckpt)
    net = net.to("cuda:0").eval()
    out_json, metrics_file = validate.result_paths(args.ckpt)
    if args.out:
        out_json, metrics_file = args.out, os.path.splitext(args.out)[0] + ".txt"
    dataset = datasets.YTVISValSet(args.ann, args.img_prefix, read_ahead=8, decode=args.decode, decode_split=args.decode_split)
    scored = dataset.has_annotations
    twin = validate.InferenceTwin(net, planes=args.planes)
    metrics = validate.validation(twin, dataset, out_json, ann_file=args.ann if scored else None, metrics_file=metrics_file if scored else None,
                                  n_slots=args.slots, decode=args.decode)
    dataset.close()
    print(f"results: {out_json}" + (f"   metrics: {metrics_file}" if scored else "   (no annotations: nothing scored)"))
    return metrics


if __name__ == "__main__":
    main()
