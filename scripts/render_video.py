#!/usr/bin/env python3
"""Annotated frames of a synthetic clip as PNG files: the clip runs through VideoBatcher (one slot) and every frame's tracked instances are
drawn on the device in display source mode (stmask_amd.display), masks and box outlines; PIL writes the images.  A demonstration tool,
not a test.  The synthetic weights and frames make arbitrary but tracked instances.

usage: python scripts/render_video.py [--frames 8] [--size 720 1280] [--out render_out]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from scripts.run_video_demo import synthetic_video_u8  # noqa: E402
from scripts.serve_videos import build_net  # noqa: E402
from stmask_amd.serve import VideoBatcher  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280])
    ap.add_argument("--config", default="STMask_plus_resnet50_config")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="render_out")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    net = build_net(a.config, "cuda")
    video = synthetic_video_u8(1, a.frames, a.size[0], a.size[1], seed=a.seed)[0].cuda()   # taken as BGR, as preprocess.py takes frames

    def save(video_id, frame_id, img):
        path = os.path.join(a.out, f"video{video_id}_frame{frame_id:04d}.png")
        Image.fromarray(img.flip(2).cpu().numpy()).save(path)                            # BGR -> RGB for the PNG
        print(path)

    VideoBatcher(net, 1).run([(0, video)], on_frame=save)
