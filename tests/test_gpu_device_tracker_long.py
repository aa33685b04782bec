"""The long clips of test_gpu_long_clips.py with the tracker on the device (BatchedClipPipeline(device_tracker=True)): the same fixtures, driver
(long_clip_check.run_long_clip, unchanged), tolerances and excused-row cap.  Holds the resolve kernel, the device-side counters and the late row
counts to the reference's own 16-frame and gaps clips: age-out, score decay, re-matching after frames without a match, a step with no detection
at all."""
import pytest
import torch

from conftest import load_golden
from long_clip_check import golden_clips, rules_decided, run_long_clip
from stmask_amd import synthetic
from test_gpu_long_clips import LONG
from test_gpu_parity import build, report

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,fixture,decides,zero_companion", LONG, ids=["long_r50_fca", "long_r50_ada", "gaps_r50_fca"])
def test_long_clip_device_tracker_matches_reference(name, fixture, decides, zero_companion):
    from stmask_amd.pipeline import BatchedClipPipeline
    g = load_golden(fixture)
    decided, rematched = rules_decided(g)
    assert decided >= decides and rematched > 0, (fixture, decided, rematched)
    T = int(g["n_frames"])
    net = build(name, bg_bias=synthetic.BENCH_BG_BIAS, planar="fp16x2")
    clips = golden_clips(g, zero_companion).cuda()
    pipe = BatchedClipPipeline(net, 2, device_tracker=True)
    pipe.use_graph = True
    depth = max(2, pipe.PREFETCH_DEPTH)
    frames = [clips[:, t].contiguous(memory_format=torch.channels_last) for t in range(T)]
    rep = run_long_clip(fixture + "/device_tracker", pipe, g, frames, next_depth=depth, zero_companion=zero_companion)
    assert pipe.graph_active, "the trunk was not replayed from HIP graphs"
    assert pipe.device_tracker and not pipe.fell_back
    report(f"long_clip_device_tracker_{fixture[:-4]}", **rep)
