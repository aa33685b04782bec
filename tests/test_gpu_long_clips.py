"""Long clips against the reference's own eval forward (gen_golden.py gen_model_full_tf): the benchmark's 16-frame full-size clip on R50-FCA and
R50-FCB(ada), and a 12-frame clip with gaps, through BatchedClipPipeline on the planar fp16x2 graph driven as bench.py's Runner drives it (trunks
replayed from HIP graphs, PREFETCH_DEPTH frames of look-ahead, two clips per step).  These are the frames where the tracker's age-out
(tracked_mask <= 10), the x0.95 score decay under eval_conf_thresh and the > 1 pixel rule first decide (track_TF.py:158-165), and where rows are
matched again after frames without a match.  Checked per frame: the whole tracker state, the reported set from detections() and from the packed
step() output (keep_flags_bits + pack_tracked kernels)."""
import pytest
import torch

from conftest import load_golden
from long_clip_check import golden_clips, rules_decided, run_long_clip
from stmask_amd import synthetic
from test_gpu_parity import build, report

pytestmark = pytest.mark.gpu

# (config, fixture, keep conditions that decide alone for some row of the fixture, frames where the companion clip is all-zero too)
LONG = [("STMask_plus_resnet50_config", "model_full_tf16_r50_fca.npz", {2, 3}, ()),
        ("STMask_plus_resnet50_ada_config", "model_full_tf16_r50_ada.npz", {1, 2}, ()),
        ("STMask_plus_resnet50_config", "model_full_tf_gaps_r50_fca.npz", {2, 3}, (6,))]


@pytest.mark.parametrize("name,fixture,decides,zero_companion", LONG, ids=["long_r50_fca", "long_r50_ada", "gaps_r50_fca"])
def test_long_clip_tracker_matches_reference(name, fixture, decides, zero_companion):
    """Every non-excused state row (rows whose outcome hangs on a comparison closer than the golden's fragile_eps in the reference's own values are
    recorded in the golden and excused from then on): count, classes and frames-since-match counters exact, boxes / scores 5e-6, mask sums and the
    > 1 pixel decision; reported ids / classes exact, boxes / scores 5e-6, from detections() and from the packed output.  The gaps clip: no detection
    on frame 0 (clip 0 only), the first detections on frame 1, frames 6-7 without detections (frame 6 in both clips: a step with no detection at
    all), re-matching from frame 8.  Across the fixtures the golden proves that each keep condition decided something on its own."""
    from stmask_amd.pipeline import BatchedClipPipeline
    g = load_golden(fixture)
    decided, rematched = rules_decided(g)
    assert decided >= decides and rematched > 0, (fixture, decided, rematched)
    T = int(g["n_frames"])
    net = build(name, bg_bias=synthetic.BENCH_BG_BIAS, planar="fp16x2")
    clips = golden_clips(g, zero_companion).cuda()
    pipe = BatchedClipPipeline(net, 2)
    pipe.use_graph = True
    depth = max(2, pipe.PREFETCH_DEPTH)
    frames = [clips[:, t].contiguous(memory_format=torch.channels_last) for t in range(T)]
    rep = run_long_clip(fixture, pipe, g, frames, next_depth=depth, zero_companion=zero_companion)
    assert pipe.graph_active, "the trunk was not replayed from HIP graphs"
    assert not pipe.fell_back
    report(f"long_clip_{fixture[:-4]}", **rep)
