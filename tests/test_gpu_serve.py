"""VideoBatcher on the MI355X: a queue of five synthetic uint8 videos (lengths 3, 7, 2, 5, 4; two source sizes) served in 2 and in 8 slots,
with graph-replayed trunks and look-ahead, gives the records of every video run alone (same net, same seeded weights, the flow of
scripts/run_video_demo.py):
* alone in a pipeline of the same width, in the slot the queue gave it, the other slots idle: same objects, categories and RLE strings, scores within
  1e-6;
* alone through BatchedClipPipeline(net, 1): same objects and categories, scores within 1e-5.  The trunk's per-image outputs depend on the batch
  size at the 1e-6 level (measured on the MI355X: head outputs of one image in a batch of 3 and of 1 differ by up to 6.7e-6), which can move a
  mask's edge pixel at 720p -- so the RLE strings are compared at equal batch width."""
import pytest
import torch

from scripts.run_video_demo import synthetic_video_u8
from stmask_amd import eval_utils, output_utils, preprocess, synthetic
from stmask_amd.config import get_cfg
from stmask_amd.fuse import optimize_for_inference
from stmask_amd.model import STMask
from stmask_amd.pipeline import BatchedClipPipeline
from stmask_amd.serve import VideoBatcher

pytestmark = pytest.mark.gpu

LENGTHS = [3, 7, 2, 5, 4]
SIZES = [(720, 1280), (480, 854)]

_cache = {}


def demo_net():
    if "net" not in _cache:
        net = STMask(get_cfg("STMask_plus_resnet50_config"))
        net.eval()
        synthetic.fill_state_dict(net, seed=0, bg_bias=4.7)
        net = net.to("cuda")
        optimize_for_inference(net, planar=True)
        net = net.to(memory_format=torch.channels_last)
        net.TemporalNet = net.TemporalNet.to(memory_format=torch.contiguous_format)
        _cache["net"] = net
    return _cache["net"]


def queue():
    vids = []
    for i, T in enumerate(LENGTHS):
        h, w = SIZES[i % 2]
        v = synthetic_video_u8(1, T, h, w, seed=40 + i)[0]
        vids.append((100 - i, v.pin_memory() if i == 3 else v.cuda()))     # one video stays in pinned host memory
    return vids


def alone_in_slot(net, width, slot, video_id, video):
    """The video alone in slot `slot` of a `width`-clip pipeline, the other slots idle, through VideoBatcher's pre-processing and output stage."""
    from stmask_amd.serve import device_prep
    pipe = BatchedClipPipeline(net, width)
    classes = ["class_%d" % i for i in range(1, net.cfg.num_classes)]
    results = []
    with torch.no_grad():
        for t in range(video.shape[0]):
            x, metas = device_prep([video[t] if b == slot else None for b in range(width)], [t if b == slot else None for b in range(width)])
            pipe.step(x, is_first=(t == 0), active=[b == slot for b in range(width)])
            det = pipe.detections()[slot]
            m = dict(metas[slot], video_id=video_id, frame_id=t)
            if det and det["box"].shape[0]:
                results.append(eval_utils.bbox2result_with_id(output_utils.postprocess_ytbvis({"detection": det}, m), m, classes))
            else:
                results.append({"video_id": video_id, "frame_id": t})
    return eval_utils.video_records(results)


def alone(net, video_id, video):
    """scripts/run_video_demo.py:run for one video, batch size 1."""
    pipe = BatchedClipPipeline(net, 1)
    classes = ["class_%d" % i for i in range(1, net.cfg.num_classes)]
    results = []
    with torch.no_grad():
        for t in range(video.shape[0]):
            x, meta = preprocess.preprocess_eval_frames(video[t:t + 1].cuda(), idx=t)
            pipe.step(x.contiguous(memory_format=torch.channels_last), is_first=(t == 0))
            det = pipe.detections()[0]
            m = dict(meta, video_id=video_id)
            if det and det["box"].shape[0]:
                post = output_utils.postprocess_ytbvis({"detection": det}, m)
                results.append(eval_utils.bbox2result_with_id(post, m, classes))
            else:
                results.append({"video_id": video_id, "frame_id": t})
    return eval_utils.video_records(results)


def test_serve_queue_equals_each_video_alone(tmp_path):
    from stmask_amd.serve import schedule
    net = demo_net()
    vids = queue()
    order = sorted(range(len(vids)), key=lambda i: vids[i][0])
    single = []
    for i in order:
        single += alone(net, *vids[i])
    assert len(single) > 5
    for slots in (2, 8):
        slot_of = {}
        for row in schedule(LENGTHS, slots):
            for b, c in enumerate(row):
                if c is not None:
                    slot_of[c[0]] = b
        expect = []
        for i in order:
            expect += alone_in_slot(net, slots, slot_of[i], *vids[i])
        vb = VideoBatcher(net, slots)
        out_file = str(tmp_path / f"results_{slots}.json") if slots == 2 else None
        got = vb.run(vids, out_file=out_file)
        assert vb.pipe.graph_active, slots                                   # the trunks were replayed from graphs
        assert [r["video_id"] for r in got] == [r["video_id"] for r in expect] == [r["video_id"] for r in single], slots
        for g, e, o in zip(got, expect, single):
            assert g["category_id"] == e["category_id"] == o["category_id"], (slots, g["video_id"])
            assert abs(g["score"] - e["score"]) <= 1e-6 and abs(g["score"] - o["score"]) <= 1e-5, (slots, g["video_id"])
            assert g["segmentations"] == e["segmentations"], (slots, g["video_id"])
        assert 0 < vb.occupancy() <= 1
        if out_file:
            import json
            assert json.load(open(out_file)) == got
