"""Data-parallel training end to end on the GPU box: two ranks under torch.distributed.run, both on device 0 with the gloo exchange (the form of
tests/test_gpu_bench_ranks.py), through tests/dp_train_worker.py -- seeded gradients against the restatement, two train_step_dp steps of the
real net, a batch that overflows on one rank alone -- then scripts/train_ytvis.py --gpus 2 with a resume, and the same first two checks over
RCCL where the machine has two devices.  The net's backward scatters with atomics and is not reproducible from run to run, so no test compares
the net's gradients with a recomputation: only exact properties are checked."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dp_restate as D
import train_data_cases as C
from dp_train_worker import SGD, SIZES
from stmask_amd import checkpoint

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = ["BIoU", "M", "C", "center", "B_shift", "M_shift", "T"]


def run_ranks(out, backend, share, parts):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "dp_train_worker.py"), out, "--backend", backend, "--parts", parts] + (["--share-gpu"] if share else [])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-3000:]
    got = [torch.load(os.path.join(out, f"rank{r}.pt")) for r in range(2)]
    print("\nseconds per part: " + "  ".join(f"rank {r['rank']} {r['seconds']}" for r in got))
    return got


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return run_ranks(str(tmp_path_factory.mktemp("dp")), "gloo", True, "seeded,net,overflow")


def check_seeded(ranks):
    a, b = ranks
    assert a["inv_world"] == b["inv_world"] == 0.5 and a["seeded_tail0"] == b["seeded_tail0"] == 0.25 + 1.25
    for i, n in enumerate(SIZES):
        g0, g1 = a["seeded_g"][i].numpy(), b["seeded_g"][i].numpy()
        assert n == 0 or not np.array_equal(g0, g1)
        # (g0 + g1) * 0.5: the sum of two fp32 values does not depend on the order, so the restatement is exact
        p1, m1, _ = D.finish_f32(a["seeded_p0"][i].numpy(), g0 + g1, a["seeded_m0"][i].numpy(), 2, SGD["lr"], SGD["momentum"], SGD["weight_decay"])
        for r in ranks:
            assert np.array_equal(D.bits(r["seeded_p1"][i].numpy()), D.bits(p1)), ("parameter", i, n, r["rank"])
            assert np.array_equal(D.bits(r["seeded_m1"][i].numpy()), D.bits(m1)), ("momentum", i, n, r["rank"])
    for r in ranks:
        assert r["seeded_counters"] == (1, 0) and not bool(r["seeded_arena_after"].view(torch.int32).any())


def check_net(ranks):
    a, b = ranks
    for r in ranks:
        assert r["net_mismatch"] is None, f"rank {r['rank']}: {r['net_mismatch']} differs between the ranks after two steps"
        assert r["net_momentum_mismatch"] is None, f"rank {r['rank']}: the momentum of {r['net_momentum_mismatch']} differs between the ranks"
        assert r["net_counters"] == (2, 0) and r["net_arena_zero"] and sorted(r["net_keys"]) == sorted(TERMS)
        assert r["net_moved"] > r["net_tensors"] - 8
        # one solo step on the rank's own batch gives other parameters: the exchange happened
        assert r["net_differs_from_solo"] > r["net_tensors"] // 2, (r["net_differs_from_solo"], r["net_tensors"])
    assert a["net_local"][0] != b["net_local"][0]                        # different batches
    assert all(np.isfinite(v) for r in ranks for terms in r["net_local"] for v in terms.values())
    for step in range(2):
        for i, k in enumerate(a["net_keys"]):
            want = (np.float32(a["net_local"][step][k]) + np.float32(b["net_local"][step][k])) * np.float32(0.5)
            for r in ranks:
                assert np.float32(r["net_logged"][step][k]) == want, (step, k, r["rank"])
                assert np.float32(r["net_log_rows"][step][i]) == want, (step, k, r["rank"])


def test_seeded_gradients_are_averaged_and_stepped_bit_equal_to_the_restatement_on_both_ranks(ranks):
    check_seeded(ranks)


def test_two_steps_of_the_real_net_leave_the_ranks_bit_identical_and_log_the_mean(ranks):
    check_net(ranks)


def test_an_overflow_on_one_rank_is_skipped_on_both(ranks):
    a, b = ranks
    assert np.isfinite(a["overflow_local_total"]) and not np.isfinite(b["overflow_local_total"])      # rank 1 alone overflowed
    for r in ranks:
        assert not np.isfinite(r["overflow_logged_total"])
        assert r["overflow_changed"] == [] and r["overflow_momentum_zero"]
        assert r["overflow_counters"] == (0, 1)
        assert r["overflow_arena_zero"]


# ---- scripts/train_ytvis.py --gpus 2 --------------------------------------------------------------------------------------------------------
def write_dataset(root):
    """train_data_cases' hand-built annotation dict and its seeded frames, as files."""
    from PIL import Image
    ann = C.annotations()
    read = C.frame_reader()
    for v in ann["videos"]:
        for name in v["file_names"]:
            path = os.path.join(root, "frames", name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(np.ascontiguousarray(read(name)[:, :, ::-1])).save(path, quality=95)
    with open(os.path.join(root, "ann.json"), "w") as fh:
        json.dump(ann, fh)
    return os.path.join(root, "ann.json"), os.path.join(root, "frames")


def test_train_script_with_two_ranks_saves_once_and_resumes(tmp_path):
    ann, frames = write_dataset(str(tmp_path))
    weights = str(tmp_path / "weights")
    cfg = "STMask_plus_resnet50_ada_config"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_ytvis.py"), ann, frames, "--config", cfg, "--gpus", "2", "--backend", "gloo",
           "--share-gpu", "--batch_size", "2", "--save_folder", weights, "--save_interval", "0", "--max_pos", "256",
           "--log", str(tmp_path / "train.jsonl")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    first = subprocess.run(cmd + ["--iters", "3"], env=env, capture_output=True, text=True, timeout=900)
    assert first.returncode == 0, first.stderr[-3000:]
    saved = sorted(os.listdir(weights))
    assert len(saved) == 2 and saved[1] == saved[0] + ".state" and saved[0].endswith("_3.pth"), saved        # one checkpoint, rank 0's
    assert first.stdout.count("saving ") == 1 and "2 ranks (gloo)" in first.stdout
    lines = [json.loads(l) for l in open(str(tmp_path / "train.jsonl"))]
    assert [l["iter"] for l in lines] == [0, 1, 2]
    state = torch.load(os.path.join(weights, saved[1]), map_location="cpu")
    assert state["iteration"] == 3 and sum(state["counters"]) == 3 and sorted(state["loader"]) == ["batch", "epoch", "seed"]
    again = subprocess.run(cmd + ["--iters", "5", "--resume", "latest"], env=env, capture_output=True, text=True, timeout=900)
    assert again.returncode == 0, again.stderr[-3000:]
    assert f"resumed {os.path.join(weights, saved[0])} at iteration 3" in again.stdout
    assert [l["iter"] for l in (json.loads(l) for l in open(str(tmp_path / "train.jsonl")))] == [0, 1, 2, 3, 4]
    assert checkpoint.parse_path(checkpoint.get_latest(weights, get_name(cfg)))[2] == 5


def get_name(cfg):
    from stmask_amd.config import get_cfg
    return get_cfg(cfg).name


# ---- RCCL, where there are two devices ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="the RCCL exchange needs two devices")
def test_the_rccl_exchange_on_two_devices(tmp_path):
    got = run_ranks(str(tmp_path), "nccl", False, "seeded,net")
    check_seeded(got)
    check_net(got)
