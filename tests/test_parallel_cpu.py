"""Data-parallel training without a GPU: the gradient arena's layout and DataParallelSGD's state dicts, the package-private binding of
csrc/dp_step.h and its refusals (nothing is launched), TrainLoader(shard=...), parallel.exchange between two gloo processes on CPU tensors, the
numpy restatement of the finish pinned to the single-rank step, and the new arguments of scripts/train_ytvis.py."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dp_restate as D
from kernel_resources import kernel_resources
import optim_restate as R
from conftest import ROOT
from stmask_amd import _lib, datasets, optim, parallel
from stmask_amd._lib import StmError
from stmask_amd.optim import DataParallelSGD, GuardedSGD

SHAPES = [(3, 5), (0,), (7,), (2, 1, 3), (4,), (2, 3, 4, 5)]


def cpu_params(seed=0):
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    ps[-1] = torch.nn.Parameter(torch.randn(SHAPES[-1]).contiguous(memory_format=torch.channels_last))     # dense in another order
    return ps


# ---- the arena -------------------------------------------------------------------------------------------------------------------------------
def test_arena_layout_views_pads_and_tail():
    params = cpu_params()
    a = parallel.GradArena(params, n_tail=8)
    assert a.offsets == [0, 16, 16, 24, 32, 36] and a.tail_offset == 36 + 120 and a.flat.numel() == 156 + 8
    assert a.flat.dtype == torch.float32 and not bool(a.flat.any())
    base = a.flat.data_ptr()
    for p, v, off in zip(params, a.views, a.offsets):
        assert v.shape == p.shape and v.stride() == p.stride()
        assert v.untyped_storage().data_ptr() == a.flat.untyped_storage().data_ptr()
        assert v.storage_offset() == off and off % 4 == 0 and base % 16 == 0                  # 16-byte boundaries
        assert v.data_ptr() == (base + 4 * off if p.numel() else 0)                            # torch gives a tensor without elements no address
    assert a.tail.data_ptr() == base + 4 * a.tail_offset and a.tail.numel() == 8
    a.bind_grads()
    assert all(p.grad is v for p, v in zip(params, a.views))
    # autograd accumulates in place: twice the same backward doubles the arena, the views stay bound, the pads stay zero
    for _ in range(2):
        sum((p * (i + 1)).sum() for i, p in enumerate(params)).backward()
    assert all(p.grad is v for p, v in zip(params, a.views))
    for i in range(len(params)):
        assert bool((a.segment(i) == 2.0 * (i + 1)).all()) and a.segment(i).numel() == params[i].numel()
    assert a.pads().numel() == 156 - sum(p.numel() for p in params) and not bool(a.pads().any())
    assert not bool(a.tail.any())
    a.write_tail([torch.tensor(float(i)) for i in range(1, 9)])
    assert a.flat[-8:].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0] and not bool(a.pads().any())
    with pytest.raises(ValueError, match="tail holds 8"):
        a.write_tail([torch.tensor(0.0)] * 9)
    with pytest.raises(ValueError, match="dense float32"):
        parallel.GradArena([torch.nn.Parameter(torch.zeros(4, 6)[:, ::2])])
    with pytest.raises(ValueError, match="dense float32"):
        parallel.GradArena([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    empty = parallel.GradArena([], n_tail=8)
    assert empty.flat.numel() == 8 and empty.pads().numel() == 0


def test_exchange_in_a_world_of_one_is_a_no_op():
    a = parallel.GradArena(cpu_params(), n_tail=8)
    a.flat.copy_(torch.arange(a.flat.numel(), dtype=torch.float32))
    before = a.flat.clone()
    parallel.exchange(a)
    assert torch.equal(a.flat, before)
    assert parallel.first_difference([a.flat]) is None


def test_dp_sgd_owns_two_arenas_and_its_state_dict_is_torch_sgds():
    params = cpu_params()
    params[2].requires_grad_(False)                      # not trainable: no segment
    opt = DataParallelSGD(params, lr=0.02, momentum=0.8, weight_decay=3e-4, world=2, rank=1)
    assert isinstance(opt, GuardedSGD) and opt.inv_world == 0.5 and len(opt.trainable) == 5
    assert opt.grads.offsets == opt.momentum.offsets and opt.momentum.n_tail == 0 and opt.grads.n_tail == 8
    assert params[2].grad is None and all(p.grad is v for p, v in zip(opt.trainable, opt.grads.views))
    for p, m in zip(opt.trainable, opt.momentum.views):
        assert opt.state[p]["momentum_buffer"] is m
    opt.zero_grad()
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is v for p, v in zip(opt.trainable, opt.grads.views))          # a no-op that keeps the views
    for i, m in enumerate(opt.momentum.views):
        m.copy_(torch.randn(m.shape) + i)
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1, 3, 4, 5]
    assert all(list(v) == ["momentum_buffer"] for v in sd["state"].values())
    assert all(v["momentum_buffer"].untyped_storage().data_ptr() != opt.momentum.flat.untyped_storage().data_ptr() for v in sd["state"].values())
    # ... into torch.optim.SGD, which runs on it, and into GuardedSGD
    back = torch.optim.SGD(cpu_params(2), lr=0.5)
    back.load_state_dict(copy.deepcopy(sd))                # torch keeps the tensors it is handed, and its step updates them in place
    bp = back.param_groups[0]["params"]
    assert back.param_groups[0]["lr"] == 0.02 and back.param_groups[0]["momentum"] == 0.8 and back.param_groups[0]["nesterov"] is False
    for k, i in enumerate([0, 1, 3, 4, 5]):
        assert torch.equal(back.state[bp[i]]["momentum_buffer"], opt.momentum.views[k])
    for p in bp:
        p.grad = torch.ones_like(p)
    back.step()
    guarded = GuardedSGD(cpu_params(3), lr=1.0)
    guarded.load_state_dict(sd)
    assert torch.equal(guarded.state[guarded._all_params()[5]]["momentum_buffer"], opt.momentum.views[4])
    # ... and back from each of the three: the momentum is copied INTO the arena, a missing or None buffer becomes zeros
    for source in (back, guarded, opt):
        fresh = DataParallelSGD(cpu_params(4), lr=1e-3, world=2, rank=0)
        for m in fresh.momentum.views:
            m.fill_(7.0)
        src = source.state_dict()
        fresh.load_state_dict(src)
        assert fresh.param_groups[0]["lr"] == 0.02 and fresh.param_groups[0]["weight_decay"] == 3e-4
        for i, p in enumerate(fresh.trainable):
            assert fresh.state[p]["momentum_buffer"] is fresh.momentum.views[i]
            want = src["state"].get(i, {}).get("momentum_buffer")
            assert torch.equal(fresh.momentum.views[i], torch.zeros_like(p) if want is None else want), (type(source).__name__, i)
    plain = torch.optim.SGD(cpu_params(5), lr=0.3, momentum=0.0)
    for p in plain.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    plain.step()                                         # momentum 0: torch's state holds momentum_buffer None
    fresh = DataParallelSGD(cpu_params(4), lr=1e-3)
    for m in fresh.momentum.views:
        m.fill_(7.0)
    fresh.load_state_dict(plain.state_dict())
    assert not bool(fresh.momentum.flat[:fresh.momentum.tail_offset].any()) and fresh.param_groups[0]["momentum"] == 0.0
    for key, value in (("dampening", 0.1), ("nesterov", True), ("maximize", True)):
        bad = plain.state_dict()
        bad["param_groups"][0][key] = value
        with pytest.raises(ValueError, match=key):
            fresh.load_state_dict(bad)


def test_dp_sgd_arguments_and_no_cpu_fallback():
    p = cpu_params()
    for kw in (dict(world=0), dict(world=2, rank=2), dict(rank=-1), dict(world=2.0), dict(n_tail=0)):
        with pytest.raises(ValueError, match="DataParallelSGD"):
            DataParallelSGD(p, lr=1e-3, **kw)
    with pytest.raises(ValueError, match="guard="):
        DataParallelSGD(p, lr=1e-3, guard="always")
    with pytest.raises(ValueError, match="lr="):
        DataParallelSGD(p, lr=float("nan"))
    opt = DataParallelSGD(p, lr=1e-3, world=3, rank=2)
    assert np.float32(opt.inv_world) == np.float32(1.0) / np.float32(3.0) == D.inv_world(3)
    with pytest.raises(StmError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(ValueError, match="no loss and no closure"):
        opt.step(torch.tensor(1.0))
    assert opt.counters() == (0, 0)


# ---- the private binding ------------------------------------------------------------------------------------------------------------------
def test_private_call_resolves_the_entry_and_checks_the_argument_count():
    with pytest.raises(StmError, match="takes 14 arguments, got 2"):
        _lib.private_call("stm_dp_sgd_finish_multi_f32", None, None)


@pytest.mark.parametrize("change,code,text", D.FINISH_REFUSALS, ids=D.REFUSAL_IDS)
def test_finish_refusals(change, code, text):
    with pytest.raises(StmError) as e:
        _lib.private_call("stm_dp_sgd_finish_multi_f32", *D.finish_args(**change))
    assert f"failed with code {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_finish_kernel_uses_no_scratch_and_no_lds():
    rows = [r for name, r in kernel_resources("optim.hip").items() if "dp_sgd_finish_multi_kernel" in name]
    assert len(rows) == 1
    assert rows[0].scratch == 0
    assert rows[0].lds == 0


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,mu,wd", [(1e-3, 0.9, 1e-4), (0.0137, 0.0, 0.0)])
def test_restatement_with_one_rank_is_the_single_rank_step(lr, mu, wd):
    p, g, m = (R.seeded_values(4099, 11 + i) * np.float32(s) for i, s in enumerate((1.0, 1e-3, 1e3)))
    p1, m1, g1 = D.finish_f32(p, g, m, 1, lr, mu, wd)
    p0, m0 = R.step_f32(p, g, m, lr, mu, wd)
    assert np.array_equal(D.bits(p1), D.bits(p0)) and np.array_equal(D.bits(m1), D.bits(m0)) and not g1.any()


def test_restatement_averages_before_the_weight_decay():
    p, g, m = (R.seeded_values(1031, 3 + i) for i in range(3))
    for world in (2, 3):
        p1, m1, _ = D.finish_f32(p, g, m, world, 1e-3, 0.9, 1e-4)
        p0, m0 = R.step_f32(p, g * D.inv_world(world), m, 1e-3, 0.9, 1e-4)
        assert np.array_equal(D.bits(p1), D.bits(p0)) and np.array_equal(D.bits(m1), D.bits(m0))
    assert D.inv_world(2) == np.float32(0.5) and D.inv_world(3).dtype == np.float32


# ---- TrainLoader(shard=...) -------------------------------------------------------------------------------------------------------------------
class CountingSet:
    def __init__(self, n):
        self.n, self.read = n, []

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        self.read.append(i)
        return i


class OkStatus:
    def raise_if_bad(self):
        pass


@pytest.fixture
def fake_collate(monkeypatch):
    monkeypatch.setattr(datasets, "collate_device", lambda records, device, max_gt, check: (list(records), OkStatus()))


def run(loader, epochs):
    out, states = [], []
    for _ in range(epochs):
        for (records,) in loader:
            out.append(records)
            states.append(loader.state())
    return out, states


@pytest.mark.parametrize("batch,shards", [(6, [(0, 1)]), (6, [(0, 2), (1, 2)]), (6, [(0, 3), (1, 3), (2, 3)]), (4, [(0, (3, 1)), (1, (3, 1))]),
                                         (5, [(0, (1, 3, 1)), (1, (1, 3, 1)), (2, (1, 3, 1))])], ids=["w1", "w2", "w3", "alloc31", "alloc131"])
def test_the_ranks_shares_concatenate_to_the_unsharded_batches(fake_collate, batch, shards):
    whole, whole_states = run(datasets.TrainLoader(CountingSet(29), batch, seed=5), 2)
    sets = [CountingSet(29) for _ in shards]
    loaders = [datasets.TrainLoader(ds, batch, seed=5, shard=s) for ds, s in zip(sets, shards)]
    assert all(len(ld) == 29 // batch for ld in loaders)
    got = [run(ld, 2) for ld in loaders]
    assert all(states == whole_states for _, states in got)                                 # state() is equal on all ranks
    for k, want in enumerate(whole):
        assert sum((batches[k] for batches, _ in got), []) == want
    sizes = [len(batches[0]) for batches, _ in got]
    second = shards[0][1]
    assert sizes == ([batch // second] * second if isinstance(second, int) else list(second))
    for ds, (batches, _) in zip(sets, got):
        assert ds.read == [i for b in batches for i in b]                                   # a rank reads its share and nothing else
    # a resume inside the second epoch, from the one sidecar, continues identically on every rank
    at = len(whole) // 2 + 2
    for s, (batches, _) in zip(shards, got):
        resumed = datasets.TrainLoader(CountingSet(29), batch, seed=0, shard=s)
        resumed.load_state(whole_states[at - 1])
        assert resumed.state() == whole_states[at - 1]
        assert run(resumed, 1)[0] == batches[at:]


def test_shard_none_is_the_loader_as_it_was_and_bad_shards_are_refused(fake_collate):
    a = datasets.TrainLoader(CountingSet(10), 3, seed=1)
    assert a.shard is None and a.share == (0, 3)
    order0 = a.order(0)
    assert [records for (records,) in a] == [order0[0:3], order0[3:6], order0[6:9]]
    for shard, text in (((0, 2), "does not split evenly"), ((0, 0), "does not split evenly"), ((0, (2, 2)), "sum to batch_size"),
                        ((0, (3, 0)), "positive"), ((2, (2, 1)), "rank=2"), ((-1, 3), "rank=-1"), ((3, 3), "rank=3")):
        with pytest.raises(ValueError, match=text):
            datasets.TrainLoader(CountingSet(10), 3, shard=shard)


# ---- two gloo processes on CPU tensors -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gloo"))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_gloo_worker.py"), out], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert [p.returncode for p in procs] == [0, 0], "\n".join(log[-2000:] for log in logs)
    return [torch.load(os.path.join(out, f"rank{r}.pt")) for r in range(2)]


def test_exchange_leaves_both_ranks_with_the_bit_identical_sum(two_ranks):
    a, b = two_ranks
    assert not torch.equal(a["local"], b["local"])
    want = a["local"] + b["local"]                         # the sum of two fp32 values does not depend on the order
    for got in (a["summed"], b["summed"]):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(want[-8:].ne(0).all())                     # the tail rode along


def test_a_nan_in_one_ranks_loss_is_not_finite_on_both(two_ranks):
    a, b = two_ranks
    tail0 = a["poisoned"].numel() - 8
    for got in (a["poisoned"], b["poisoned"]):
        assert not bool(torch.isfinite(got[tail0]))
        assert bool(torch.isfinite(got[:tail0]).all()) and bool(torch.isfinite(got[tail0 + 1:]).all())
    assert torch.equal(a["poisoned"][:tail0], b["poisoned"][:tail0])


def test_checksum_comparison_and_broadcast_between_the_ranks(two_ranks):
    for r, got in enumerate(two_ranks):
        assert got["first_difference_same"] is None and got["first_difference_rank"] == 1
        assert got["broadcast"][0].tolist() == [1.0] * 4 and got["broadcast"][1].tolist() == [7]


# ---- scripts/train_ytvis.py ------------------------------------------------------------------------------------------------------------------
def test_train_script_arguments_and_the_single_gpu_objects(capsys):
    from scripts import train_ytvis
    a = train_ytvis.parse_args(["ann.json", "frames"])
    assert (a.gpus, a.backend, a.batch_alloc, a.share_gpu) == (1, "nccl", None, False)
    params = cpu_params()
    opt = train_ytvis.make_optimizer(a, params, 1e-3)
    assert type(opt) is GuardedSGD and all(p.grad is None for p in params)                  # --gpus 1: today's objects
    loader = train_ytvis.make_loader(a, CountingSet(9), "cpu")
    assert loader.shard is None and loader.batch_size == 4 and loader.share == (0, 4)
    a = train_ytvis.parse_args(["ann.json", "frames", "--gpus", "2", "--backend", "gloo", "--share-gpu", "--batch_alloc", "3,1"])
    assert (a.gpus, a.backend, a.batch_alloc, a.share_gpu) == (2, "gloo", (3, 1), True)
    opt = train_ytvis.make_optimizer(a, cpu_params(), 1e-3, rank=1)
    assert type(opt) is DataParallelSGD and (opt.world, opt.rank, opt.guard) == (2, 1, "loss")
    assert train_ytvis.make_loader(a, CountingSet(9), "cpu", rank=1).share == (3, 4)
    a = train_ytvis.parse_args(["ann.json", "frames", "--gpus", "4", "--batch_size", "8", "--guard", "off"])
    assert train_ytvis.make_loader(a, CountingSet(9), "cpu", rank=3).share == (6, 8)
    assert train_ytvis.make_optimizer(a, cpu_params(), 1e-3, rank=3).guard is None
    for bad in (["--gpus", "3"], ["--gpus", "0"], ["--gpus", "2", "--batch_alloc", "3,2"], ["--gpus", "2", "--batch_alloc", "4"],
                ["--gpus", "2", "--batch_alloc", "4,0"], ["--gpus", "2", "--batch_alloc", "a,b"], ["--gpus", "2", "--share-gpu"],
                ["--backend", "mpi"]):
        with pytest.raises(SystemExit):
            train_ytvis.parse_args(["ann.json", "frames"] + bad)
    capsys.readouterr()
