"""The training loop's host side without a GPU: train.LossLog on CPU tensors, stmask_amd.checkpoint (names, latest / interrupt, atomic writes,
bare-.pth resume), TrainLoader.state / load_state, and the learning rate at a resumed iteration."""
import math
import os

import pytest
import torch

from stmask_amd import checkpoint, datasets
from stmask_amd.optim import GuardedSGD
from stmask_amd.train import LossLog, lr_at


# ---- LossLog ------------------------------------------------------------------------------------------------------------------------------
def terms(a, b):
    return {"B": torch.tensor(float(a)), "M": torch.tensor(float(b))}


def test_loss_log_wraps_its_ring_and_keeps_the_window():
    log = LossLog(["B", "M"], capacity=4, window=3)
    assert log.names == ["B", "M", "Total"]
    assert all(math.isnan(v) and math.isnan(avg) for v, avg in log.read().values())          # nothing appended yet
    seen = []
    for i in range(11):                                                                       # wraps the 4 rows of the ring more than twice
        log.append(terms(i, 2 * i))
        seen.append(float(i))
        if i % 3 == 2 or i == 10:
            got = log.read()
            assert [r[0] for r in log.rows] == seen[-len(log.rows):] and len(log.rows) == (2 if i == 10 else 3)
            want = sum(seen[-3:]) / 3
            assert got["B"] == (float(i), want) and got["M"] == (2.0 * i, 2 * want) and got["Total"] == (3.0 * i, 3 * want)
    assert log.ring.shape == (4, 3) and log.read()["B"] == (10.0, 9.0) and log.rows == []     # a read with nothing new repeats the figures


def test_loss_log_mean_ignores_values_that_are_not_finite():
    log = LossLog(["B", "M"], capacity=8, window=100)
    for a, b in ((1.0, 1.0), (float("nan"), 2.0), (3.0, float("inf")), (5.0, 4.0), (float("-inf"), 7.0)):
        log.append(terms(a, b))
    got = log.read()
    assert math.isinf(got["B"][0]) and got["B"][1] == (1.0 + 3.0 + 5.0) / 3
    assert got["M"] == (7.0, (1.0 + 2.0 + 4.0 + 7.0) / 4)
    assert math.isinf(got["Total"][0]) and got["Total"][1] == (2.0 + 9.0) / 2                 # the sum is finite only where both terms are


def test_loss_log_overflow_raises_at_read():
    log = LossLog(["B", "M"], capacity=4)
    for i in range(4):
        log.append(terms(i, i))
    log.read()
    for i in range(5):
        log.append(terms(i, i))
    with pytest.raises(RuntimeError, match="5 rows appended since the last read, the ring holds 4"):
        log.read()
    with pytest.raises(ValueError):
        LossLog([], capacity=4)


# ---- checkpoint: names --------------------------------------------------------------------------------------------------------------------------
def test_names_and_parsing():
    assert checkpoint.save_path("STMask_plus_base", 3, 12000, "w") == os.path.join("w", "STMask_plus_base_3_12000.pth")
    assert checkpoint.save_path("a", 0, 7, "", interrupt=True) == "a_0_7_interrupt.pth"
    assert checkpoint.parse_path("w/STMask_plus_base_3_12000.pth") == ("STMask_plus_base", 3, 12000)
    assert checkpoint.parse_path("/x/y/STMask_plus_base_12_345_interrupt.pth") == ("STMask_plus_base", 12, 345)
    assert checkpoint.parse_path("a_b_1_2") == ("a_b", 1, 2)
    for bad in ("weights.pth", "resnet50-19c8e357.pth", "a_1_x.pth", "_1_2.pth"):
        with pytest.raises(ValueError):
            checkpoint.parse_path(bad)


def touch(folder, name):
    path = os.path.join(str(folder), name)
    open(path, "wb").close()
    return path


def test_get_latest_interrupt_and_removal(tmp_path):
    assert checkpoint.get_latest(str(tmp_path), "net") is None and checkpoint.get_interrupt(str(tmp_path)) is None
    touch(tmp_path, "net_0_100.pth")
    touch(tmp_path, "net_2_9000.pth")
    touch(tmp_path, "net_1_10000.pth")
    touch(tmp_path, "net_1_10000.pth.state")
    touch(tmp_path, "net_plus_5_99999.pth")            # another model whose name begins alike
    touch(tmp_path, "net_backbone.pth")                # not a checkpoint name
    assert checkpoint.get_latest(str(tmp_path), "net") == os.path.join(str(tmp_path), "net_1_10000.pth")
    assert checkpoint.get_latest(str(tmp_path), "net_plus") == os.path.join(str(tmp_path), "net_plus_5_99999.pth")
    intr = touch(tmp_path, "net_2_10500_interrupt.pth")
    touch(tmp_path, "net_2_10500_interrupt.pth.state")
    assert checkpoint.get_interrupt(str(tmp_path)) == intr
    assert checkpoint.get_latest(str(tmp_path), "net") == intr                                # the reference counts the interrupt file too
    checkpoint.remove_interrupt(str(tmp_path))
    assert checkpoint.get_interrupt(str(tmp_path)) is None and not os.path.exists(intr + ".state")
    # keep_latest: the loop removes the previous latest, sidecar included
    latest = checkpoint.get_latest(str(tmp_path), "net")
    checkpoint.remove(latest)
    assert not os.path.exists(latest) and not os.path.exists(latest + ".state")
    assert checkpoint.get_latest(str(tmp_path), "net") == os.path.join(str(tmp_path), "net_2_9000.pth")


# ---- checkpoint: files ----------------------------------------------------------------------------------------------------------------------------
class TinyNet(torch.nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(3, 4)
        self.b = torch.nn.Linear(4, 2)

    def save_weights(self, path):
        torch.save(self.state_dict(), path)

    def load_weights(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))


class FakeLoader:
    def __init__(self):
        self.got = None

    def state(self):
        return {"seed": 3, "epoch": 4, "batch": 5}

    def load_state(self, state):
        self.got = state


def test_save_and_load_round_trip_with_sidecar(tmp_path):
    net = TinyNet(0)
    opt = GuardedSGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    for p in net.parameters():
        opt.state[p]["momentum_buffer"] = torch.randn_like(p)
    path = checkpoint.save_path("tiny", 4, 77, str(tmp_path))
    checkpoint.save(path, net, opt, 77, 4, FakeLoader())
    assert sorted(os.listdir(str(tmp_path))) == ["tiny_4_77.pth", "tiny_4_77.pth.state"]      # no temporary file stays
    plain = torch.load(path, map_location="cpu")                                              # the weights file is a plain state dict
    assert sorted(plain) == sorted(net.state_dict()) and all(torch.equal(plain[k], v) for k, v in net.state_dict().items())
    net2, loader2 = TinyNet(1), FakeLoader()
    opt2 = GuardedSGD(net2.parameters(), lr=0.5, momentum=0.1)
    got = checkpoint.load(path, net2, opt2, loader2)
    assert got == {"iteration": 77, "epoch": 4, "sidecar": True} and loader2.got == {"seed": 3, "epoch": 4, "batch": 5}
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
    assert opt2.param_groups[0]["lr"] == 0.01 and opt2.param_groups[0]["momentum"] == 0.9
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]["momentum_buffer"], opt2.state[q]["momentum_buffer"])
    # the sidecar's optimizer part is torch SGD's layout
    ref = torch.optim.SGD(TinyNet(2).parameters(), lr=1.0)
    ref.load_state_dict(torch.load(path + ".state", map_location="cpu")["optimizer"])
    assert ref.param_groups[0]["lr"] == 0.01


def test_bare_pth_takes_the_iteration_from_its_name(tmp_path):
    net = TinyNet(0)
    path = checkpoint.save_path("tiny", 2, 4321, str(tmp_path), interrupt=True)
    net.save_weights(path)
    net2 = TinyNet(1)
    opt2 = GuardedSGD(net2.parameters(), lr=0.5)
    loader2 = FakeLoader()
    assert checkpoint.load(path, net2, opt2, loader2) == {"iteration": 4321, "epoch": 2, "sidecar": False}
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
    assert loader2.got is None and opt2.param_groups[0]["lr"] == 0.5 and len(opt2.state) == 0  # momentum restarts at zero, as in the reference


def test_an_interrupted_save_leaves_the_previous_file(tmp_path):
    net = TinyNet(0)
    path = checkpoint.save_path("tiny", 0, 10, str(tmp_path))
    checkpoint.save(path, net, None, 10, 0)
    before = open(path, "rb").read()
    before_state = open(path + ".state", "rb").read()

    class Dies(TinyNet):
        def save_weights(self, path):
            with open(path, "wb") as f:
                f.write(b"half a file")
            raise KeyboardInterrupt

    with pytest.raises(KeyboardInterrupt):
        checkpoint.save(path, Dies(1), None, 11, 0)
    assert open(path, "rb").read() == before and open(path + ".state", "rb").read() == before_state
    assert sorted(os.listdir(str(tmp_path))) == ["tiny_0_10.pth", "tiny_0_10.pth.state"]
    written = []
    real = os.replace
    try:                                                                    # the file appears under its name by a rename in its own folder
        os.replace = lambda a, b: (written.append((a, b)), real(a, b))[1]
        checkpoint.save(path, TinyNet(2), None, 12, 0)
    finally:
        os.replace = real
    assert [b for _, b in written] == [path, path + ".state"]
    assert all(os.path.dirname(a) == os.path.dirname(b) and a != b for a, b in written)
    assert open(path, "rb").read() != before


# ---- TrainLoader: resume ------------------------------------------------------------------------------------------------------------------------
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


def test_loader_resumes_inside_an_epoch_without_reading_what_it_skips(fake_collate):
    full = datasets.TrainLoader(CountingSet(23), 4, seed=5)
    assert full.state() == {"seed": 5, "epoch": 0, "batch": 0}
    epochs, states = [], []
    for _ in range(3):
        epoch = []
        for (records,) in full:
            epoch.append(records)
            states.append(full.state())
        epochs.append(epoch)
    assert len(epochs[0]) == 5 and epochs[0] != epochs[1]
    # the state after batch k of epoch e says (e, k + 1); after the last batch of an epoch, the next epoch from its start
    assert states[5 + 1] == {"seed": 5, "epoch": 1, "batch": 2} and states[4] == {"seed": 5, "epoch": 1, "batch": 0}
    ds = CountingSet(23)
    resumed = datasets.TrainLoader(ds, 4, seed=0)
    resumed.load_state(states[5 + 1])
    assert resumed.state() == states[5 + 1]                                  # before the first batch is drawn, too
    got = [records for (records,) in resumed]
    assert got == epochs[1][2:]
    assert sorted(ds.read) == sorted(i for batch in epochs[1][2:] for i in batch)          # no record of batches 0 and 1 was read
    assert [records for (records,) in resumed] == epochs[2]                  # and the next epoch is the uninterrupted run's
    # resuming at an epoch's end starts the next one
    resumed.load_state(states[4])
    assert [records for (records,) in resumed] == epochs[1]
    with pytest.raises(ValueError):
        resumed.load_state({"seed": 5, "epoch": 0, "batch": 6})


def test_loader_without_load_state_is_unchanged(fake_collate):
    a = datasets.TrainLoader(CountingSet(10), 3, seed=1)
    order0, order1 = a.order(0), a.order(1)
    assert [records for (records,) in a] == [order0[0:3], order0[3:6], order0[6:9]]
    assert [records for (records,) in a] == [order1[0:3], order1[3:6], order1[6:9]] and a.epoch == 2


def test_lr_at_the_resumed_iteration_is_the_uninterrupted_runs():
    kw = dict(lr=1e-3, gamma=0.1, lr_steps=[150, 200], lr_warmup_until=50, lr_warmup_init=1e-4)
    run = [lr_at(i, **kw) for i in range(260)]
    for resumed_at in (0, 17, 50, 51, 149, 150, 199, 200, 259):             # lr_at is a pure function of the iteration: no loop state to restore
        assert [lr_at(i, **kw) for i in range(resumed_at, 260)] == run[resumed_at:]
    assert run[17] == (1e-3 - 1e-4) * (17 / 50) + 1e-4 and run[150] == 1e-3 * 0.1 and run[200] == 1e-3 * 0.1 ** 2
