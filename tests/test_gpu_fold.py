"""csrc/fold.hip on the MI355X against the numpy restatement of fuse._fold (tests/fold_restate.py, itself held to torch's CPU fold by
tests/test_validate_cpu.py), bit for bit.  The shapes are the smallest that reach every path of the kernel: numel and inner that are no multiple
of 4 (the 4-byte tail; channels that change inside a 16-byte access), tensors of 18432 and 4105 elements (several workgroups, a last chunk that
is not full, a chunk boundary inside a channel), a dst that starts one element into its buffer (the 4-byte path for the whole tensor), a bias
row without a source, 65 and 130 rows (two and three calls), rows of two eps values in one call (a launch each), and a running_var of 0, a
negative gamma, a variance of +inf and one of NaN among the channels.  Every dst lies between guard elements that must stay as they were."""
import numpy as np
import pytest
import torch

import fold_restate as R
from stmask_amd import _lib, validate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (3, 5, 3), (64, 32, 1), (7, 3, 3), (64, 32, 3), (5, 821, 1)]      # (O, C, k)
GUARD, SENTINEL = 8, np.float32(-12345.5)


class BN:
    """The four tensors and eps of a BatchNorm on the device, as validate.fold_row reads them."""

    def __init__(self, channels, seed, eps):
        self.host = R.seeded_bn(channels, seed, nonfinite=True)
        self.weight, self.bias, self.running_mean, self.running_var = (torch.from_numpy(a).to(DEV) for a in self.host)
        self.eps = eps


class Case:
    """One destination between guards, its row and the bits the restatement expects."""

    def __init__(self, kind, shape, seed, eps, offset, with_src=True):
        O, C, k = shape
        g = np.random.default_rng(seed)
        self.bn = BN(O, seed + 1, eps) if kind != validate.COPY else None
        dims = (O,) if kind == validate.BIAS else (O, C, k, k)
        src = g.normal(0, 0.3, dims).astype(np.float32) if with_src else None
        if kind == validate.COPY:
            src.reshape(-1)[::7] = np.nan                                   # a copy moves bits, whatever they say
            self.want = src
        elif kind == validate.WEIGHT:
            gamma, _, _, var = self.bn.host
            self.want = R.fold_weight(src, gamma, var, eps)
        else:
            self.want = R.fold_bias(src, *self.bn.host, eps)
        n = int(np.prod(dims))
        self.buf = torch.full((n + 2 * GUARD + 1,), float(SENTINEL), device=DEV)
        self.dst = self.buf[GUARD + offset:GUARD + offset + n].view(dims)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.src = torch.from_numpy(src).to(DEV) if with_src else None
        self.row = validate.fold_row(kind, self.dst, self.src, self.bn)

    def check(self, what):
        got = self.buf.cpu().numpy()
        assert np.array_equal(R.bits(got[self.lo:self.hi]), R.bits(self.want).reshape(-1)), what
        assert (got[:self.lo] == SENTINEL).all() and (got[self.hi:] == SENTINEL).all(), what


def cases_of(shape, seed, eps, offset):
    return [Case(validate.WEIGHT, shape, seed, eps, offset), Case(validate.BIAS, shape, seed + 10, eps, offset),
            Case(validate.BIAS, shape, seed + 20, eps, offset, with_src=False), Case(validate.COPY, shape, seed + 30, eps, offset)]


def run(cases):
    with torch.cuda.device(DEV):
        calls = validate.fold_rows([c.row for c in cases])
    torch.cuda.synchronize()
    return calls


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_kernel_equals_the_restatement_bit_for_bit(eps, offset):
    cases = [c for i, shape in enumerate(SHAPES) for c in cases_of(shape, 100 * i, eps, offset)]
    assert len(cases) <= _lib.FOLD_MAX_ROWS and run(cases) == 1
    aligned = [c.dst.data_ptr() % 16 == 0 for c in cases]
    assert all(aligned) if offset == 0 else not any(aligned)                  # the 16-byte path, or the 4-byte path for every tensor
    for i, c in enumerate(cases):
        c.check((SHAPES[i // 4], i % 4, eps, offset))
    nan_rows = [c for c in cases if c.bn is not None and c.want.shape[0] >= 3]
    assert nan_rows and all(np.isnan(c.want[2]).all() and not np.isnan(c.want[0]).any() for c in nan_rows)      # the non-finite variance travelled


@pytest.mark.parametrize("n_rows,calls", [(65, 2), (130, 3)])
def test_more_rows_than_a_table_holds_take_more_calls(n_rows, calls):
    small = SHAPES[:4]
    cases = []
    while len(cases) < n_rows:
        i = len(cases) // 4
        cases += cases_of(small[i % 4], 1000 + i, 1e-5, (i // 4) % 2)
    cases = cases[:n_rows]
    assert run(cases) == calls
    for i, c in enumerate(cases):
        c.check(i)


def test_rows_of_two_eps_values_in_one_call():
    cases = [c for i, eps in enumerate([1e-5, 1e-3, 1e-3, 1e-5]) for c in cases_of(SHAPES[1 + i % 3], 2000 + i, eps, 0)]
    assert run(cases) == 1
    for i, c in enumerate(cases):
        c.check(i)


def test_rows_without_elements_are_passed_over():
    empty = _lib.FoldRow()
    empty.kind = _lib.FOLD_COPY
    cases = cases_of(SHAPES[1], 3000, 1e-5, 0)
    with torch.cuda.device(DEV):
        validate.fold_rows([empty, cases[0].row, empty, cases[1].row, empty])
        validate.fold_rows([empty])
    torch.cuda.synchronize()
    cases[0].check("weight")
    cases[1].check("bias")
