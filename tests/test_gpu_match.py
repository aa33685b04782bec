"""The device target assignment (csrc/match.hip: layers.match, layers.match_batch, ops.match_priors, layers.encode) against the reference's
fp32 goldens of tests/golden/match_cases.npz.

The integer targets and the matched boxes are exact, and loc_t's columns 0-1 are bit-exact.  Columns 2-3 hold a log: they are judged by
their largest error against an fp64 encode of the same matched boxes, which may be at most twice the largest error of the reference's own
fp32 values against the same fp64 values on that case (the kernel evaluates the log in double and rounds once, so it needs no more)."""
import pytest
import torch

import match_cases as MC
from stmask_amd import layers, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_results = {}


def _dev_case(name):
    c = MC.case(name)
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _run(name):
    """Every entry point once per case (and the per-image form twice), shared by the tests below."""
    if name in _results:
        return _results[name]
    d = _dev_case(name)
    pos, neg = MC.thresholds()
    P = d["priors"].shape[0]
    out = {}
    for tag in ("match", "match_again"):
        loc_t = torch.full((3, P, 4), -7.0, device=DEV)
        conf_t, idx_t, ids_t = (torch.full((3, P), -7, dtype=torch.int64, device=DEV) for _ in range(3))
        layers.match(pos, neg, d["bbox"], d["labels"], d["ids"], d["priors"], None, d["conf"], loc_t, conf_t, idx_t, ids_t, 1)
        out[tag] = (loc_t, conf_t, idx_t, ids_t)
    out["batch"] = layers.match_batch(pos, neg, [d["bbox"]], [d["labels"]], [d["ids"]], d["priors"], d["conf"][None])
    out["raw"] = ops.match_priors(d["bbox"], d["labels"], d["ids"], [d["bbox"].shape[0]], d["priors"][None].contiguous(), d["conf"][None], pos, neg,
                                  want_status=True)
    torch.cuda.synchronize()
    _results[name] = out
    return out


def _check_against_golden(name, loc_t, conf_t, idx_t, ids_t, gt_boxes_t=None):
    c = MC.case(name)
    loc_t, conf_t, idx_t, ids_t = loc_t.cpu(), conf_t.cpu(), idx_t.cpu(), ids_t.cpu()
    assert torch.equal(idx_t, c["idx_t"]), name
    assert torch.equal(conf_t, c["conf_t"]), name
    assert torch.equal(ids_t, c["ids_t"]), name
    matched = c["bbox"][c["idx_t"]]
    if gt_boxes_t is not None:
        assert torch.equal(gt_boxes_t.cpu(), matched), name
    assert torch.equal(loc_t[:, :2], c["loc_t"][:, :2]), name
    f64 = MC.encode_f64(matched, c["priors"])[:, 2:]
    err_dev = float((loc_t[:, 2:].double() - f64).abs().max())
    err_ref = float((c["loc_t"][:, 2:].double() - f64).abs().max())
    print(f"{name}: log columns, largest error against fp64: device {err_dev:.3e}, reference fp32 {err_ref:.3e}")
    assert err_dev <= 2 * err_ref, (name, err_dev, err_ref)


@pytest.mark.parametrize("name", MC.names())
def test_match_fills_its_row_with_the_reference_targets(name):
    loc_t, conf_t, idx_t, ids_t = _run(name)["match"]
    _check_against_golden(name, loc_t[1], conf_t[1], idx_t[1], ids_t[1])
    for r in (0, 2):                                   # the other rows are untouched
        assert bool((loc_t[r] == -7.0).all()) and all(bool((t[r] == -7).all()) for t in (conf_t, idx_t, ids_t))


@pytest.mark.parametrize("name", MC.names())
def test_match_batch_and_raw_entry_give_the_reference_targets(name):
    r = _run(name)
    loc_t, conf_t, idx_t, ids_t, gt = r["batch"]
    assert loc_t.shape[0] == 1 and conf_t.dtype == idx_t.dtype == ids_t.dtype == torch.int64
    _check_against_golden(name, loc_t[0], conf_t[0], idx_t[0], ids_t[0], gt[0])
    loc_r, gt_r, conf_r, idx_r, ids_r, status = r["raw"]          # priors given per image ([B, P, 4])
    _check_against_golden(name, loc_r[0], conf_r[0], idx_r[0], ids_r[0], gt_r[0])
    assert status.tolist() == [0]


@pytest.mark.parametrize("name", MC.names())
def test_runs_are_bit_identical(name):
    r = _run(name)
    for a, b in zip(r["match"], r["match_again"]):
        assert torch.equal(a, b)
    m, bt = r["match"], r["batch"]
    assert torch.equal(m[0][1].view(torch.int32), bt[0][0].view(torch.int32))
    for k in (1, 2, 3):
        assert torch.equal(m[k][1], bt[k][0])
    assert torch.equal(bt[0].view(torch.int32), r["raw"][0].view(torch.int32))


def test_ragged_batch_equals_per_image_calls():
    names = MC.ragged_names()
    ds = [_dev_case(n) for n in names]
    assert [d["bbox"].shape[0] for d in ds] == [1, 7, 20]
    pos, neg = MC.thresholds()
    conf = torch.stack([d["conf"] for d in ds])
    loc_t, conf_t, idx_t, ids_t, gt = layers.match_batch(pos, neg, [d["bbox"] for d in ds], [d["labels"] for d in ds], [d["ids"] for d in ds],
                                                         ds[0]["priors"], conf)
    assert loc_t.shape == (3, 15345, 4) and gt.shape == (3, 15345, 4) and conf_t.shape == idx_t.shape == ids_t.shape == (3, 15345)
    for b, n in enumerate(names):
        _check_against_golden(n, loc_t[b], conf_t[b], idx_t[b], ids_t[b], gt[b])
        one = _run(n)["match"]
        assert torch.equal(loc_t[b].view(torch.int32), one[0][1].view(torch.int32))
        assert torch.equal(conf_t[b], one[1][1]) and torch.equal(idx_t[b], one[2][1]) and torch.equal(ids_t[b], one[3][1])


def test_conf_that_requires_grad_is_read_detached():
    d = _dev_case("p300_g5")
    pos, neg = MC.thresholds()
    conf = d["conf"][None].clone().requires_grad_()
    with torch.enable_grad():
        outs = layers.match_batch(pos, neg, [d["bbox"]], [d["labels"]], [d["ids"]], d["priors"], conf * 1.0)
        P = d["priors"].shape[0]
        loc_t = torch.zeros(1, P, 4, device=DEV)
        conf_t, idx_t, ids_t = (torch.zeros(1, P, dtype=torch.int64, device=DEV) for _ in range(3))
        layers.match(pos, neg, d["bbox"], d["labels"], d["ids"], d["priors"], None, (conf * 1.0)[0], loc_t, conf_t, idx_t, ids_t, 0)
    for t in outs + (loc_t, conf_t, idx_t, ids_t):
        assert t.grad_fn is None and not t.requires_grad
    _check_against_golden("p300_g5", outs[0][0], outs[1][0], outs[2][0], outs[3][0], outs[4][0])
    _check_against_golden("p300_g5", loc_t[0], conf_t[0], idx_t[0], ids_t[0])


def test_targets_of_other_layouts_are_filled_through_a_copy():
    """Target tensors that are not contiguous fp32 / int64 rows (here a strided view) are filled all the same."""
    d = _dev_case("p37_g5")
    pos, neg = MC.thresholds()
    P = d["priors"].shape[0]
    loc_t = torch.zeros(2, P, 8, device=DEV)[:, :, ::2]
    conf_t, idx_t, ids_t = (torch.zeros(2, 2 * P, dtype=torch.int64, device=DEV)[:, ::2] for _ in range(3))
    layers.match(pos, neg, d["bbox"], d["labels"], d["ids"], d["priors"], None, d["conf"], loc_t, conf_t, idx_t, ids_t, 1)
    _check_against_golden("p37_g5", loc_t[1], conf_t[1], idx_t[1], ids_t[1])


def test_out_of_contract_boxes_are_flagged_not_run_into():
    """A box with x2 <= x1 is outside the contract: the status word says so (bit 1), and a valid call says 0."""
    d = _dev_case("p37_g5")
    pos, neg = MC.thresholds()
    bad = d["bbox"].clone()
    bad[2, 2] = bad[2, 0]
    status = ops.match_priors(bad, d["labels"], d["ids"], [5], d["priors"], d["conf"][None], pos, neg, want_status=True)[5]
    assert status.tolist() == [2]


def test_encode_matches_the_reference():
    m, p, ref = MC.encode_case()
    out = layers.encode(m.to(DEV), p.to(DEV)).cpu()
    assert torch.equal(out[:, :2], ref[:, :2])
    f64 = MC.encode_f64(m, p)
    err_dev, err_ref = float((out[:, 2:].double() - f64[:, 2:]).abs().max()), float((ref[:, 2:].double() - f64[:, 2:]).abs().max())
    print(f"encode: log columns, largest error against fp64: device {err_dev:.3e}, reference fp32 {err_ref:.3e}")
    assert err_dev <= 2 * err_ref
    assert layers.encode(m[:0].to(DEV), p[:0].to(DEV)).shape == (0, 4)


def test_encode_with_a_gradient_follows_autograd_of_the_fp64_expression():
    m, p, ref = MC.encode_case()
    go = torch.randn(m.shape, generator=torch.Generator().manual_seed(5))
    m64, p64 = m.double().requires_grad_(), p.double().requires_grad_()
    f64 = MC.encode_f64(m64, p64)
    f64.backward(go.double())
    md, pd = m.to(DEV).requires_grad_(), p.to(DEV).requires_grad_()
    out = layers.encode(md, pd)
    assert out.grad_fn is not None
    out.backward(go.to(DEV))
    o = out.detach().cpu()
    assert torch.equal(o[:, :2], ref[:, :2])
    err_dev = float((o[:, 2:].double() - f64.detach()[:, 2:]).abs().max())
    err_ref = float((ref[:, 2:].double() - f64.detach()[:, 2:]).abs().max())
    print(f"encode (autograd path): log columns, largest error against fp64: device {err_dev:.3e}, reference fp32 {err_ref:.3e}")
    assert err_dev <= 2 * err_ref
    for g32, g64 in ((md.grad, m64.grad), (pd.grad, p64.grad)):
        assert bool(((g32.cpu().double() - g64).abs() <= 1e-5 * g64.abs().clamp(min=1)).all())
