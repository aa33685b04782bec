"""The cases of tests/golden/match_cases.npz (written by tests/golden/gen_match_golden.py from the reference's fp32 match and encode) as
tensors, shared by tests/test_match_cpu.py and tests/test_gpu_match.py.  Loaded once per process; nothing here is modified by a test."""
import functools

import torch

from conftest import load_golden

LEVELS = ("p_48x80", "p_24x40", "p_12x20", "p_6x10", "p_3x5")


@functools.lru_cache(maxsize=None)
def _files():
    return load_golden("match_cases.npz"), load_golden("priors.npz")


def names():
    return [str(n) for n in _files()[0]["case_names"]]


def ragged_names():
    return [str(n) for n in _files()[0]["ragged"]]


def thresholds():
    z = _files()[0]
    return float(z["pos"]), float(z["neg"])


def _priors(which):
    pz = _files()[1]
    if which in LEVELS:
        return pz[which]
    allp = torch.cat([pz[k] for k in LEVELS])
    return allp if which == "all" else allp[:int(which[len("prefix"):])]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: priors [P,4], bbox [G,4], labels, ids [G] int64, conf [P,C] fp32 (rebuilt from its seed where the file holds only the rows the
    reference read: those rows must come out exactly as stored), and the reference's fp32 loc_t [P,4], conf_t, idx_t, ids_t [P] int64."""
    z = _files()[0]
    which = str(z["case_priors"][names().index(name)])
    g = {k[len(name) + 2:]: v for k, v in z.items() if k.startswith(name + "__")}
    priors = _priors(which).contiguous()
    P, C = priors.shape[0], int(z["n_classes"])
    if "conf" in g:
        conf = g["conf"]
    else:
        conf = 2 * torch.randn(P, C, generator=torch.Generator().manual_seed(int(g["conf_seed"])))
        assert torch.equal(conf[g["conf_rows_idx"].long()], g["conf_rows"]), f"{name}: the seeded conf differs from the rows the reference read"
    assert conf.shape == (P, C)
    return dict(name=name, priors=priors, bbox=g["bbox"], labels=g["labels"], ids=g["ids"], conf=conf, loc_t=g["loc_t_T"].t().contiguous(),
                conf_t=g["conf_t"].long(), idx_t=g["idx_t"].long(), ids_t=g["ids_t"].long(), n_keep=int(g["n_keep"]), n_multi=int(g["n_multi"]),
                margin=float(g["margin"]))


def encode_case():
    z = _files()[0]
    return z["enc_matched"], z["enc_priors"], z["enc_out"]


def encode_f64(matched, priors):
    """encode (box_utils.py:223-233) in fp64 on the fp32 inputs: the yardstick of the log columns."""
    m, p = matched.double(), priors.double()
    return torch.cat([((m[:, :2] + m[:, 2:]) / 2 - p[:, :2]) / (0.1 * p[:, 2:]), torch.log((m[:, 2:] - m[:, :2]) / p[:, 2:]) / 0.2], 1)
