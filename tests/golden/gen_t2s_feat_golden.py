#!/usr/bin/env python3
"""Golden vectors of T2S_concat_feat, made by importing the reference's own Python (build container only).

    python tests/golden/gen_t2s_feat_golden.py           # writes tests/golden/t2s_feat_cases.npz

The reference's correlate (layers/modules/track_to_segment_head.py:40-62, its sampler served by the CPU oracle as in gen_golden.py) and the
F.relu(torch.cat(...)) of STMask.py:291-296 on the seeded inputs of tests/t2s_feat_restate.py, for the cases marked ref there.  Forward values only:
the oracle's sampler carries no gradient on the CPU."""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import install_stubs, save  # noqa: E402

import t2s_feat_restate as R  # noqa: E402


def main():
    install_stubs()
    from datasets.config import set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.modules.track_to_segment_head import correlate
    out = {}
    for name, spec in R.CASES.items():
        if not spec["ref"]:
            continue
        c = R.draw_case(name)
        fpn, t2s = c["fpn"], c["t2s"]
        with torch.no_grad():
            fpn_ref, fpn_next = fpn[::2].contiguous(), fpn[1::2].contiguous()
            x_ref, x_next = t2s[::2].contiguous(), t2s[1::2].contiguous()
            x_corr = correlate(fpn_ref, fpn_next, patch_size=c["P"])
            out[name] = F.relu(torch.cat([x_corr, x_ref, x_next], dim=1))
        out[name + "_fpn_sum"] = fpn.double().sum()          # the inputs are drawn again by the tests: their checksums guard the generator
        out[name + "_t2s_sum"] = t2s.double().sum()
    save("t2s_feat_cases.npz", **out)


if __name__ == "__main__":
    main()
