#!/usr/bin/env python
"""Video mask AP of a YouTube-VIS results file: a thin command line over stmask_amd.eval_utils.calc_metrics (the reference's
layers/eval_utils.py calc_metrics; the mask work runs on the MI355X, see stmask_amd/vis_eval.py and INTEGRATION.md section 18).

    python scripts/score_results.py ANN.json RESULTS.json [--out FILE]

Prints the 12 summary lines in cocoapi's layout and, last, the 12 numbers as one JSON line; --out also writes the summary lines to FILE."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("annotations", help="YouTube-VIS annotation json (videos, categories, annotations)")
    ap.add_argument("results", help="results json as results2json_videoseg writes it")
    ap.add_argument("--out", default=None, help="also write the 12 summary lines to this file")
    args = ap.parse_args(argv)
    from stmask_amd.eval_utils import calc_metrics
    stats = calc_metrics(args.annotations, args.results, args.out)
    names = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
    print(json.dumps({n: float(v) for n, v in zip(names, stats)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
