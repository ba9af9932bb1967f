#!/usr/bin/env python3
"""Observed errors of `xmca_amd.prepare.time_filter` against the longdouble truth of tests/time_filter_cases.py over every run and
dtype of tests/test_gpu_time_filter.py: the largest error / bound per run, the bound being the one the test computes per entry
(nothing of it measured), and whether the NaN positions are the restatement's.  Prints one JSON line with the worst ratio per dtype
and mode (the whole record is written to --out when given).

    python scripts/time_filter_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import time_filter_cases as C  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.prepare import time_filter  # noqa: E402

MODE_NAMES = {"s": "strict", "n": "strict_trim", "r": "renormalise"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _hip.Handle(0)
    runs, worst = [], {}
    for case, mode, complement in C.runs():
        for dtype in C.DTYPES:
            got = time_filter(C.case_field(case, dtype), C.case_weights(case), complement=complement, min_weight=case[6], handle=dev,
                              **C.MODES[mode])
            isnan, y, bound = C.reference(case, mode, complement, dtype)
            ratio = C.worst_ratio(got, isnan, y, bound)
            same = bool(np.array_equal(np.isnan(got), isnan))
            runs.append(dict(case=case[0], T=case[1], N=case[2], L=case[3], mode=MODE_NAMES[mode], complement=complement, dtype=dtype,
                             live=int((~isnan).sum()), entries=int(isnan.size), error_over_bound=ratio, nan_positions_as_expected=same))
            key = "%s_%s" % (dtype, MODE_NAMES[mode])
            worst[key] = max(worst.get(key, 0.0), ratio)
    res = {"what": "device time_filter() against the longdouble truth: worst error / bound over %d runs; the bound per entry is "
                   "2 [(L + 4) 2^-53 (sum |w x| + |S| sum_present |w|) / |den| + 2^-53 (|x_t| + |y|)] (+ half a float32 spacing at |y| "
                   "for float32), den = 1 and no |S| term in strict mode" % len(runs),
           "device": "MI355X (gfx950)", "tile": list(_hip.time_filter_tile()), "worst_error_over_bound": worst,
           "all_nan_positions_as_expected": all(r["nan_positions_as_expected"] for r in runs), "runs": runs}
    print(json.dumps({"worst_error_over_bound": worst, "all_nan_positions_as_expected": res["all_nan_positions_as_expected"],
                      "n_runs": len(runs)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
