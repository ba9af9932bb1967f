#!/usr/bin/env python3
"""Observed errors of `xmca_amd.lagged.lead_lag_maps` against the longdouble truth of tests/lead_lag_cases.py over every case, dtype
and dof mode of tests/test_gpu_lead_lag.py: the largest error / bound of r and of slope per run, the bound being the one the test
computes per entry (nothing of it measured), the largest p error / allowance against scipy, and whether `pairs`, `dof` and the NaN
positions are the restatement's.  Prints one JSON line with the worst ratios per dtype and mode (the whole record is written to --out
when given).

    python scripts/lead_lag_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import lead_lag_cases as C  # noqa: E402
from test_gpu_lead_lag import p_ratio  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.lagged import lead_lag_maps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _hip.Handle(0)
    runs, worst = [], {}
    for case in C.CASES:
        name, T, N, q, lags, pattern, min_pairs = case
        for dtype in C.DTYPES:
            for dof in C.DOFS:
                got = lead_lag_maps(C.case_field(case, dtype), C.case_index(case), lags, min_pairs=min_pairs, dof=dof, handle=dev)
                rest, truth, br, bs = C.reference(name, dtype, dof)
                live = rest["live"]
                exact = bool(np.array_equal(got["pairs"], rest["pairs"]) and np.array_equal(got["dof"], rest["dof"])
                             and np.array_equal(np.isnan(got["r"]), ~live) and np.array_equal(np.isnan(got["slope"]), ~live)
                             and np.array_equal(np.isnan(got["p"]), ~live | (rest["dof"] < 3)))
                ratios = dict(r=C.worst_ratio(got["r"], truth["r"], br, live), slope=C.worst_ratio(got["slope"], truth["slope"], bs, live),
                              p=p_ratio(got["p"], got["r"], got["dof"]))
                runs.append(dict(case=name, T=T, N=N, q=q, lags=len(lags), gaps=pattern, min_pairs=min_pairs, dtype=dtype, dof=dof,
                                 live=int(live.sum()), entries=int(live.size), error_over_bound=ratios, integers_and_nan_positions_exact=exact))
                for k, v in ratios.items():
                    key = "%s_%s_%s" % (dtype, dof, k)
                    worst[key] = max(worst.get(key, 0.0), v)
    res = {"what": "device lead_lag_maps() against the longdouble truth: worst error / bound over %d runs; per entry, with u = 2^-53 and n "
                   "pairs, d(Cab) = 2 (n + 6) u [sum |a' b'| + sum |a'| sum |b'| / n], dr = dCxy / sqrt(Cxx Cyy) + (|r| / 2) (dCxx / Cxx + "
                   "dCyy / Cyy) + 2 u |r|, dslope = dCxy / Cyy + |slope| dCyy / Cyy + 2 u |slope|, the allowance 2 d (+ half a float32 "
                   "spacing at the value for float32); p against scipy at the device's own r and dof, within the allowance of "
                   "tests/test_gpu_patterns.py" % len(runs),
           "device": "MI355X (gfx950)", "tile": list(_hip.lead_lag_tile()), "worst_error_over_bound": worst,
           "all_integers_and_nan_positions_exact": all(r["integers_and_nan_positions_exact"] for r in runs), "runs": runs}
    print(json.dumps({"worst_error_over_bound": worst, "all_integers_and_nan_positions_exact": res["all_integers_and_nan_positions_exact"],
                      "n_runs": len(runs)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
