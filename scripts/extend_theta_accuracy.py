#!/usr/bin/env python3
"""Observed errors of the device's Theta fits and imaginary planes against the numpy restatement (tests/theta_cases.py), over the
shapes of tests/test_gpu_theta_extension.py: m in {1, 2, 3, 4, 12}, T in {2m, 2m + 1, one more}, N = 130, float32 and float64
fields.  Per case: the largest alpha difference (bound 2 * 16^-6), the largest ratio of a difference in b0 / level / s to its bound,
and the largest plane difference with its bound - the bounds of `theta_cases.tolerances`, derived from the restatement alone.
Prints one JSON line (also written to --out when given).

    python scripts/extend_theta_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import theta_cases as tc  # noqa: E402
from xmca_amd import _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _hip.Handle(0)
    cases, worst = [], {"alpha": 0.0, "fit_over_bound": 0.0, "planes_over_bound": 0.0, "first_round_gap": float("inf")}
    for m in tc.M_VALUES:
        for T in tc.lengths(m):
            for dtype in (np.float64, np.float32):
                X = tc.columns(T, 130, m, seed=100 * m + T).astype(dtype)
                dev.set_field(0, X)
                fit = dev.theta_fit(0, X.shape[1], m)
                dev.complexify_theta(T, m)
                im = dev.get_field_imag(0, X.shape)
                X64 = X.astype(np.float64)
                pair = tc.checked_fits(X64, m)
                tol = tc.tolerances(X64, m, pair)
                err = np.abs(fit - tc.packed(pair))
                err_im = float(np.abs(im - tc.analytic_signal(X64, m, pair).imag).max())
                gap = min(tc.first_round_gap(f["first_round"]) for f in pair)
                case = {"m": m, "T": T, "N": X.shape[1], "dtype": np.dtype(dtype).name, "alpha_diff": float(err[:, 0].max()),
                        "fit_over_bound": float((err[:, 1:] / tol["fit"][:, 1:]).max()), "planes_diff": err_im,
                        "planes_bound": float(tol["planes"]), "first_round_gap": None if np.isinf(gap) else float(gap)}
                cases.append(case)
                worst["alpha"] = max(worst["alpha"], case["alpha_diff"])
                worst["fit_over_bound"] = max(worst["fit_over_bound"], case["fit_over_bound"])
                worst["planes_over_bound"] = max(worst["planes_over_bound"], err_im / case["planes_bound"])
                worst["first_round_gap"] = min(worst["first_round_gap"], gap)
    res = {"what": "device Theta fits and planes against the numpy restatement", "alpha_bound": tc.ALPHA_STEP, "worst": worst, "cases": cases}
    line = json.dumps(res)
    print(json.dumps({"worst": worst, "n_cases": len(cases)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
