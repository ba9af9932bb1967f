#!/usr/bin/env python3
"""Observed errors of `xmca_amd.prepare.anomalies` against the numpy restatement (tests/anomalies_cases.py) over every case, gap
pattern and dtype of tests/test_gpu_anomalies.py: the field and the coefficients against `lstsq`, the weighted mean of the residual
along every basis column, and the coefficients of a second application.  float64 figures are in units of max|X|, float32 fields
in float32 ulps of max|X| (tests/anomalies_cases.py `figures`).  Prints one JSON line with the worst figures (the whole record is
written to --out when given); the bounds of the tests are these worst figures times 8.

    python scripts/anomalies_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import anomalies_cases as C  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.prepare import anomalies  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _hip.Handle(0)
    cases, worst = [], {}
    for case in C.CASES:
        for pattern in C.patterns_of(case):
            for dtype in ("float64", "float32"):
                X, expected = C.case_field(case, pattern, dtype)
                B = C.basis_of(case)
                out = anomalies(X, basis=B, handle=dev)
                again = anomalies(out["field"], basis=B, handle=dev)
                fig = C.figures(case, pattern, dtype, out, again)
                fig["fitted_as_expected"] = bool(np.array_equal(out["fitted"], expected))
                cases.append(dict(case=C.case_name(case), pattern=pattern, dtype=dtype, **fig))
                for name, v in fig.items():
                    if name != "fitted_as_expected":
                        key = name + "_" + dtype
                        worst[key] = max(worst.get(key, 0.0), v)
    res = {"what": "device anomalies() against the numpy lstsq restatement: worst figures over %d runs; float64 in units of max|X|, "
                   "float32 field / orthogonality / refit in float32 ulps of max|X|, coefficients in max|X|" % len(cases),
           "device": "MI355X (gfx950)", "worst": worst,
           "bounds": {"float64_of_max_abs_X": 8 * worst["field_float64"], "float64_rule": "8 x worst field_float64; must stay below 1e-11",
                      "float32_ulps_of_max_abs_X": 1.0,
                      "float32_rule": "one float32 spacing at max|X|: both sides round a float64 residual no larger than max|X| once, and "
                                      "the float64 values differ by far less than a spacing; measured worst field_float32 = %g"
                                      % worst["field_float32"]},
           "all_fitted_as_expected": all(c["fitted_as_expected"] for c in cases), "cases": cases}
    print(json.dumps({"worst": worst, "all_fitted_as_expected": res["all_fitted_as_expected"], "n_runs": len(cases)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
