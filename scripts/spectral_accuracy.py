#!/usr/bin/env python3
"""Observed errors of `xmca_amd.spectral.spectral_maps` against the longdouble truth of tests/spectral_cases.py over every case and
dtype of tests/test_gpu_spectral.py: the largest error / bound of every map per run, the bound being the one the test computes per
entry (nothing of it measured), the largest p error / allowance at the device's own coherence, and whether `segments` and the NaN
positions are the restatement's.  Prints one JSON line with the worst ratios per dtype (the whole record is written to --out when
given).

    python scripts/spectral_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import spectral_cases as C  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.spectral import spectral_maps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _hip.Handle(0)
    runs, worst = [], {}
    for case in C.CASES:
        name, T, N, q, L, step, window, detrend, bins, pattern, ms = case
        for dtype in C.DTYPES:
            X, index, kw = C.case_call(case, dtype)
            got = spectral_maps(X, index, nperseg=L, handle=dev, **kw)
            rest, truth, allow, phase_ok = C.reference(name, dtype)
            exact = bool(np.array_equal(got["segments"], rest["segments"]))
            ratios = {}
            for key in C.MAPS[:1 if q == 0 else None]:
                live = C.live_of(rest, key)
                exact = exact and bool(np.array_equal(np.isnan(got[key]), ~live))
                ratios[key] = C.worst_ratio(got[key], truth[key], allow[key], phase_ok if key == "phase" else live, circular=key == "phase")
            if q:
                exact = exact and bool(np.array_equal(np.isnan(got["p"]), ~rest["live"]))
                ratios["p"] = C.p_ratio(got["p"], got["coherence"], rest["ke"], rest["live"])
            runs.append(dict(case=name, T=T, N=N, q=q, nperseg=L, step=step, window=window, detrend=detrend, bins=len(bins), gaps=pattern,
                             min_segments=ms, dtype=dtype, live_columns=int(rest["col_live"].sum()),
                             live_ratio_entries=int(rest["live"].sum()) if q else 0, phases_compared=int(phase_ok.sum()) if q else 0,
                             error_over_bound=ratios, segments_and_nan_positions_exact=exact))
            for k, v in ratios.items():
                worst["%s_%s" % (dtype, k)] = max(worst.get("%s_%s" % (dtype, k), 0.0), v)
    res = {"what": "device spectral_maps() against the longdouble truth (unrounded tables): worst error / bound over %d runs; per entry, with "
                   "u = 2^-53, each part of a segment's Z within dz = (L + 4) u (sum |w x'| + |W_k| sum |x'| / L), Z within ez = sqrt(2) dz; "
                   "dSxx = sum_m (2 |Z| ez + ez^2) + (K_n + 3) u Sxx, dSyy likewise, dC = sqrt(2) [sum_m (|Y| ez + |Z| ey + ey ez) + "
                   "(2 K_n + 3) u sum_m |Y| |Z|]; d power = scale dSxx + 5 u power, d coherence = 2 |C| dC / (Sxx Syy) + coherence (dSxx / Sxx + "
                   "dSyy / Syy + 6 u), d gain = dC / Syy + gain (dSyy / Syy + 4 u), d phase = dC / |C| + 4 pi u where |C| > 2^10 dC; the "
                   "allowance 2 d (+ half a float32 spacing at the value for float32); p against (1 - coherence)^(Ke - 1) in longdouble at the "
                   "device's own coherence within 16 u (1 + |ln p|) p" % len(runs),
           "device": "MI355X (gfx950)", "tile": list(_hip.spectral_tile()), "worst_error_over_bound": worst,
           "all_segments_and_nan_positions_exact": all(r["segments_and_nan_positions_exact"] for r in runs), "runs": runs}
    print(json.dumps({"worst_error_over_bound": worst, "all_segments_and_nan_positions_exact": res["all_segments_and_nan_positions_exact"],
                      "n_runs": len(runs)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
