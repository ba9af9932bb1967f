#!/usr/bin/env python3
"""solve(complexify=True, extend='theta', period=12) at C2 size (T = 2920 x N = 10 000 float64, tests/golden_inputs.gen_A): the
whole solve and, from the handle's stage timers, the Theta fit kernels (csrc/theta.h: seasonal means + drift, then the grid zoom
for alpha) and the products that form the imaginary planes.  Beside them the extend='exp' solve of the same input, for scale -
there is nothing to compare the theta solve with: the host route needs statsmodels and fits 20 000 models in a Python loop.
Prints one JSON line (also written to --out when given).  Reports numbers; asserts no threshold.

    python scripts/extend_theta_bench.py [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from golden_inputs import gen_A  # noqa: E402
from xmca_amd.array import MCA  # noqa: E402


def timed_solve(X, extend):
    m = MCA(X)
    dev = m._device()
    dev.reset_timings()
    t0 = time.perf_counter()
    m.solve(complexify=True, extend=extend, period=12)
    s = m.singular_values(10)          # (solve returns once the device result is there; the values are on the host already)
    return time.perf_counter() - t0, dev.timings(), s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    X = gen_A()
    res = {"case": "C2 EOF T=%d x N=%d float64, solve(complexify=True, extend=..., period=12); best of %d after a warm-up" % (X.shape + (args.reps,))}
    for extend in ("theta", "exp"):
        timed_solve(X, extend)                              # warm-up: code objects, pools, workspaces
        runs = [timed_solve(X, extend) for _ in range(args.reps)]
        best = min(runs, key=lambda r: r[0])
        res[extend] = {"solve_s": best[0], "solve_s_all": [r[0] for r in runs],
                       "stages_ms": {k: v for k, v in best[1].items() if k in ("theta_fit", "hilbert_extended")},
                       "sigma_1": float(best[2][0])}
    res["theta"]["fit_kernels_ms"] = res["theta"]["stages_ms"].get("theta_fit")
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
