#!/usr/bin/env python3
"""solve(complexify=True, extend='exp', period=12) and bootstrapping(10) of that model at C2 size (T = 2920 x N = 10 000
float64, tests/golden_inputs.gen_A): the device route (X_im = G X with the extended operator assembled on the GPU) against the
reference's host procedure (`_extend_on_host=True`: per-column regression and forecast, scipy.signal.hilbert of the 3T-long
series, complex upload - in every bootstrap replicate too).  Prints one JSON line (also written to --out when given).

    python scripts/extend_bench.py [--runs 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from golden_inputs import gen_A  # noqa: E402
from xmca_amd.array import MCA  # noqa: E402


def timed_solve(X, on_host):
    m = MCA(X)
    m._extend_on_host = on_host
    t0 = time.perf_counter()
    m.solve(complexify=True, extend='exp', period=12)
    s = m.singular_values(10)          # (solve returns once the device result is there; the values are on the host already)
    return m, time.perf_counter() - t0, s


def timed_bootstrap(m, runs):
    np.random.seed(5)
    t0 = time.perf_counter()
    out = m.bootstrapping(runs, n_modes=4)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    X = gen_A()
    timed_solve(X, False)                                   # warm-up: code objects, pools, workspaces
    md, t_dev, s_dev = timed_solve(X, False)
    mh, t_host, s_host = timed_solve(X, True)
    tb_dev, b_dev = timed_bootstrap(md, args.runs)
    tb_host, b_host = timed_bootstrap(mh, args.runs)
    res = {
        "case": "C2 EOF T=2920 x N=10000 float64, solve(complexify=True, extend='exp', period=12) + bootstrapping(%d, n_modes=4)" % args.runs,
        "solve_s": {"device": t_dev, "host_extension": t_host, "speedup": t_host / t_dev},
        "bootstrap_s": {"device": tb_dev, "host_extension": tb_host, "speedup": tb_host / tb_dev, "runs": args.runs},
        "sigma_rel_diff": float(np.max(np.abs(s_dev - s_host) / s_host)),
        "bootstrap_rel_diff": float(np.max(np.abs(b_dev - b_host)) / np.max(np.abs(b_host))),
    }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
