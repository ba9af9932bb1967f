#!/usr/bin/env python3
"""homogeneous_patterns() / heterogeneous_patterns() on the device route (xmca_correlation_maps: correlations, p-values and the final
layout on the device) against the host route (`_patterns_on_host=True`: xmca_correlate, then scipy.special.betainc and the NaN
re-insertion in numpy - what the class did before ABI 13) on the same seeded inputs.

Legs: C2 (T = 2920 x N = 10 000 float64, tests/golden_inputs.gen_A) after rotate(10): homogeneous_patterns(10); c5_scaled (float32,
1200 x 144 x 288, NaN columns added here) after rotate(10): homogeneous_patterns(10); c3_reduced (two float64 fields, 1000 x 4000 and
1000 x 3000) after rotate(10): heterogeneous_patterns(10).  Each route has a handle of its own, so neither evicts the other's
resident result.  Every call returns after a stream synchronise (the entry points copy the result to the host); the first call of
each leg is the warm-up (it also fetches what the PCs need) and is reported apart, then --repeats timed calls, the two routes
alternating (min / median / max).  `separated` says whether the device route's median is below the host route's median by more than
the host route's own min-max spread.  Prints one JSON line (also written to --out).

    python scripts/patterns_bench.py [--repeats 7] [--out FILE]
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

from golden_inputs import gen_A, gen_C, make_input  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.array import MCA  # noqa: E402


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def _models(fields, rot):
    out = {}
    for route in ("device", "host"):
        m = MCA(*fields, handle=_hip.Handle(0))
        m._patterns_on_host = route == "host"
        m.solve()
        m.rotate(rot)
        out[route] = m
    return out


def _diff(dev, host):
    """largest |r_device - r_host| and largest relative p difference over the p above 1e-250 (both routes, every field)"""
    (rd, pd), (rh, ph) = dev, host
    dr = dp = 0.0
    for k in rd:
        if not (np.array_equal(np.isnan(rd[k]), np.isnan(rh[k])) and np.array_equal(np.isnan(pd[k]), np.isnan(ph[k]))):
            return {"error": "NaN patterns differ"}
        if rd[k].dtype != rh[k].dtype or rd[k].shape != rh[k].shape:
            return {"error": "dtypes / shapes differ"}
        dr = max(dr, float(np.nanmax(np.abs(rd[k] - rh[k]))))
        ok = ph[k] >= 1e-250
        dp = max(dp, float(np.max(np.abs(pd[k][ok] - ph[k][ok]) / ph[k][ok])))
    return {"max_abs_r_diff": dr, "max_rel_p_diff": dp}


def _leg(name, models, call, repeats, values):
    res = {"leg": name, "values_per_map": values}
    outs, ts = {}, {"device": [], "host": []}
    for route, m in models.items():
        t0 = time.perf_counter()
        outs[route] = call(m)
        res[route + "_first_s"] = time.perf_counter() - t0
    for _ in range(repeats):
        for route, m in models.items():
            t0 = time.perf_counter()
            call(m)
            ts[route].append(time.perf_counter() - t0)
    for route in ts:
        res[route + "_s"] = _stats(ts[route])
    res["speedup_median"] = res["host_s"]["median"] / res["device_s"]["median"]
    res["separated"] = res["host_s"]["median"] - res["device_s"]["median"] > res["host_s"]["max"] - res["host_s"]["min"]
    res.update(_diff(outs["device"], outs["host"]))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = []
    X = gen_A()
    ms = _models((X,), 10)
    legs.append(_leg("c2_rot10_homogeneous_10", ms, lambda m: m.homogeneous_patterns(10), args.repeats, X.shape[1] * 10))
    del ms, X
    C = gen_C(1200, 144, 288).copy()
    C[:, 3:7, 10:20] = np.nan                        # land points: masked columns
    ms = _models((C,), 10)
    legs.append(_leg("c5_scaled_rot10_homogeneous_10", ms, lambda m: m.homogeneous_patterns(10), args.repeats, C[0].size * 10))
    del ms, C
    A, B = make_input("c3_reduced")
    ms = _models((A, B), 10)
    legs.append(_leg("c3_reduced_rot10_heterogeneous_10", ms, lambda m: m.heterogeneous_patterns(10), args.repeats,
                     (A.shape[1] + B.shape[1]) * 10))
    res = {"case": "patterns bench: device (xmca_correlation_maps) vs _patterns_on_host", "repeats": args.repeats, "legs": legs}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
