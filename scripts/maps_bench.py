#!/usr/bin/env python3
"""eofs(scaling=...) / spatial_amplitude() / spatial_phase() on the device route (xmca_get_maps: factors, divisors, amplitude / phase and
the NaN rows of masked grid points on the device) against the numpy route (`_maps_on_host=True`: xmca_get_eofs, then the scaling, mask
and amplitude / phase passes over N x q in numpy - what the class did before xmca_get_maps) on the same seeded inputs.

Only the public getters and the `_maps_on_host` attribute are used, so the same file runs on a commit without the device route: the
attribute is ignored there and both columns are the old code - the baseline.  `--baseline FILE` reads such an output and adds, per
leg, the baseline's figures of the 'device' column and whether this run's device-route median stays within the baseline's median plus
its own min-max spread.

Legs: C2 (T = 2920 x N = 10 000 float64, tests/golden_inputs.gen_A) after rotate(10): eofs(10, 'max'), eofs(10, 'std'); c5_scaled
(float32, 1200 x 144 x 288, NaN columns added here) after rotate(10): eofs(10), eofs(10, 'max'), eofs(10, 'std'); c3_reduced (two
float64 fields, 1000 x 4000 and 1000 x 3000) complexified, after rotate(10, 2): spatial_amplitude(10, 'max'), spatial_phase(10);
with --c5-full the 1200 x 720 x 1440 float32 field after rotate(10): eofs(10, 'max').  Each route has a handle of its own, so neither
evicts the other's resident result.  Every call returns after a stream synchronise (the entry points copy the result to the host);
the first call of each leg is reported apart, then --repeats timed calls, the two routes alternating (min / median / max).
`separated` says whether the device route's median is below the numpy route's median by more than the numpy route's own min-max
spread.  Prints one JSON line per leg and one for the whole run (also written to --out).

    python scripts/maps_bench.py [--repeats 9] [--c5-full] [--baseline FILE] [--out FILE]
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


def _models(fields, cplx, rot):
    out = {}
    for route in ("device", "host"):
        m = MCA(*fields, handle=_hip.Handle(0))
        m._maps_on_host = route == "host"
        m.solve(complexify=cplx)
        m.rotate(*rot)
        out[route] = m
    return out


def _diff(dev, host, circular):
    """largest |device - host| over the largest |host|, every field; phases (`circular`): largest circular distance in radians"""
    worst = 0.0
    for k in dev:
        if dev[k].dtype != host[k].dtype or dev[k].shape != host[k].shape:
            return {"error": "dtypes / shapes differ"}
        if not np.array_equal(np.isnan(dev[k]), np.isnan(host[k])):
            return {"error": "NaN patterns differ"}
        if circular:
            worst = max(worst, float(np.nanmax(np.abs(np.angle(np.exp(1j * (dev[k] - host[k])))))))
        else:
            worst = max(worst, float(np.nanmax(np.abs(dev[k] - host[k])) / np.nanmax(np.abs(host[k]))))
    return {"max_circular_diff_rad" if circular else "max_rel_diff": worst}


def _leg(name, models, call, repeats, values, baseline):
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
    res["resident"] = all(set(m._V._pending) == set(m._keys) for m in models.values())      # nothing was fetched by either route
    res.update(_diff(outs["device"], outs["host"], "phase" in name))
    base = baseline.get(name)
    if base is not None:
        b = base["device_s"]
        res["baseline_s"] = b
        res["speedup_median_over_baseline"] = b["median"] / res["device_s"]["median"]
        res["within_baseline_spread"] = res["device_s"]["median"] <= b["median"] + (b["max"] - b["min"])
        res["separated_from_baseline"] = b["median"] - res["device_s"]["median"] > b["max"] - b["min"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--c5-full", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    baseline = {}
    if args.baseline:
        with open(args.baseline) as fh:
            baseline = {leg["leg"]: leg for leg in json.loads(fh.readline())["legs"]}
    legs = []

    def run(prefix, models, calls, values):
        for name, call in calls:
            legs.append(_leg(prefix + "_" + name, models, call, args.repeats, values, baseline))

    X = gen_A()
    run("c2_rot10", _models((X,), False, (10,)),
        [("eofs_10_max", lambda m: m.eofs(10, scaling='max')), ("eofs_10_std", lambda m: m.eofs(10, scaling='std'))], X.shape[1] * 10)
    del X
    C = gen_C(1200, 144, 288).copy()
    C[:, 3:7, 10:20] = np.nan                        # land points: masked columns
    run("c5_scaled_masked_rot10", _models((C,), False, (10,)),
        [("eofs_10", lambda m: m.eofs(10)), ("eofs_10_max", lambda m: m.eofs(10, scaling='max')),
         ("eofs_10_std", lambda m: m.eofs(10, scaling='std'))], C[0].size * 10)
    del C
    A, B = make_input("c3_reduced")
    run("c3_reduced_complex_rot10p2", _models((A, B), True, (10, 2)),
        [("spatial_amplitude_10_max", lambda m: m.spatial_amplitude(10, scaling='max')),
         ("spatial_phase_10", lambda m: m.spatial_phase(10))], (A.shape[1] + B.shape[1]) * 10)
    del A, B
    if args.c5_full:
        C = gen_C()
        run("c5_full_rot10", _models((C,), False, (10,)), [("eofs_10_max", lambda m: m.eofs(10, scaling='max'))], C[0].size * 10)
        del C
    res = {"case": "maps bench: device (xmca_get_maps) vs _maps_on_host", "repeats": args.repeats,
           "device_route_present": hasattr(_hip.Handle, "maps"), "legs": legs}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
