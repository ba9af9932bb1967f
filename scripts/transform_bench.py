#!/usr/bin/env python3
"""predict() and reconstructed_fields() on the device (xmca_predict / xmca_reconstruct) against the host route
(`_transform_on_host=True`: vectors fetched, numpy products, host scaling and NaN re-insertion) on the same seeded inputs.

Legs: C2 (T = 2920 x N = 10 000 float64, tests/golden_inputs.gen_A) predict(X_train) unrotated with n=None and after rotate(10),
reconstructed_fields(10) and reconstructed_fields() of the unrotated model; c5_scaled (float32, 1200 x 144 x 288, NaN columns
added here) after rotate(10): predict(X_train, n=10) and reconstructed_fields(10).  Each route has a handle of its own, so neither
evicts the other's resident result.  Every call returns after a stream synchronise (the entry points copy the result to the
host); the first call of each leg is the warm-up, then --repeats timed calls (min / median / max).  The host route's first call
also fetches the vectors: it is reported apart (`host_first_s`).  PCIe bytes follow from the sizes of the copies each route makes.
Prints one JSON line (also written to --out).

    python scripts/transform_bench.py [--repeats 5] [--out FILE] [--device-only]
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

from golden_inputs import gen_A, gen_C  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.array import MCA  # noqa: E402


def _timed(fn, repeats):
    t0 = time.perf_counter()
    out = fn()
    first = time.perf_counter() - t0
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return out, first, ts


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def _diff(a, b):
    a, b = a[next(iter(a))], b[next(iter(b))]
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return "NaN patterns differ"
    if not np.isfinite(b).any():
        return "both all NaN (a null mode, sigma = 0, enters: 0 / 0 as in the reference)"
    return float(np.nanmax(np.abs(a - b)) / np.nanmax(np.abs(b)))


def _models(X, rot, device_only):
    out = {}
    for route in ("device",) + (() if device_only else ("host",)):
        m = MCA(X, handle=_hip.Handle(0))
        m._transform_on_host = route == "host"
        m.solve()
        if rot:
            m.rotate(rot)
        out[route] = m
    return out


def _leg(name, models, call, repeats, pcie):
    res = {"leg": name}
    outs = {}
    for route, m in models.items():
        out, first, ts = _timed(lambda: call(m), repeats)
        outs[route] = out
        res[route + "_s"] = _stats(ts)
        if route == "host":
            res["host_first_s"] = first
    if "host" in outs:
        res["speedup_median"] = res["host_s"]["median"] / res["device_s"]["median"]
        res["max_rel_diff"] = _diff(outs["device"], outs["host"])
    res["pcie_bytes"] = pcie
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    legs = []
    X = gen_A()
    T, N = X.shape
    r = min(T, N)
    ms = _models(X, None, args.device_only)
    legs.append(_leg("c2_predict_unrotated_all", ms, lambda m: m.predict(X), args.repeats,
                     {"device": 8 * (T * N + T * r + r * r), "host_first_call": 8 * N * r}))
    legs.append(_leg("c2_reconstruct_10", ms, lambda m: m.reconstructed_fields(10), args.repeats,
                     {"device": 8 * (T * N + 2 * T * 10), "host_first_call": 8 * (N * 10 + T * 10)}))
    legs.append(_leg("c2_reconstruct_all", ms, lambda m: m.reconstructed_fields(), args.repeats,
                     {"device": 8 * (T * N + 2 * T * r), "host_first_call": 8 * (N * r + T * r)}))
    for m in ms.values():
        m.rotate(10)
    legs.append(_leg("c2_predict_rot10", ms, lambda m: m.predict(X), args.repeats,
                     {"device": 8 * (T * N + T * 10 + 10 * 10), "host_first_call": 8 * N * r}))
    del ms
    (C,) = (gen_C(1200, 144, 288),)
    C = C.copy()
    C[:, 3:7, 10:20] = np.nan                        # land points: masked columns
    Tc, Nc = C.shape[0], C[0].size
    ms = _models(C, 10, args.device_only)
    Nk = ms["device"]._fields_store["left"].shape[1]
    rc = min(Tc, Nk)
    legs.append(_leg("c5_scaled_rot10_predict", ms, lambda m: m.predict(C, n=10), args.repeats,
                     {"device": 4 * Tc * Nc + 8 * Tc * 10, "host_first_call": 4 * Nk * rc}))
    legs.append(_leg("c5_scaled_rot10_reconstruct_10", ms, lambda m: m.reconstructed_fields(10), args.repeats,
                     {"device": 8 * (Tc * Nc + 2 * Tc * 10), "host_first_call": 4 * Nk * rc + 8 * Tc * 10}))
    res = {"case": "transform bench: device (xmca_predict / xmca_reconstruct) vs _transform_on_host", "repeats": args.repeats,
           "legs": legs}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
