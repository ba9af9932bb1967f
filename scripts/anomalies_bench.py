#!/usr/bin/env python3
"""anomalies(X, period=12, trend=True) - monthly means and a trend, k = 13 - of a real float64 field against the only route there
was before it: vectorised numpy on the host threads (`X - B (B^+ X)` without gaps; with gaps the masked normal equations by one
product per moment and a batched `numpy.linalg.solve`).  Measured per shape without gaps and with 30 % random gaps
(numpy.random.default_rng(0)), and on the device both numpy in -> numpy out (upload and download included) and GPU tensor in ->
GPU tensor out.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A, float64): `small`, 480 x 5 000, and `c2`,
2920 x 10 000.

The driver starts FRESH processes that alternate between the legs - host, device, host, device, ... - so that both see the same
session.  A process makes one warm-up call per shape, gap setting and route and then --repeats timed calls.  The record keeps the
seconds per call over all timed calls of all processes (median [min, max]), the stage timers of one device call, and the largest
difference of the two legs' results on a probe of entries, relative to max|X|.

    python scripts/anomalies_bench.py [--rounds 3] [--repeats 3] [--out profiles/anomalies_bench.json]

`--trace-leg` runs one C2 call with gaps (numpy in, numpy out) and nothing else, for a kernel trace of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD, GAPS = 12, 0.3
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
STAGES = ("reg_mask", "reg_moments", "reg_solve", "reg_residual")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def field(T, N, gaps):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from golden_inputs import gen_A
    X = np.array(gen_A(T, N), dtype=np.float64)
    if gaps:
        hole = np.random.default_rng(0).random((T, N)) < GAPS
        hole[:2 * PERIOD] = False                 # (every grid point keeps two full periods: all of them are fitted)
        X[hole] = np.nan
    return X


def host_route(X, B):
    """the vectorised numpy route"""
    present = np.isfinite(X)
    if present.all():
        return X - B @ (np.linalg.pinv(B) @ X)
    k = B.shape[1]
    X0 = np.where(present, X, 0.0)
    pairs = (B[:, :, None] * B[:, None, :]).reshape(B.shape[0], k * k)
    G = (pairs.T @ present.astype(np.float64)).T.reshape(-1, k, k)
    c = np.linalg.solve(G, (B.T @ X0).T[:, :, None])[:, :, 0].T
    return np.where(present, X - B @ c, np.nan)


def _probe(F):
    flat = F.reshape(-1)
    return [float(v) for v in flat[:: max(1, flat.size // 64)][:64]]


def leg(kind, repeats, shapes):
    """one process: every shape and gap setting; prints one JSON line"""
    sys.path.insert(0, HERE)
    from xmca_amd.prepare import time_basis
    out = []
    if kind == "device":
        import torch
        from xmca_amd import _hip
        from xmca_amd.prepare import anomalies
        dev = _hip.default_handle()
    for name, T, N in SHAPES:
        if name not in shapes:
            continue
        B = time_basis(T, period=PERIOD, trend=True)
        for gaps in (False, True):
            X = field(T, N, gaps)
            entry = {"shape": name, "field": [T, N], "gaps": gaps, "max_abs": float(np.nanmax(np.abs(X)))}
            if kind == "host":
                def call():
                    t0 = time.perf_counter()
                    F = host_route(X, B)
                    return time.perf_counter() - t0, F
                routes = {"numpy": call}
            else:
                Xt = torch.from_numpy(X).to(torch.device("cuda", dev.device))

                def call_numpy():
                    t0 = time.perf_counter()
                    F = anomalies(X, basis=B, handle=dev)["field"]
                    return time.perf_counter() - t0, F

                def call_tensor():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    F = anomalies(Xt, basis=B, handle=dev)["field"]          # (the call returns with its stream drained)
                    return time.perf_counter() - t0, F
                routes = {"numpy_to_numpy": call_numpy, "tensor_to_tensor": call_tensor}
            for route, call in routes.items():
                first = call()[0]
                calls = [call() for _ in range(repeats)]
                F = calls[-1][1]
                F = F.cpu().numpy() if kind == "device" and route == "tensor_to_tensor" else F
                entry[route] = {"warmup_call_s": first, "s_per_call": [c[0] for c in calls], "probe": _probe(F),
                                "all_fitted": bool(np.array_equal(np.isnan(F), np.isnan(X)))}
            if kind == "device":
                dev.reset_timings()
                call_tensor()
                entry["stages_ms_tensor_call"] = {k: v for k, v in dev.timings().items() if k in STAGES + ("ingest_strided",)}
            out.append(entry)
    print("LEG " + json.dumps({"kind": kind, "cases": out}), flush=True)


def trace_leg():
    """one call at C2 with gaps and nothing else: run under a kernel trace"""
    sys.path.insert(0, HERE)
    from xmca_amd.prepare import anomalies
    name, T, N = SHAPES[int(os.environ.get("TRACE_SHAPE", "1"))]
    out = anomalies(field(T, N, True), period=PERIOD, trend=True)
    print("traced %s: %d of %d grid points fitted" % (name, int(out["fitted"].sum()), N), flush=True)


def _run_leg(label, kind, repeats, shapes):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repeats", str(repeats), "--shapes", ",".join(shapes)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("the %s leg failed (exit %d):\n%s" % (label, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
    print("%s done" % label, flush=True)
    return json.loads(line[4:])


def drive(rounds, repeats, shapes):
    legs = {"host": [], "device": []}
    for rnd in range(rounds):
        for kind in ("host", "device"):
            legs[kind].append(_run_leg("round %d %s" % (rnd, kind), kind, repeats, shapes))
    record = {"case": "anomalies(X, period=%d, trend=True): k = %d basis columns; gaps: %d %% at random after the first two periods"
                      % (PERIOD, PERIOD + 1, round(GAPS * 100)), "dtype": "float64",
              "generator": "tests/golden_inputs.gen_A, gaps from default_rng(0)", "processes_per_leg": rounds,
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: host, device",
              "host_route": "vectorised numpy on the host threads (OMP_NUM_THREADS=%s): X - B (pinv(B) X) without gaps; masked normal "
                            "equations by one product per moment and a batched solve with gaps" % os.environ.get("OMP_NUM_THREADS", "unset"),
              "cases": [],
              "not_measured": ["float32 fields at benchmark size", "the full-size C5 field", "more than one rank",
                               "the chunked column pass as the route to the moments (only the GEMM route was built)"]}
    for i in range(len(legs["host"][0]["cases"])):
        h = [p["cases"][i] for p in legs["host"]]
        d = [p["cases"][i] for p in legs["device"]]
        entry = {"shape": h[0]["shape"], "field": h[0]["field"], "gaps": h[0]["gaps"],
                 "host_numpy": {"s_per_call": _stats([t for p in h for t in p["numpy"]["s_per_call"]]),
                                "warmup_call_s": [p["numpy"]["warmup_call_s"] for p in h]}}
        ref = np.array(h[-1]["numpy"]["probe"])
        for route in ("numpy_to_numpy", "tensor_to_tensor"):
            entry[route] = {"s_per_call": _stats([t for p in d for t in p[route]["s_per_call"]]),
                            "warmup_call_s": [p[route]["warmup_call_s"] for p in d],
                            "all_fitted": all(p[route]["all_fitted"] for p in d),
                            "probe_max_diff_to_host_over_max_abs": float(np.nanmax(np.abs(np.array(d[-1][route]["probe"]) - ref)) / h[0]["max_abs"])}
            entry[route]["speedup_median"] = entry["host_numpy"]["s_per_call"]["median"] / entry[route]["s_per_call"]["median"]
            entry[route]["max_below_host_min"] = entry[route]["s_per_call"]["max"] < entry["host_numpy"]["s_per_call"]["min"]
        entry["stages_ms_tensor_call"] = [p["stages_ms_tensor_call"] for p in d]
        record["cases"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process, shape, gap setting and route")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["device", "host"], help="(internal) measure one leg in this process")
    ap.add_argument("--trace-leg", action="store_true", help="one C2 call of this revision, for a kernel trace")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.trace_leg:
        trace_leg()
        return
    if args.leg:
        leg(args.leg, args.repeats, shapes)
        return
    record = drive(args.rounds, args.repeats, shapes)
    print(json.dumps(record)[:6000], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
