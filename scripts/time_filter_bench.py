#!/usr/bin/env python3
"""time_filter(X, lanczos_weights(L, 1 / 40)) of a real field against the only route there was before it: vectorised numpy on the
host threads.  The host route is the fastest one numpy offers at these shapes - the filter as a banded T x T matrix and one BLAS
product per plane (W @ X; with gaps W @ X0 and W @ P, then the quotient and the NaN rule) - so its time does not depend on L; a tap
loop over shifted slices runs on one thread and is slower at every L measured here.

Runs per shape and L in {25, 121, 1025}: float64 strict low-pass without gaps; float64 missing='renormalise' with 30 % random gaps
(numpy.random.default_rng(0)); and float32 strict once, at C2 and L = 121.  On the device both numpy in -> numpy out (upload and
download included) and GPU tensor in -> GPU tensor out.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A): `small`, 480 x 5 000 (L = 1025 is left out
there: the record is shorter than the filter), and `c2`, 2920 x 10 000.

The driver starts FRESH processes that alternate between the legs - host, device, host, device, ... - so that both see the same
session.  A process makes one warm-up call per run and route and then --repeats timed calls.  The record keeps the seconds per call
over all timed calls of all processes (median [min, max]), the stage timers of one device call, and the largest difference of the
two legs' results on a probe of entries, relative to max|X|.

    python scripts/time_filter_bench.py [--rounds 3] [--repeats 3] [--out profiles/time_filter_bench.json]

`--trace-leg` runs one tensor-to-tensor float64 call per L at C2 (strict, then renormalise with gaps) and nothing else, for a kernel
trace of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAPS, CUTOFF, MIN_WEIGHT = 0.3, 1.0 / 40.0, 0.5
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
LENGTHS = (25, 121, 1025)
STAGES = ("ingest_strided", "time_filter")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def runs_of(shapes):
    """(shape name, T, N, L, dtype, renormalise) of every run"""
    out = []
    for name, T, N in SHAPES:
        if name not in shapes:
            continue
        for L in LENGTHS:
            if L > T:
                continue
            out.append((name, T, N, L, "float64", False))
            out.append((name, T, N, L, "float64", True))
        if name == "c2":
            out.append((name, T, N, 121, "float32", False))
    return out


_FIELDS = {}


def field(T, N, gaps, dtype):
    key = (T, N)
    if key not in _FIELDS:
        sys.path.insert(0, os.path.join(HERE, "tests"))
        from golden_inputs import gen_A
        _FIELDS[key] = np.array(gen_A(T, N), dtype=np.float64)
    X = _FIELDS[key].astype(dtype)
    if gaps:
        X[np.random.default_rng(0).random((T, N)) < GAPS] = np.nan
    return X


def band_matrix(w, T, dtype):
    """the T x T matrix of the correlation, rows whose window leaves the record cut off at the edges"""
    L, h = len(w), len(w) // 2
    W = np.zeros((T, T), dtype=dtype)
    for k in range(L):
        d = k - h
        rows = np.arange(max(0, -d), min(T, T - d))
        W[rows, rows + d] = w[k]
    return W


def host_route(X, w, renormalise):
    """the vectorised numpy route: one BLAS product per plane"""
    T = X.shape[0]
    h = len(w) // 2
    W = band_matrix(w, T, X.dtype)
    if not renormalise:
        S = W @ X
        S[:h] = np.nan
        S[T - h:] = np.nan
        return S
    present = np.isfinite(X)
    num = W @ np.where(present, X, 0)
    den = W @ present.astype(X.dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(present & (den >= MIN_WEIGHT * w.sum()), num / den, np.nan).astype(X.dtype)


def _probe(F):
    flat = F.reshape(-1)
    return [float(v) for v in flat[flat.size // 3:: max(1, flat.size // 192)][:64]]


def leg(kind, repeats, shapes):
    """one process: every run; prints one JSON line"""
    sys.path.insert(0, HERE)
    from xmca_amd.prepare import lanczos_weights
    out = []
    if kind == "device":
        import torch
        torch.cuda.init()                      # (torch's runtime first, then the library's)
        from xmca_amd import _hip
        from xmca_amd.prepare import time_filter
        dev = _hip.default_handle()
    for name, T, N, L, dtype, renorm in runs_of(shapes):
        X = field(T, N, renorm, dtype)
        w = lanczos_weights(L, CUTOFF)
        kw = dict(missing="renormalise", min_weight=MIN_WEIGHT) if renorm else dict()
        entry = {"shape": name, "field": [T, N], "L": L, "dtype": dtype, "renormalise": renorm, "max_abs": float(np.nanmax(np.abs(X)))}
        if kind == "host":
            def call():
                t0 = time.perf_counter()
                F = host_route(X, w, renorm)
                return time.perf_counter() - t0, F
            routes = {"numpy": call}
        else:
            Xt = torch.from_numpy(X).to(torch.device("cuda", dev.device))

            def call_numpy():
                t0 = time.perf_counter()
                F = time_filter(X, w, handle=dev, **kw)
                return time.perf_counter() - t0, F

            def call_tensor():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                F = time_filter(Xt, w, handle=dev, **kw)          # (the call returns with its stream drained)
                return time.perf_counter() - t0, F
            routes = {"numpy_to_numpy": call_numpy, "tensor_to_tensor": call_tensor}
        for route, call in routes.items():
            first = call()[0]
            calls = [call() for _ in range(repeats)]
            F = calls[-1][1]
            F = F.cpu().numpy() if kind == "device" and route == "tensor_to_tensor" else F
            entry[route] = {"warmup_call_s": first, "s_per_call": [c[0] for c in calls], "probe": _probe(F),
                            "nan_fraction": float(np.isnan(F).mean())}
        if kind == "device":
            dev.reset_timings()
            call_tensor()
            entry["stages_ms_tensor_call"] = {k: v for k, v in dev.timings().items() if k in STAGES}
            del Xt
        out.append(entry)
    print("LEG " + json.dumps({"kind": kind, "cases": out}), flush=True)


def trace_leg():
    """one tensor-to-tensor call per L at C2 and nothing else: run under a kernel trace"""
    sys.path.insert(0, HERE)
    import torch
    torch.cuda.init()                          # (torch's runtime first, then the library's)
    from xmca_amd import _hip
    from xmca_amd.prepare import lanczos_weights, time_filter
    dev = _hip.default_handle()
    name, T, N = SHAPES[1]
    for renorm in (False, True):
        Xt = torch.from_numpy(field(T, N, renorm, "float64")).to(torch.device("cuda", dev.device))
        for L in LENGTHS:
            kw = dict(missing="renormalise", min_weight=MIN_WEIGHT) if renorm else dict()
            F = time_filter(Xt, lanczos_weights(L, CUTOFF), handle=dev, **kw)
            print("traced %s L = %d renormalise = %s: %.4f of the entries NaN" % (name, L, renorm, float(torch.isnan(F).double().mean())), flush=True)


def _run_leg(label, kind, repeats, shapes):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repeats", str(repeats), "--shapes", ",".join(shapes)],
                       capture_output=True, text=True, timeout=900)
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
    record = {"case": "time_filter(X, lanczos_weights(L, 1 / 40)): strict low-pass without gaps, and missing='renormalise' "
                      "(min_weight = %g) with %d %% gaps at random" % (MIN_WEIGHT, round(GAPS * 100)),
              "generator": "tests/golden_inputs.gen_A, gaps from default_rng(0)", "processes_per_leg": rounds,
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: host, device",
              "host_route": "vectorised numpy on the host threads (OMP_NUM_THREADS=%s): the filter as a banded T x T matrix, one BLAS "
                            "product per plane (W X; with gaps W X0 and W P, the quotient and the NaN rule); its time does not depend "
                            "on L" % os.environ.get("OMP_NUM_THREADS", "unset"),
              "cases": [],
              "not_measured": ["float32 fields other than C2 at L = 121", "complement=True (one more read of the tile's rows)",
                               "edges='trim'", "asymmetric or band-pass weights (the kernel does not look at the values)",
                               "the full-size C5 field", "more than one rank"]}
    for i in range(len(legs["host"][0]["cases"])):
        h = [p["cases"][i] for p in legs["host"]]
        d = [p["cases"][i] for p in legs["device"]]
        entry = {k: h[0][k] for k in ("shape", "field", "L", "dtype", "renormalise")}
        entry["host_numpy"] = {"s_per_call": _stats([t for p in h for t in p["numpy"]["s_per_call"]]),
                               "warmup_call_s": [p["numpy"]["warmup_call_s"] for p in h]}
        ref = np.array(h[-1]["numpy"]["probe"])
        for route in ("numpy_to_numpy", "tensor_to_tensor"):
            got = np.array(d[-1][route]["probe"])
            both = np.isfinite(ref) & np.isfinite(got)
            entry[route] = {"s_per_call": _stats([t for p in d for t in p[route]["s_per_call"]]),
                            "warmup_call_s": [p[route]["warmup_call_s"] for p in d], "nan_fraction": d[-1][route]["nan_fraction"],
                            "probe_nan_positions_as_host": bool(np.array_equal(np.isnan(ref), np.isnan(got))),
                            "probe_max_diff_to_host_over_max_abs": float(np.max(np.abs(got[both] - ref[both])) / h[0]["max_abs"]) if both.any() else None}
            entry[route]["speedup_median"] = entry["host_numpy"]["s_per_call"]["median"] / entry[route]["s_per_call"]["median"]
            entry[route]["max_below_host_min"] = entry[route]["s_per_call"]["max"] < entry["host_numpy"]["s_per_call"]["min"]
        entry["stages_ms_tensor_call"] = [p["stages_ms_tensor_call"] for p in d]
        record["cases"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process, run and route")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["device", "host"], help="(internal) measure one leg in this process")
    ap.add_argument("--trace-leg", action="store_true", help="one C2 call per L of this revision, for a kernel trace")
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
