#!/usr/bin/env python3
"""spectral_maps(X, index, nperseg=256) - step 128, Hann, detrend='mean', all 129 bins - against the host route, scipy.signal on the host
threads.

The host route.  Without gaps: scipy.signal.welch of the field and of the index and scipy.signal.csd(index_j, X) along time, whole
planes at once (scipy's FFT over all columns); coherence, phase, gain and p from those in numpy.  With gaps scipy refuses the NaN, so
the host gets the per-column masked loop: for every column the present segments are found from a running count of missing values,
stacked into one series, and scipy averages over exactly those with nperseg = L and noverlap = 0 - welch(x), and per index series
welch(y_j) and csd(y_j, x) over the same segments.  The columns are shared among the host threads.

Gaps: 30 % of every column is missing as one run (an outage), at a place that moves with the column (37 n mod the free length) -
scattered gaps at that rate would leave no whole segment of 256 steps anywhere.

Runs per shape: float64 without and with gaps, q = 0 and q = 2.  On the device both numpy in -> numpy out (upload and download
included) and GPU tensor in -> GPU tensors out.  Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A):
`small`, 480 x 5 000, and `c2`, 2920 x 10 000.  The index: the first columns of a seeded AR(1) plane.

The driver starts FRESH processes that alternate between the legs - host, device, host, device, ... - so that both see the same
session.  A process makes one warm-up call per run and route and then --repeats timed calls.  The record keeps the seconds per call
over all timed calls of all processes (median [min, max]), the stage timers of one device call, and the largest difference of the two
legs' power and coherence on a probe of entries.

    python scripts/spectral_bench.py [--rounds 3] [--repeats 3] [--out profiles/spectral_bench.json]

`--trace-leg` runs one tensor-to-tensor float64 call at C2 (with gaps, q = 2) and nothing else, for a kernel trace of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAPS, L, STEP, MIN_SEGMENTS = 0.3, 256, 128, 2
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
STAGES = ("ingest_strided", "spectral_center", "spectral_index", "spectral_segments", "spectral_finish")
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def runs_of(shapes):
    """(shape name, T, N, gaps, q) of every run"""
    return [(name, T, N, gaps, q) for name, T, N in SHAPES if name in shapes for gaps in (False, True) for q in (0, 2)]


_FIELDS = {}


def field(T, N, gaps):
    key = (T, N)
    if key not in _FIELDS:
        sys.path.insert(0, os.path.join(HERE, "tests"))
        from golden_inputs import gen_A
        _FIELDS[key] = np.array(gen_A(T, N), dtype=np.float64)
    X = _FIELDS[key].copy()
    if gaps:
        run = int(round(GAPS * T))
        for n in range(N):
            start = (37 * n) % (T - run)
            X[start:start + run, n] = np.nan
    return X


def index(T, q):
    e = np.random.default_rng(1).standard_normal((T, 2))
    y = np.empty((T, 2))
    y[0] = e[0]
    for t in range(1, T):
        y[t] = 0.6 * y[t - 1] + 0.8 * e[t]
    return (y + 3.0)[:, :q] if q else None


def _ratios(pxx, pyy, pxy, kn, ke):
    """coherence, phase, gain and p from the averaged spectra"""
    with np.errstate(invalid="ignore", divide="ignore"):
        coh = np.clip(np.abs(pxy) ** 2 / (pxx[..., None] * pyy), 0, 1)
        p = np.exp((ke[kn][None, :, None] - 1) * np.log1p(-coh))
        return coh, np.angle(pxy), np.abs(pxy) / pyy, p


def host_route(X, y, gaps):
    """scipy.signal on the host threads: whole planes without gaps, the per-column masked loop with them"""
    import scipy.signal
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, HERE)
    from xmca_amd.spectral import effective_segments, welch_window
    T, N = X.shape
    q = 0 if y is None else y.shape[1]
    K = (T - L) // STEP + 1
    ke = effective_segments(np.arange(K + 1), welch_window("hann", L), STEP)
    F = L // 2 + 1
    yc = None if y is None else y - y.mean(axis=0)
    kw = dict(window="hann", nperseg=L, detrend="constant")
    if not gaps:
        pxx = scipy.signal.welch(X, noverlap=L - STEP, axis=0, **kw)[1]
        out = dict(power=pxx, segments=np.full(N, K, dtype=np.int32))
        if q:
            pyy = scipy.signal.welch(yc, noverlap=L - STEP, axis=0, **kw)[1]
            pxy = np.stack([scipy.signal.csd(yc[:, j][:, None], X, noverlap=L - STEP, axis=0, **kw)[1] for j in range(q)], axis=-1)
            pyy = np.broadcast_to(pyy[:, None, :], pxy.shape)
            coh, phase, gain, p = _ratios(pxx, pyy, pxy, out["segments"], ke)
            out.update(index_power=pyy, cospectrum=pxy.real, quadrature=pxy.imag, coherence=coh, phase=phase, gain=gain, p=p)
        return out
    missing = np.concatenate([np.zeros((1, N), dtype=np.int64), np.cumsum(np.isnan(X), axis=0)])
    starts = np.arange(K) * STEP
    whole = (missing[starts + L] - missing[starts]) == 0                       # (K, N): the present segments
    kn = whole.sum(axis=0).astype(np.int32)
    pxx = np.full((F, N), np.nan)
    pyy, pxy = np.full((F, N, q), np.nan), np.full((F, N, q), np.nan, dtype=complex)
    rows = starts[:, None] + np.arange(L)[None, :]

    def columns(lo, hi):
        for n in range(lo, hi):
            if kn[n] < MIN_SEGMENTS:
                continue
            at = rows[whole[:, n]].reshape(-1)
            xs = X[at, n]
            pxx[:, n] = scipy.signal.welch(xs, noverlap=0, **kw)[1]
            for j in range(q):
                ys = yc[at, j]
                pyy[:, n, j] = scipy.signal.welch(ys, noverlap=0, **kw)[1]
                pxy[:, n, j] = scipy.signal.csd(ys, xs, noverlap=0, **kw)[1]
    cuts = np.linspace(0, N, THREADS + 1).astype(int)
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(lambda i: columns(cuts[i], cuts[i + 1]), range(THREADS)))
    out = dict(power=pxx, segments=kn)
    if q:
        coh, phase, gain, p = _ratios(pxx, pyy, pxy, kn, ke)
        out.update(index_power=pyy, cospectrum=pxy.real, quadrature=pxy.imag, coherence=coh, phase=phase, gain=gain, p=p)
    return out


def _probe(F):
    flat = np.asarray(F).reshape(-1)
    return [float(v) for v in flat[flat.size // 3:: max(1, flat.size // 192)][:64]]


def leg(kind, repeats, shapes):
    """one process: every run; prints one JSON line"""
    sys.path.insert(0, HERE)
    out = []
    if kind == "device":
        import torch
        torch.cuda.init()                      # (torch's runtime first, then the library's)
        from xmca_amd import _hip
        from xmca_amd.spectral import spectral_maps
        dev = _hip.default_handle()
    for name, T, N, gaps, q in runs_of(shapes):
        X, y = field(T, N, gaps), index(T, q)
        entry = {"shape": name, "field": [T, N], "nperseg": L, "step": STEP, "bins": L // 2 + 1, "q": q, "dtype": "float64", "gaps": gaps}
        if kind == "host":
            def call():
                t0 = time.perf_counter()
                F = host_route(X, y, gaps)
                return time.perf_counter() - t0, F
            routes = {"scipy": call}
        else:
            Xt = torch.from_numpy(X).to(torch.device("cuda", dev.device))

            def call_numpy():
                t0 = time.perf_counter()
                F = spectral_maps(X, y, nperseg=L, step=STEP, min_segments=MIN_SEGMENTS, handle=dev)
                return time.perf_counter() - t0, F

            def call_tensor():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                F = spectral_maps(Xt, y, nperseg=L, step=STEP, min_segments=MIN_SEGMENTS, handle=dev)          # (returns with its stream drained)
                return time.perf_counter() - t0, F
            routes = {"numpy_to_numpy": call_numpy, "tensor_to_tensor": call_tensor}
        for route, call in routes.items():
            first = call()[0]
            calls = [call() for _ in range(repeats)]
            res = calls[-1][1]
            probes = {}
            for key in ("power",) + (("coherence",) if q else ()):
                v = res[key]
                probes[key] = _probe(v.cpu().numpy() if kind == "device" and route == "tensor_to_tensor" else v)
            seg = res["segments"]
            seg = seg.cpu().numpy() if kind == "device" and route == "tensor_to_tensor" else seg
            entry[route] = {"warmup_call_s": first, "s_per_call": [c[0] for c in calls], "probe": probes, "mean_segments": float(np.mean(seg))}
        if kind == "device":
            dev.reset_timings()
            call_tensor()
            entry["stages_ms_tensor_call"] = {k: v for k, v in dev.timings().items() if k in STAGES}
            del Xt
        out.append(entry)
    print("LEG " + json.dumps({"kind": kind, "cases": out}), flush=True)


def trace_leg():
    """one tensor-to-tensor call at C2 and nothing else: run under a kernel trace"""
    sys.path.insert(0, HERE)
    import torch
    torch.cuda.init()                          # (torch's runtime first, then the library's)
    from xmca_amd import _hip
    from xmca_amd.spectral import spectral_maps
    dev = _hip.default_handle()
    name, T, N = SHAPES[1]
    Xt = torch.from_numpy(field(T, N, True)).to(torch.device("cuda", dev.device))
    F = spectral_maps(Xt, index(T, 2), nperseg=L, step=STEP, min_segments=MIN_SEGMENTS, handle=dev)
    print("traced %s, nperseg %d, q = 2: %.2f segments per column" % (name, L, float(F["segments"].double().mean())), flush=True)


def _run_leg(label, kind, repeats, shapes):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repeats", str(repeats), "--shapes", ",".join(shapes)],
                       capture_output=True, text=True, timeout=1100)
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
    record = {"case": "spectral_maps(X, index, nperseg=%d), step %d, Hann, detrend='mean', all %d bins, min_segments = %d: float64 without gaps "
                      "and with %d %% of every column missing as one run, q = 0 and q = 2" % (L, STEP, L // 2 + 1, MIN_SEGMENTS, round(GAPS * 100)),
              "generator": "tests/golden_inputs.gen_A, one missing run per column at (37 n) mod the free length, index AR(1) from default_rng(1)",
              "processes_per_leg": rounds, "timed_calls_per_process": repeats, "order": "alternating fresh processes: host, device",
              "host_route": "scipy.signal.welch / csd on the host (%d threads): whole planes without gaps; with gaps the per-column masked loop - "
                            "the present segments of a column stacked into one series that scipy averages with noverlap = 0 - the columns shared "
                            "among the threads" % THREADS,
              "cases": [],
              "not_measured": ["float32 fields", "other nperseg, steps, windows and bin subsets at benchmark size", "q = 1, 3, 4 at benchmark size",
                               "scattered gaps at benchmark size", "the full-size C5 field", "more than one rank", "hardware counters"]}
    for i in range(len(legs["host"][0]["cases"])):
        h = [p["cases"][i] for p in legs["host"]]
        d = [p["cases"][i] for p in legs["device"]]
        entry = {k: h[0][k] for k in ("shape", "field", "nperseg", "step", "bins", "q", "dtype", "gaps")}
        entry["host_scipy"] = {"s_per_call": _stats([t for p in h for t in p["scipy"]["s_per_call"]]),
                               "warmup_call_s": [p["scipy"]["warmup_call_s"] for p in h], "mean_segments": h[-1]["scipy"]["mean_segments"]}
        for route in ("numpy_to_numpy", "tensor_to_tensor"):
            entry[route] = {"s_per_call": _stats([t for p in d for t in p[route]["s_per_call"]]),
                            "warmup_call_s": [p[route]["warmup_call_s"] for p in d], "mean_segments": d[-1][route]["mean_segments"]}
            for key, ref in h[-1]["scipy"]["probe"].items():
                ref, got = np.array(ref), np.array(d[-1][route]["probe"][key])
                both = np.isfinite(ref) & np.isfinite(got)
                entry[route]["probe_%s_nan_positions_as_host" % key] = bool(np.array_equal(np.isnan(ref), np.isnan(got)))
                entry[route]["probe_max_%s_diff_to_host_relative" % key] = float(np.max(np.abs(got[both] - ref[both])) / np.max(np.abs(ref[both]))) if both.any() else None
            entry[route]["speedup_median"] = entry["host_scipy"]["s_per_call"]["median"] / entry[route]["s_per_call"]["median"]
            entry[route]["max_below_host_min"] = entry[route]["s_per_call"]["max"] < entry["host_scipy"]["s_per_call"]["min"]
        entry["stages_ms_tensor_call"] = [p["stages_ms_tensor_call"] for p in d]
        record["cases"].append(entry)
    record["device_max_below_host_min_in_every_row"] = all(c[r]["max_below_host_min"] for c in record["cases"] for r in ("numpy_to_numpy", "tensor_to_tensor"))
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process, run and route")
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
