#!/usr/bin/env python3
"""lead_lag_maps(X, index, range(-24, 25)) with q = 2 index series against the fastest vectorised numpy route found on the host threads.

The host route forms every moment as a BLAS product: with X0 the zero-filled centred field, M its presence mask and, per (lag, series),
the shifted index plane Ylag[t, (l, j)] = y'[t - l, j] (zero outside the record) and the indicator I[t, l] of t - l lying inside it,
    Sxy = X0^T Ylag,  Sx = X0^T I,  Sxx = (X0^2)^T I,  Sy = M^T Ylag,  Syy = M^T Ylag^2,  n = M^T I
(without gaps the three M products are column sums of Ylag, Ylag^2 and I).  Then r, slope, the Bretherton factor from vectorised
lag-1 sums, and p by scipy.special.betainc.  A loop over the lags with one masked pass over T x N each was slower where it was tried,
at 480 x 5 000 on 16 host threads: 2.4 s (no gaps) / 3.3 s (gaps) for its moments alone against 0.3 - 0.5 s of the whole BLAS route
(the BLAS products use all host threads, the masked passes one).

Runs per shape: float64 without gaps and with 30 % random gaps (numpy.random.default_rng(0)), both dof modes; float32 once at C2 with
gaps and dof='n'.  On the device both numpy in -> numpy out (upload and download included) and GPU tensor in -> GPU tensors out.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A): `small`, 480 x 5 000, and `c2`, 2920 x 10 000.
The index: the first two columns of a seeded AR(1) plane.

The driver starts FRESH processes that alternate between the legs - host, device, host, device, ... - so that both see the same
session.  A process makes one warm-up call per run and route and then --repeats timed calls.  The record keeps the seconds per call
over all timed calls of all processes (median [min, max]), the stage timers of one device call, and the largest difference of the two
legs' r on a probe of entries.

    python scripts/lead_lag_bench.py [--rounds 3] [--repeats 3] [--out profiles/lead_lag_bench.json]

`--trace-leg` runs one tensor-to-tensor float64 call at C2 (with gaps, dof='bretherton') and nothing else, for a kernel trace of its
own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAPS, MIN_PAIRS, Q = 0.3, 8, 2
LAGS = list(range(-24, 25))
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
STAGES = ("ingest_strided", "lead_lag_center", "lead_lag_lag1", "lead_lag_moments", "lead_lag_finish")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def runs_of(shapes):
    """(shape name, T, N, dtype, gaps, dof) of every run"""
    out = []
    for name, T, N in SHAPES:
        if name not in shapes:
            continue
        for gaps in (False, True):
            for dof in ("n", "bretherton"):
                out.append((name, T, N, "float64", gaps, dof))
        if name == "c2":
            out.append((name, T, N, "float32", True, "n"))
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


def index(T):
    e = np.random.default_rng(1).standard_normal((T, Q))
    y = np.empty((T, Q))
    y[0] = e[0]
    for t in range(1, T):
        y[t] = 0.6 * y[t - 1] + 0.8 * e[t]
    return y + 3.0


def host_route(X, y, lags, min_pairs, dof, gaps):
    """the vectorised numpy route: the moments as BLAS products, p by scipy"""
    import scipy.special
    T, N = X.shape
    q, L = y.shape[1], len(lags)
    yc = y - y.mean(axis=0)
    present = ~np.isnan(X)
    n0 = present.sum(axis=0)
    X0 = np.where(present, X, 0).astype(np.float64)
    cn = X0.sum(axis=0) / np.maximum(n0, 1)
    X0 = np.where(present, X0 - cn, 0.0)
    Ylag = np.zeros((T, L, q))
    inside = np.zeros((T, L))
    for g, l in enumerate(lags):
        lo, hi = max(0, l), min(T, T + l)
        Ylag[lo:hi, g] = yc[lo - l:hi - l]
        inside[lo:hi, g] = 1.0
    Ylag = Ylag.reshape(T, L * q)
    first = X0.T @ np.concatenate([Ylag, inside], axis=1)
    sxy, sx = first[:, :L * q].reshape(N, L, q), first[:, L * q:]
    sxx = (X0 * X0).T @ inside
    if gaps:
        Mf = present.astype(np.float64)
        second = Mf.T @ np.concatenate([Ylag, Ylag * Ylag, inside], axis=1)
        sy, syy, n = second[:, :L * q].reshape(N, L, q), second[:, L * q:2 * L * q].reshape(N, L, q), second[:, 2 * L * q:]
    else:
        sy = np.broadcast_to(Ylag.sum(axis=0).reshape(1, L, q), (N, L, q))
        syy = np.broadcast_to((Ylag * Ylag).sum(axis=0).reshape(1, L, q), (N, L, q))
        n = np.broadcast_to(inside.sum(axis=0)[None, :], (N, L))
    with np.errstate(invalid="ignore", divide="ignore"):
        cxx = sxx - sx * sx / n
        cyy = syy - sy * sy / n[..., None]
        cxy = sxy - sx[..., None] * sy / n[..., None]
        live = (n >= min_pairs)[..., None] & (cxx > 2.0 ** -40 * sxx)[..., None] & (cyy > 2.0 ** -40 * syy)
        r = np.clip(cxy / np.sqrt(cxx[..., None] * cyy), -1, 1)
        slope = cxy / cyy
        d = np.broadcast_to(n[..., None], r.shape)
        if dof == "bretherton":
            both = present[1:] & present[:-1]
            npairs = both.sum(axis=0)
            rho_x = np.where(npairs > 0, ((X0[1:] * X0[:-1]).sum(axis=0) / np.maximum(npairs, 1)) / ((X0 * X0).sum(axis=0) / np.maximum(n0, 1)), 0.0)
            rho_x = np.clip(np.nan_to_num(rho_x), -1, 1)
            rho_y = np.clip(((yc[1:] * yc[:-1]).sum(axis=0) / (T - 1)) / ((yc * yc).sum(axis=0) / T), -1, 1)
            rho = rho_x[:, None, None] * rho_y[None, None, :]
            f = np.where(rho <= 0, 1.0, (1 - rho) / (1 + rho))
            d = np.minimum(d, np.floor(d * f))
        d = np.where(live, d, 0)
        r = np.where(live, r, np.nan).astype(X.dtype)
        a = d / 2 - 1
        p = np.where(live & (d >= 3), 2 * scipy.special.betainc(np.where(d >= 3, a, 1.0), np.where(d >= 3, a, 1.0),
                                                               np.clip((1 - np.abs(np.nan_to_num(r.astype(np.float64)))) / 2, 0, 1)), np.nan)
    order = (1, 0, 2)
    return dict(r=r.transpose(order), slope=np.where(live, slope, np.nan).astype(X.dtype).transpose(order), p=p.transpose(order),
                dof=d.astype(np.int32).transpose(order), pairs=n.astype(np.int32).T)


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
        from xmca_amd.lagged import lead_lag_maps
        dev = _hip.default_handle()
    for name, T, N, dtype, gaps, dof in runs_of(shapes):
        X, y = field(T, N, gaps, dtype), index(T)
        entry = {"shape": name, "field": [T, N], "lags": len(LAGS), "q": Q, "dtype": dtype, "gaps": gaps, "dof": dof}
        if kind == "host":
            def call():
                t0 = time.perf_counter()
                F = host_route(X, y, LAGS, MIN_PAIRS, dof, gaps)
                return time.perf_counter() - t0, F
            routes = {"numpy": call}
        else:
            Xt = torch.from_numpy(X).to(torch.device("cuda", dev.device))

            def call_numpy():
                t0 = time.perf_counter()
                F = lead_lag_maps(X, y, LAGS, min_pairs=MIN_PAIRS, dof=dof, handle=dev)
                return time.perf_counter() - t0, F

            def call_tensor():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                F = lead_lag_maps(Xt, y, LAGS, min_pairs=MIN_PAIRS, dof=dof, handle=dev)          # (the call returns with its stream drained)
                return time.perf_counter() - t0, F
            routes = {"numpy_to_numpy": call_numpy, "tensor_to_tensor": call_tensor}
        for route, call in routes.items():
            first = call()[0]
            calls = [call() for _ in range(repeats)]
            r = calls[-1][1]["r"]
            r = r.cpu().numpy() if kind == "device" and route == "tensor_to_tensor" else r
            entry[route] = {"warmup_call_s": first, "s_per_call": [c[0] for c in calls], "probe": _probe(r), "nan_fraction": float(np.isnan(r).mean())}
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
    from xmca_amd.lagged import lead_lag_maps
    dev = _hip.default_handle()
    name, T, N = SHAPES[1]
    Xt = torch.from_numpy(field(T, N, True, "float64")).to(torch.device("cuda", dev.device))
    F = lead_lag_maps(Xt, index(T), LAGS, min_pairs=MIN_PAIRS, dof="bretherton", handle=dev)
    print("traced %s, %d lags, q = %d: %.4f of the entries NaN" % (name, len(LAGS), Q, float(torch.isnan(F["r"]).double().mean())), flush=True)


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
    record = {"case": "lead_lag_maps(X, index, range(-24, 25)), q = %d, min_pairs = %d: without gaps and with %d %% gaps at random, dof 'n' and "
                      "'bretherton'" % (Q, MIN_PAIRS, round(GAPS * 100)),
              "generator": "tests/golden_inputs.gen_A, gaps from default_rng(0), index AR(1) from default_rng(1)", "processes_per_leg": rounds,
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: host, device",
              "host_route": "vectorised numpy on the host threads (OMP_NUM_THREADS=%s): the moments as BLAS products of the zero-filled "
                            "centred field, its square and its mask with the shifted index planes of all lags at once, p by "
                            "scipy.special.betainc; a loop of masked passes per lag was slower at 480 x 5 000 (2.4 - 3.3 s for its moments alone)" % os.environ.get("OMP_NUM_THREADS", "unset"),
              "cases": [],
              "not_measured": ["float32 fields other than C2 with gaps and dof='n'", "other q and other numbers of lags at benchmark size",
                               "the full-size C5 field", "more than one rank"]}
    for i in range(len(legs["host"][0]["cases"])):
        h = [p["cases"][i] for p in legs["host"]]
        d = [p["cases"][i] for p in legs["device"]]
        entry = {k: h[0][k] for k in ("shape", "field", "lags", "q", "dtype", "gaps", "dof")}
        entry["host_numpy"] = {"s_per_call": _stats([t for p in h for t in p["numpy"]["s_per_call"]]),
                               "warmup_call_s": [p["numpy"]["warmup_call_s"] for p in h]}
        ref = np.array(h[-1]["numpy"]["probe"])
        for route in ("numpy_to_numpy", "tensor_to_tensor"):
            got = np.array(d[-1][route]["probe"])
            both = np.isfinite(ref) & np.isfinite(got)
            entry[route] = {"s_per_call": _stats([t for p in d for t in p[route]["s_per_call"]]),
                            "warmup_call_s": [p[route]["warmup_call_s"] for p in d], "nan_fraction": d[-1][route]["nan_fraction"],
                            "probe_nan_positions_as_host": bool(np.array_equal(np.isnan(ref), np.isnan(got))),
                            "probe_max_r_diff_to_host": float(np.max(np.abs(got[both] - ref[both]))) if both.any() else None}
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
