#!/usr/bin/env python3
"""extended_rule_n(12, 1, n_runs=100, n_modes=10) of a real one-field float64 model (this revision) against the only route there
was before it, run ON THE PARENT COMMIT: `extended_eofs(12, 1, 10)` on the device, then on the host, per run, a numpy AR(1)
surrogate (numpy's generator, the recurrence as a loop over the time steps, vectorised over the columns), the M thin numpy
products R_j (diag(d) V_j), the centring and the norms; phi and d come from numpy once per call.  Both legs are timed from `MCA(X)`
(the upload of X) to the numpy results.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A, float64): `small`, 480 x 5 000, and `c2`,
2920 x 10 000; M = 12, tau = 1.

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session.  A process makes one warm-up call per shape (the baseline's with 2 runs: it warms the same code) and then
--repeats timed calls.  Every process leaves its record in --legs-dir; the driver's record is built from ALL records found there,
so that the rounds of a measurement may be separate invocations.  The record keeps, per shape and leg, the seconds per call over
all timed calls of all processes (median [min, max]), the same per surrogate, and the stage timers of the new route
(`Handle.timings()` of one call) as front / surrogate generation / GEMM / projection.

    python scripts/extended_rule_n_bench.py --parent DIR --legs-dir DIR2 [--rounds 3] [--repeats 3]
                                            [--out profiles/extended_rule_n_bench.json]

DIR: a checkout of the parent commit with its library built (`python -m xmca_amd.build` there).  Without --parent only this
revision is measured.  `--trace-leg` runs one C2 call of this revision and nothing else, for a kernel trace of its own.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, TAU, RUNS = 10, 12, 1, 100
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
FRONT = ("gram", "lag_gram", "eeof_eigh", "eeof_project", "mcssa_scale")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def host_route(MCA, X, n_runs, rng):
    """the baseline: extended EOFs on the device of the parent commit, everything of the test on the host"""
    T, N = X.shape
    Tp = T - (M - 1) * TAU
    res = MCA(X).extended_eofs(M, TAU, K)
    V = res['eofs']['left']                                   # (M, N, K)
    Xc = X - X.mean(axis=0)
    d = Xc.std(axis=0, ddof=1)
    phi = np.sum(Xc[:-1] * Xc[1:], axis=0) / np.sum(Xc * Xc, axis=0)
    B = V * d[None, :, None]
    a = np.sqrt((1.0 - phi) * (1.0 + phi))
    out = np.empty((n_runs, K))
    for r in range(n_runs):
        R = rng.standard_normal((T, N))
        for t in range(1, T):
            R[t] = phi * R[t - 1] + a * R[t]
        Q = R[:Tp] @ B[0]
        for j in range(1, M):
            Q += R[j * TAU:j * TAU + Tp] @ B[j]
        Q -= Q.mean(axis=0)
        out[r] = np.sum(Q * Q, axis=0)
    return res['singular_values'], out.T / (Tp - 1)


def leg(repo, kind, repeats, shapes):
    """one process: every shape on the checkout `repo`; prints one JSON line"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, repo)
    from golden_inputs import gen_A
    from xmca_amd import _hip
    from xmca_amd.array import MCA
    import xmca_amd
    assert os.path.dirname(os.path.abspath(xmca_amd.__file__)) == os.path.join(os.path.abspath(repo), "xmca_amd")
    out = []
    for name, T, N in SHAPES:
        if name not in shapes:
            continue
        X = gen_A(T, N)
        rng = np.random.default_rng(1)

        def call(n_runs=RUNS):
            t0 = time.perf_counter()
            if kind == "device":
                res = MCA(X).extended_rule_n(M, TAU, n_runs=n_runs, n_modes=K, seed=1)
                sv, null = res['singular_values'], res['surrogates']
            else:
                sv, null = host_route(MCA, X, n_runs, rng)
            print("  %s %s: a call of %d runs took %.3f s" % (kind, name, n_runs, time.perf_counter() - t0), file=sys.stderr, flush=True)
            return time.perf_counter() - t0, sv, null
        first = call(RUNS if kind == "device" else 2)[0]
        calls = [call() for _ in range(repeats)]
        entry = {"shape": name, "field": [T, N], "warmup_call_s": first, "s_per_call": [c[0] for c in calls],
                 "singular_values": [float(v) for v in calls[-1][1][:3]],
                 "null_median_over_singular_value": [float(v) for v in np.median(calls[-1][2], axis=1) / calls[-1][1]]}
        if kind == "device":
            dev = _hip.default_handle()
            dev.reset_timings()
            call()
            entry["stages_ms"] = dev.timings()
        out.append(entry)
    print("LEG " + json.dumps({"repo": repo, "kind": kind, "shapes": out}), flush=True)


def trace_leg():
    """one call at C2 and nothing else: run under a kernel trace"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    from golden_inputs import gen_A
    from xmca_amd.array import MCA
    name, T, N = SHAPES[int(os.environ.get("TRACE_SHAPE", "1"))]
    res = MCA(gen_A(T, N)).extended_rule_n(M, TAU, n_runs=RUNS, n_modes=K, seed=1)
    print("traced %s: exceedance %s" % (name, res['exceedance']), flush=True)


def _run_leg(label, repo, kind, repeats, shapes, legs_dir):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repo", repo, "--repeats", str(repeats),
                        "--shapes", ",".join(shapes)], stdout=subprocess.PIPE, text=True, timeout=1100)      # (stderr: progress, passed on)
    if r.returncode != 0:
        raise SystemExit("the %s leg failed (exit %d)" % (label, r.returncode))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
    print("%s: %s" % (label, line[4:]), flush=True)
    n = len(glob.glob(os.path.join(legs_dir, "leg_*.json")))
    with open(os.path.join(legs_dir, "leg_%03d_%s.json" % (n, kind)), "w") as fh:
        fh.write(line[4:] + "\n")


def _split(stages, n_runs):
    front = sum(stages.get(k, 0.0) for k in FRONT)
    return {"front_ms": front, "surrogate_ms": stages.get("mcssa_surrogate", 0.0), "gemm_ms": stages.get("mcssa_gemm", 0.0),
            "projection_ms": stages.get("mcssa_project", 0.0),
            "per_surrogate_ms": (stages.get("mcssa_surrogate", 0.0) + stages.get("mcssa_gemm", 0.0) + stages.get("mcssa_project", 0.0)) / n_runs}


def drive(parent, rounds, repeats, shapes, legs_dir):
    os.makedirs(legs_dir, exist_ok=True)
    labels = {"host": "extended_eofs_on_parent_then_numpy", "device": "this_revision"}
    for rnd in range(rounds):
        for kind, repo in ([("host", parent)] if parent else []) + [("device", HERE)]:
            _run_leg("round %d %s" % (rnd, labels[kind]), repo, kind, repeats, shapes, legs_dir)
    legs = {"host": [], "device": []}
    for path in sorted(glob.glob(os.path.join(legs_dir, "leg_*.json"))):
        rec = json.load(open(path))
        legs[rec["kind"]].append(rec)
    record = {"case": "extended_rule_n(%d, %d, n_runs=%d, n_modes=%d), one real field" % (M, TAU, RUNS, K), "dtype": "float64",
              "generator": "tests/golden_inputs.gen_A", "processes_per_leg": {labels[k]: len(v) for k, v in legs.items()},
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: baseline, this revision, ...", "shapes": [],
              "not_measured": ["float32 fields at benchmark size", "the full-size C5 field", "more than one rank"]}
    for name, T, N in SHAPES:
        entry = {"shape": name, "field": [T, N]}
        for kind, label in labels.items():
            per = [s for p in legs[kind] for s in p["shapes"] if s["shape"] == name]
            if not per:
                continue
            calls = [t for p in per for t in p["s_per_call"]]
            entry[label] = {"s_per_call": _stats(calls), "s_per_surrogate": _stats([t / RUNS for t in calls]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per], "singular_values": per[-1]["singular_values"],
                            "null_median_over_singular_value": per[-1]["null_median_over_singular_value"]}
            if kind == "device":
                entry[label]["stages_ms"] = [p["stages_ms"] for p in per]
                entry[label]["stage_split_of_one_call"] = _split(per[-1]["stages_ms"], RUNS)
        if len(entry) > 2:
            record["shapes"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg started by this invocation")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process and shape")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--legs-dir", default="out/extended_rule_n_legs", help="where the processes' records are kept and read from")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["device", "host"], help="(internal) measure one leg in this process")
    ap.add_argument("--trace-leg", action="store_true", help="one C2 call of this revision, for a kernel trace")
    ap.add_argument("--repo", default=HERE)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.trace_leg:
        trace_leg()
        return
    if args.leg:
        leg(args.repo, args.leg, args.repeats, shapes)
        return
    record = drive(args.parent, args.rounds, args.repeats, shapes, args.legs_dir)
    print(json.dumps(record), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
