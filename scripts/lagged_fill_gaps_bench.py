#!/usr/bin/env python3
"""fill_gaps(X, 10, max_iter=20, tol=0, embedding=12, tau=1) of a real float64 field with 30 % random gaps and 2 % wholly missing
time steps (this revision) against the only route there was before it, run ON THE PARENT COMMIT: a host loop that, per iteration,
takes `MCA(A).extended_reconstruct(12, 1, mode=slice(1, 10), original_scale=False)` and writes it into the gaps with numpy.  Both
legs start from the field with NaN on the host and end with the filled field on the host; both run 20 iterations, and the record
reports seconds per iteration.

The two legs are DIFFERENT algorithms: `MCA(A)` centres the columns of the plane again in every iteration and `extended_eofs`
centres every window, the device loop centres once and never again.  `--distance-leg` reports, on the small
shape after 5 iterations, how far each leg lies from its own numpy restatement and from the other (RMS over the filled entries
over the RMS of the field).

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A, float64): `small`, 480 x 5 000, and `c2`,
2920 x 10 000.  The gaps are drawn with numpy.random.default_rng(0).

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session.  A process makes one warm-up call per shape and then --repeats timed calls (3 processes x 3 calls: 9 per leg).

    python scripts/lagged_fill_gaps_bench.py --parent DIR [--rounds 3] [--repeats 3] [--out profiles/lagged_fill_gaps_bench.json]

DIR: a checkout of the parent commit with its library built (`python -m xmca_amd.build` there).  Without --parent only this
revision is measured.  `--trace-leg` runs one C2 call of this revision and one of fill_gaps without an embedding and nothing else,
for a kernel trace of its own.  `--kernel-leg` times the lagged fill kernel alone at C2 (`Handle.gap_lag_fill_step`, stage timer
"gap_fill"), for the register-tile heights of XMCA_GAP_LAG_ROWS.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, TAU, ITERATIONS, GAPS, DEAD = 10, 12, 1, 20, 0.3, 0.02
DISTANCE_ITERATIONS = 5
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
STAGES = ("gap_center", "gram", "gap_lag_gram", "gap_eigh", "gap_project", "gap_fill", "gap_finish")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def gappy_field(T, N):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from golden_inputs import gen_A
    X = np.array(gen_A(T, N), dtype=np.float64)
    rng = np.random.default_rng(0)
    X[rng.random((T, N)) < GAPS] = np.nan
    X[rng.choice(np.arange(2, T - 2), size=int(round(DEAD * T)), replace=False), :] = np.nan
    return X


def host_loop(MCA, X, iterations=ITERATIONS):
    """the iteration over the public API as it stood: one model per iteration, its reconstructed component into the gaps"""
    present = np.isfinite(X)
    mean = np.nanmean(X, axis=0)
    A = np.where(present, X - mean, 0.0)
    for _ in range(iterations):
        R = MCA(A).extended_reconstruct(M, TAU, mode=slice(1, K), original_scale=False)['left']
        A = np.where(present, A, R)
    return np.where(present, X, A + mean)


def host_loop_restated(X, iterations):
    """numpy float64 of `host_loop`: columns centred again, windows centred (the double centring of the lag-summed Gram matrix),
    the K leading modes, diagonal averaging"""
    present = np.isfinite(X)
    mean = np.nanmean(X, axis=0)
    A = np.where(present, X - mean, 0.0)
    T = X.shape[0]
    Tp = T - (M - 1) * TAU
    count = np.zeros(T)
    for j in range(M):
        count[j * TAU:j * TAU + Tp] += 1
    for _ in range(iterations):
        B = A - A.mean(axis=0)
        W = [B[j * TAU:j * TAU + Tp] - B[j * TAU:j * TAU + Tp].mean(axis=0) for j in range(M)]
        Kc = sum(w @ w.T for w in W)
        Z = np.linalg.eigh(Kc)[1][:, ::-1][:, :K].T
        R = np.zeros_like(A)
        for j, w in enumerate(W):
            R[j * TAU:j * TAU + Tp] += Z.T @ (Z @ w)
        A = np.where(present, A, R / count[:, None])
    return np.where(present, X, A + mean)


def leg(repo, kind, repeats, shapes):
    """one process: every shape on the checkout `repo`; prints one JSON line"""
    sys.path.insert(0, repo)
    from xmca_amd import _hip
    from xmca_amd.array import MCA
    import xmca_amd
    assert os.path.dirname(os.path.abspath(xmca_amd.__file__)) == os.path.join(os.path.abspath(repo), "xmca_amd")
    if kind == "device":
        from xmca_amd.gaps import fill_gaps
    out = []
    for name, T, N in SHAPES:
        if name not in shapes:
            continue
        X = gappy_field(T, N)

        def call():
            t0 = time.perf_counter()
            if kind == "device":
                fill_gaps(X, K, max_iter=ITERATIONS, tol=0.0, embedding=M, tau=TAU)
            else:
                host_loop(MCA, X)
            return time.perf_counter() - t0
        first = call()
        entry = {"shape": name, "field": [T, N], "warmup_call_s": first, "s_per_iteration": [call() / ITERATIONS for _ in range(repeats)]}
        if kind == "device":
            dev = _hip.default_handle()
            dev.reset_timings()
            call()
            entry["stages_ms"] = dev.timings()
        out.append(entry)
    print("LEG " + json.dumps({"repo": repo, "kind": kind, "shapes": out}), flush=True)


def distance_leg():
    """both legs and their numpy restatements on the small shape, DISTANCE_ITERATIONS iterations; prints one JSON line"""
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from xmca_amd.array import MCA
    from xmca_amd.gaps import fill_gaps
    import lagged_fill_gaps_cases as C
    name, T, N = SHAPES[0]
    X = gappy_field(T, N)
    gone = ~np.isfinite(X)
    rms = float(np.sqrt(np.nanmean(X ** 2)))
    its = DISTANCE_ITERATIONS
    fields = {"device": fill_gaps(X, K, max_iter=its, tol=0.0, embedding=M, tau=TAU)['field'],
              "device_restated": C.mssa_fill(X, K, M, TAU, its, 0.0)['field'],
              "host_loop": host_loop(MCA, X, its), "host_loop_restated": host_loop_restated(X, its)}

    def dist(a, b):
        return float(np.sqrt(np.mean((fields[a][gone] - fields[b][gone]) ** 2)) / rms)
    print("LEG " + json.dumps({"shape": name, "iterations": its, "what": "RMS difference over the filled entries / RMS of the field",
                               "device_vs_its_restatement": dist("device", "device_restated"),
                               "host_loop_vs_its_restatement": dist("host_loop", "host_loop_restated"),
                               "device_vs_host_loop": dist("device", "host_loop")}), flush=True)


def trace_leg():
    """one lagged call at C2, one call without an embedding, and nothing else: run under a kernel trace"""
    sys.path.insert(0, HERE)
    from xmca_amd.gaps import fill_gaps
    name, T, N = SHAPES[int(os.environ.get("TRACE_SHAPE", "1"))]
    X = gappy_field(T, N)
    res = fill_gaps(X, K, max_iter=ITERATIONS, tol=0.0, embedding=M, tau=TAU)
    one = fill_gaps(X, K, max_iter=ITERATIONS, tol=0.0)
    print("traced %s: last change %.6e (embedding %d), %.6e (one window)" % (name, res['history'][-1], M, one['history'][-1]), flush=True)


def kernel_leg():
    """the lagged fill kernel alone at C2: median of 7 launches of `gap_lag_fill_step` by the stage timer; prints one JSON line"""
    sys.path.insert(0, HERE)
    from xmca_amd import _hip
    name, T, N = SHAPES[1]
    rng = np.random.default_rng(0)
    A = rng.standard_normal((T, N))
    mask = np.isnan(gappy_field(T, N)).astype(np.uint8)
    Z = rng.standard_normal((K, T - (M - 1) * TAU))
    P = rng.standard_normal((M * K, N))
    dev = _hip.default_handle()
    ms = []
    for i in range(8):
        dev.reset_timings()
        dev.gap_lag_fill_step(A, mask, Z, P, M, TAU)
        ms.append(dev.timings()["gap_fill"])
    print("LEG " + json.dumps({"rows": os.environ.get("XMCA_GAP_LAG_ROWS", "default"), "shape": name, "masked_share": float(mask.mean()),
                               "gap_fill_ms_first": ms[0], "gap_fill_ms": _stats(ms[1:])}), flush=True)


def _run_leg(label, args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit("the %s leg failed (exit %d):\n%s" % (label, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
    print("%s: %s" % (label, line[4:1500]), flush=True)
    return json.loads(line[4:])


def drive(parent, rounds, repeats, shapes):
    legs_spec = ([("host_loop_on_parent", parent, "host")] if parent else []) + [("this_revision", HERE, "device")]
    legs = {label: [] for label, _, _ in legs_spec}
    for rnd in range(rounds):
        for label, repo, kind in legs_spec:
            legs[label].append(_run_leg("round %d %s" % (rnd, label), ["--leg", kind, "--repo", repo, "--repeats", str(repeats),
                                                                       "--shapes", ",".join(shapes)]))
    record = {"case": "fill_gaps(X, %d, max_iter=%d, tol=0, embedding=%d, tau=%d), %d %% random gaps and %d %% wholly missing time steps"
                      % (K, ITERATIONS, M, TAU, round(GAPS * 100), round(DEAD * 100)), "dtype": "float64",
              "baseline": "per iteration MCA(A).extended_reconstruct(%d, %d, mode=slice(1, %d), original_scale=False) on the parent "
                          "commit, then the fill in numpy: another algorithm (columns and windows centred again)" % (M, TAU, K),
              "generator": "tests/golden_inputs.gen_A, gaps from default_rng(0)", "processes_per_leg": rounds,
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: " + ", ".join(label for label, _, _ in legs_spec),
              "shapes": [], "distances": _run_leg("distances", ["--distance-leg"]),
              "fill_kernel_at_c2_by_register_tile": [_run_leg("kernel rows %s" % r, ["--kernel-leg"], {"XMCA_GAP_LAG_ROWS": r})
                                                     for r in ("16", "32", "64")],
              "not_measured": ["float32 fields at benchmark size", "the full-size C5 field", "candidates of n_modes at benchmark size",
                               "runs to convergence (both legs run 20 iterations)", "the distances at C2 (small shape only)",
                               "more than one rank"]}
    for i, name in enumerate(n for n, *_ in SHAPES if n in shapes):
        entry = {}
        for label, _, _ in legs_spec:
            per = [p["shapes"][i] for p in legs[label]]
            entry.update({"shape": name, "field": per[0]["field"]})
            entry[label] = {"s_per_iteration": _stats([t for p in per for t in p["s_per_iteration"]]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per]}
            if label == "this_revision":
                entry[label]["stages_ms_of_one_call"] = {s: per[-1]["stages_ms"].get(s) for s in STAGES}
        if parent:
            a, b = entry["host_loop_on_parent"], entry["this_revision"]
            entry.update({"ratio_of_medians": a["s_per_iteration"]["median"] / b["s_per_iteration"]["median"],
                          "new_max_below_baseline_min": b["s_per_iteration"]["max"] < a["s_per_iteration"]["min"]})
        record["shapes"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process and shape")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["device", "host"], help="(internal) measure one leg in this process")
    ap.add_argument("--distance-leg", action="store_true", help="(internal) both legs against their numpy restatements")
    ap.add_argument("--kernel-leg", action="store_true", help="the lagged fill kernel alone at C2")
    ap.add_argument("--trace-leg", action="store_true", help="one C2 call of this revision, for a kernel trace")
    ap.add_argument("--repo", default=HERE)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.trace_leg:
        trace_leg()
    elif args.kernel_leg:
        kernel_leg()
    elif args.distance_leg:
        distance_leg()
    elif args.leg:
        leg(args.repo, args.leg, args.repeats, shapes)
    else:
        record = drive(args.parent, args.rounds, args.repeats, shapes)
        print(json.dumps(record)[:4000], flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
