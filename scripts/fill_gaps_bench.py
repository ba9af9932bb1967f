#!/usr/bin/env python3
"""fill_gaps(X, 10, max_iter=20, tol=0) of a real float64 field with 30 % random gaps (this revision) against the only route there
was before it, run ON THE PARENT COMMIT: a host loop that, per iteration, uploads the current plane with `MCA(A)`, takes
`solve(n_modes=10)`, `eofs(10)`, `pcs(10)` and `singular_values(10)` back, forms the truncated reconstruction with numpy and
writes it into the gaps.  Both legs start from the field with NaN on the host and end with the filled field on the host; both
run 20 iterations, and the record reports seconds per iteration.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A, float64): `small`, 480 x 5 000, and `c2`,
2920 x 10 000.  The gaps are drawn with numpy.random.default_rng(0).

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session.  A process makes one warm-up call per shape and then --repeats timed calls.  The record keeps, per shape and
leg, the seconds per iteration over all timed calls of all processes (median [min, max]), the stage timers of the new route
(`Handle.timings()` of one call, summed over its 20 iterations), the share of the new kernels in them, and the RMS difference of
the filled values of the two legs relative to the RMS of the field (the host loop centres the plane again in every `MCA(A)`, the
device loop does not: the two are the same algorithm up to that).

    python scripts/fill_gaps_bench.py --parent DIR [--rounds 3] [--repeats 3] [--out profiles/fill_gaps_bench.json]

DIR: a checkout of the parent commit with its library built (`python -m xmca_amd.build` there).  Without --parent only this
revision is measured.  `--trace-leg` runs one C2 call of this revision and nothing else, for a kernel trace of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, ITERATIONS, GAPS = 10, 20, 0.3
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
STAGES = ("gap_center", "gram", "gap_eigh", "gap_project", "gap_fill", "gap_finish")       # (the handle also reports sub-timers of the eigensolver)


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def gappy_field(T, N):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from golden_inputs import gen_A
    X = np.array(gen_A(T, N), dtype=np.float64)
    X[np.random.default_rng(0).random((T, N)) < GAPS] = np.nan
    return X


def host_loop(MCA, X):
    """DINEOF over the public API as it stood: one model per iteration"""
    T = X.shape[0]
    present = np.isfinite(X)
    mean = np.nanmean(X, axis=0)
    A = np.where(present, X - mean, 0.0)
    for _ in range(ITERATIONS):
        m = MCA(A)                                  # centres the plane again and uploads it
        m.solve(n_modes=K)
        U, V = m.pcs(K)['left'], m.eofs(K)['left']
        s = np.sqrt(m.singular_values(K) * (T - 1))
        U = U / np.linalg.norm(U, axis=0)
        V = V / np.linalg.norm(V, axis=0)
        R = (U * s) @ V.T + A.mean(axis=0)
        A = np.where(present, A, R)
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
        gone = ~np.isfinite(X)

        def call():
            t0 = time.perf_counter()
            if kind == "device":
                F = fill_gaps(X, K, max_iter=ITERATIONS, tol=0.0)['field']
            else:
                F = host_loop(MCA, X)
            return time.perf_counter() - t0, F
        first = call()[0]
        calls = [call() for _ in range(repeats)]
        F = calls[-1][1]
        entry = {"shape": name, "field": [T, N], "warmup_call_s": first, "s_per_iteration": [c[0] / ITERATIONS for c in calls],
                 "filled_rms": float(np.sqrt(np.mean(F[gone] ** 2))), "field_rms": float(np.sqrt(np.nanmean(X ** 2))),
                 "filled_probe": [float(v) for v in F[gone][:: max(1, int(gone.sum()) // 64)][:64]]}
        if kind == "device":
            dev = _hip.default_handle()
            dev.reset_timings()
            call()
            entry["stages_ms"] = dev.timings()
        out.append(entry)
    print("LEG " + json.dumps({"repo": repo, "kind": kind, "shapes": out}), flush=True)


def trace_leg():
    """one call at C2 and nothing else: run under a kernel trace"""
    sys.path.insert(0, HERE)
    from xmca_amd.gaps import fill_gaps
    name, T, N = SHAPES[int(os.environ.get("TRACE_SHAPE", "1"))]
    res = fill_gaps(gappy_field(T, N), K, max_iter=ITERATIONS, tol=0.0)
    print("traced %s: last change %.6e" % (name, res['history'][-1]), flush=True)


def _run_leg(label, repo, kind, repeats, shapes):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repo", repo, "--repeats", str(repeats),
                        "--shapes", ",".join(shapes)], capture_output=True, text=True, timeout=900)
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
            legs[label].append(_run_leg("round %d %s" % (rnd, label), repo, kind, repeats, shapes))
    record = {"case": "fill_gaps(X, %d, max_iter=%d, tol=0), %d %% random gaps" % (K, ITERATIONS, round(GAPS * 100)), "dtype": "float64",
              "generator": "tests/golden_inputs.gen_A, gaps from default_rng(0)", "processes_per_leg": rounds,
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: " + ", ".join(label for label, _, _ in legs_spec),
              "shapes": [],
              "not_measured": ["float32 fields at benchmark size", "the full-size C5 field", "candidates of n_modes at benchmark size",
                               "more than one rank", "runs to convergence (both legs run 20 iterations)"]}
    for i, name in enumerate(n for n, *_ in SHAPES if n in shapes):
        entry = {}
        for label, _, _ in legs_spec:
            per = [p["shapes"][i] for p in legs[label]]
            entry.update({"shape": name, "field": per[0]["field"]})
            entry[label] = {"s_per_iteration": _stats([t for p in per for t in p["s_per_iteration"]]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per], "filled_rms": per[-1]["filled_rms"]}
            if label == "this_revision":
                entry[label]["stages_ms"] = [p["stages_ms"] for p in per]
                st = per[-1]["stages_ms"]
                new = sum(st.get(s, 0.0) for s in ("gap_center", "gap_fill", "gap_finish"))
                entry[label]["new_kernels_share_of_stage_time"] = new / sum(st.get(s, 0.0) for s in STAGES)
        if parent:
            a, b = entry["host_loop_on_parent"], entry["this_revision"]
            pa, pb = (np.array(legs[label][-1]["shapes"][i]["filled_probe"]) for label in ("host_loop_on_parent", "this_revision"))
            entry.update({"speedup_median": a["s_per_iteration"]["median"] / b["s_per_iteration"]["median"],
                          "new_max_below_baseline_min": b["s_per_iteration"]["max"] < a["s_per_iteration"]["min"],
                          "filled_probe_rms_diff_over_field_rms": float(np.sqrt(np.mean((pa - pb) ** 2)) /
                                                                        legs["this_revision"][-1]["shapes"][i]["field_rms"])})
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
    record = drive(args.parent, args.rounds, args.repeats, shapes)
    print(json.dumps(record)[:4000], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
