#!/usr/bin/env python3
"""bootstrap_eofs(n_runs, 10) of a real one-field float64 model: wall time per replicate on the device (this revision) against
the host loop over the public API that was the only way before it, run ON THE PARENT COMMIT - per replicate
`MCA(X[idx]).solve(n_modes=10)`, `eofs(10)`, alignment and accumulation of the deviations in numpy.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A: low-rank Gaussian signal + unit noise,
float64): `small`, 480 x 5 000, and `c2`, 2920 x 10 000 with few replicates per call.  Both legs use the same row indices
(`bootstrap_row_indices` of this revision, block_size 1, seed 5).

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session.  A process builds and solves the model, makes one warm-up call and then --repeats timed calls; a call returns
when mean and standard error are numpy arrays on the host.  The record keeps, per shape and leg, the seconds per replicate over
all timed calls of all processes (median [min, max]); for this revision also the seconds per replicate of `bootstrapping()`
(variances only, the same number of replicates) for scale, and the largest difference between the two legs' standard errors.

    python scripts/bootstrap_patterns_bench.py --parent DIR [--rounds 3] [--repeats 3] [--out profiles/bootstrap_patterns_bench.json]

DIR: a checkout of the parent commit with its library built (`python -m xmca_amd.build` there).  Without --parent only this
revision is measured.  `--trace-leg` runs one small call of this revision and nothing else, for a kernel trace of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10
SHAPES = (("small", 480, 5000, 16), ("c2", 2920, 10_000, 4))          # name, T, N, replicates per call


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def row_indices(n_runs, T):
    """the draw of `bootstrap_row_indices(n_runs, T, 1, seed=5)`, spelled out so that the parent checkout can make it too"""
    return np.random.default_rng(5).integers(0, T, (n_runs, T)).astype(np.int64)


def host_loop(MCA, X, idx, v0):
    """the definition of DESIGN.md 2.13 through the public API: one model per replicate"""
    R = len(idx)
    S, Q = np.zeros_like(v0), np.zeros_like(v0)
    for rows in idx:
        m = MCA(X[rows])
        m.solve(n_modes=K)
        v = m.eofs(K)['left']
        c = (v0 * v).sum(axis=0)
        d = np.where(c < 0, -1.0, 1.0) * v - v0
        S += d
        Q += d * d
    return v0 + S / R, np.sqrt(np.maximum(0.0, Q - S * S / R) / (R - 1))


def leg(repo, kind, repeats, shapes):
    """one process: every shape on the checkout `repo`; prints one JSON line"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, repo)
    from golden_inputs import gen_A
    from xmca_amd.array import MCA
    import xmca_amd
    assert os.path.dirname(os.path.abspath(xmca_amd.__file__)) == os.path.join(os.path.abspath(repo), "xmca_amd")
    out = []
    for name, T, N, runs in SHAPES:
        if name not in shapes:
            continue
        X = gen_A(T, N)
        idx = row_indices(runs, T)
        m = MCA(X)
        m.solve(n_modes=K)
        v0 = np.array(m.eofs(K)['left'])
        Xc = X - X.mean(axis=0)

        def call():
            t0 = time.perf_counter()
            if kind == "device":
                res = m.bootstrap_eofs(runs, K, indices=idx)
                mean, std = res['mean']['left'], res['std']['left']
            else:
                mean, std = host_loop(MCA, Xc, idx, v0)
            return time.perf_counter() - t0, mean, std
        first, mean, std = call()
        ts = [call()[0] / runs for _ in range(repeats)]
        entry = {"shape": name, "field": [T, N], "runs_per_call": runs, "warmup_call_s": first, "s_per_replicate": ts,
                 "std_sample": [float(v) for v in std[::max(N // 8, 1), 0]], "std_max_mode0": float(std[:, 0].max())}
        if kind == "device":
            tv = []
            for _ in range(repeats + 1):
                np.random.seed(5)
                t0 = time.perf_counter()
                m.bootstrapping(runs, n_modes=K, disable_progress=True)
                tv.append((time.perf_counter() - t0) / runs)
            entry["bootstrapping_values_only_s_per_replicate"] = tv[1:]
        out.append(entry)
        del m
    print("LEG " + json.dumps({"repo": repo, "kind": kind, "shapes": out}), flush=True)


def trace_leg():
    """one call at the small shape and nothing else: run under a kernel trace"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    from golden_inputs import gen_A
    from xmca_amd.array import MCA
    name, T, N, runs = SHAPES[int(os.environ.get("TRACE_SHAPE", "0"))]
    m = MCA(gen_A(T, N))
    m.solve(n_modes=K)
    res = m.bootstrap_eofs(runs, K, indices=row_indices(runs, T))
    print("traced %s: %d replicates, max std of mode 1 %.3e" % (name, runs, res['std']['left'][:, 0].max()), flush=True)


def drive(parent, rounds, repeats, shapes):
    legs_spec = ([("host_loop_on_parent", parent, "hostloop")] if parent else []) + [("this_revision", HERE, "device")]
    legs = {label: [] for label, _, _ in legs_spec}
    for rnd in range(rounds):
        for label, repo, kind in legs_spec:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repo", repo, "--repeats", str(repeats),
                                "--shapes", ",".join(shapes)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("the %s leg failed (exit %d):\n%s" % (label, r.returncode, r.stderr[-3000:]))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
            legs[label].append(json.loads(line[4:]))
            print("round %d %s: %s" % (rnd, label, line[4:]), flush=True)
    record = {"case": "bootstrap_eofs(n_runs, %d) after solve(n_modes=%d), one real field" % (K, K), "dtype": "float64",
              "generator": "tests/golden_inputs.gen_A", "processes_per_leg": rounds, "timed_calls_per_process": repeats,
              "order": "alternating fresh processes: " + ", ".join(label for label, _, _ in legs_spec), "shapes": [],
              "not_measured": ["float32 fields", "complex models at the size of C3", "two-field models at benchmark size",
                               "the full-size C5 field", "more than one rank", "block sizes other than 1"]}
    for i, name in enumerate(n for n, *_ in SHAPES if n in shapes):
        entry = {}
        for label, _, _ in legs_spec:
            per = [p["shapes"][i] for p in legs[label]]
            entry.update({"shape": name, "field": per[0]["field"], "runs_per_call": per[0]["runs_per_call"]})
            entry[label] = {"s_per_replicate": _stats([t for p in per for t in p["s_per_replicate"]]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per], "std_sample": per[-1]["std_sample"],
                            "std_max_mode0": per[-1]["std_max_mode0"]}
            if "bootstrapping_values_only_s_per_replicate" in per[0]:
                entry[label]["bootstrapping_values_only_s_per_replicate"] = _stats(
                    [t for p in per for t in p["bootstrapping_values_only_s_per_replicate"]])
        if parent:
            a, b = entry["host_loop_on_parent"], entry["this_revision"]
            pa, pb = a["s_per_replicate"], b["s_per_replicate"]
            spread = (pa["max"] - pa["min"]) + (pb["max"] - pb["min"])
            sa, sb = np.array(a["std_sample"]), np.array(b["std_sample"])
            entry.update({"speedup_median": pa["median"] / pb["median"], "spread_s": spread,
                          "separated": abs(pa["median"] - pb["median"]) > spread,
                          "max_std_sample_diff_over_max_std": float(np.max(np.abs(sa - sb)) / b["std_max_mode0"])})
        record["shapes"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process and shape")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["device", "hostloop"], help="(internal) measure one leg in this process")
    ap.add_argument("--trace-leg", action="store_true", help="one small call of this revision, for a kernel trace")
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
    print(json.dumps(record), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
