#!/usr/bin/env python3
"""extended_reconstruct(12, 1, mode) of a real one-field float64 model (this revision) against the only route there was before
it, run ON THE PARENT COMMIT: `extended_eofs(12, n_modes=10)` on the device, then numpy on the host - one outer product
(T' x q)(q x N) per lag from the PCs and the lag patterns, the diagonal averaging, the window means of the centred field and the
field's mean.  Both legs are timed from `MCA(X)` (the upload of X) to the finished T x N float64 result: a numpy array, or with
--output torch a tensor on the GPU (the baseline uploads its host result; the new route writes it there).

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A, float64): `small`, 480 x 5 000, and `c2`,
2920 x 10 000; M = 12, tau = 1; the mode groups 1-10 and the pair 1-2.

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session.  A process makes one warm-up call per shape, group and output and then --repeats timed calls.  The record keeps
the seconds per call over all timed calls of all processes (median [min, max]), the stage timers of the new route
(`Handle.timings()` of one call) and the largest difference of the two legs' results over max|X|.

    python scripts/extended_reconstruct_bench.py --parent DIR [--rounds 3] [--repeats 3] [--out profiles/extended_reconstruct_bench.json]

DIR: a checkout of the parent commit with its library built (`python -m xmca_amd.build` there).  Without --parent only this
revision is measured.  `--trace-leg` runs one C2 call (modes 1-10, numpy) of this revision and nothing else, for a kernel trace
of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, TAU = 10, 12, 1
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))
GROUPS = (("modes_1_10", 10), ("pair_1_2", slice(1, 2)))
OUTPUTS = ("numpy", "torch")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def host_route(model, X, mode, output):
    """what a user of the parent commit does: patterns and PCs from the device, the rest in numpy"""
    T, N = X.shape
    Tp = T - (M - 1) * TAU
    res = model.extended_eofs(M, TAU, K)
    sel = slice(0, mode) if isinstance(mode, int) else slice(mode.start - 1, mode.stop)
    coeff = res['pcs'][:, sel] * np.sqrt(res['singular_values'][sel])           # s_k u_k
    eofs = res['eofs']['left']
    mean = X.mean(axis=0)
    Xc = X - mean
    R = np.zeros((T, N))
    m = np.zeros((T, N))
    count = np.zeros(T)
    for j in range(M):
        rows = slice(j * TAU, j * TAU + Tp)
        R[rows] += coeff @ eofs[j][:, sel].T
        m[rows] += Xc[rows].mean(axis=0)
        count[rows] += 1
    R += m
    R /= count[:, None]
    R += mean
    if output == "torch":
        import torch
        R = torch.from_numpy(R).to("cuda:0")
        torch.cuda.synchronize()
    return R


def leg(repo, kind, repeats, shapes):
    """one process: every shape, group and output on the checkout `repo`; prints one JSON line"""
    import torch                                     # (before the first device call)
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
        for group, mode in GROUPS:
            for output in OUTPUTS:
                def call():
                    t0 = time.perf_counter()
                    if kind == "reconstruct":
                        R = MCA(X, output=output).extended_reconstruct(M, TAU, mode)['left']
                    else:
                        R = host_route(MCA(X), X, mode, output)
                    return time.perf_counter() - t0, R
                first = call()[0]
                calls = [call() for _ in range(repeats)]
                R = calls[-1][1]
                R = R.cpu().numpy() if output == "torch" else R
                probe = R[:: max(1, T // 7), :: max(1, N // 11)]
                entry = {"shape": name, "field": [T, N], "group": group, "output": output, "warmup_call_s": first,
                         "s_per_call": [c[0] for c in calls], "probe": [float(v) for v in probe.reshape(-1)],
                         "max_abs_field": float(np.abs(X).max())}
                if kind == "reconstruct":
                    dev = _hip.default_handle()
                    dev.reset_timings()
                    call()
                    entry["stages_ms"] = dev.timings()
                out.append(entry)
    print("LEG " + json.dumps({"repo": repo, "kind": kind, "entries": out}), flush=True)


def trace_leg():
    """one call at C2 and nothing else: run under a kernel trace"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    from golden_inputs import gen_A
    from xmca_amd.array import MCA
    name, T, N = SHAPES[int(os.environ.get("TRACE_SHAPE", "1"))]
    R = MCA(gen_A(T, N)).extended_reconstruct(M, TAU, K)['left']
    print("traced %s: R[0, 0] = %.6e" % (name, R[0, 0]), flush=True)


def _run_leg(label, repo, kind, repeats, shapes):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repo", repo, "--repeats", str(repeats),
                        "--shapes", ",".join(shapes)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("the %s leg failed (exit %d):\n%s" % (label, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
    print("%s: done" % label, flush=True)
    return json.loads(line[4:])


def drive(parent, rounds, repeats, shapes):
    legs_spec = ([("extended_eofs_then_numpy_on_parent", parent, "baseline")] if parent else []) + [("this_revision", HERE, "reconstruct")]
    legs = {label: [] for label, _, _ in legs_spec}
    for rnd in range(rounds):
        for label, repo, kind in legs_spec:
            legs[label].append(_run_leg("round %d %s" % (rnd, label), repo, kind, repeats, shapes))
    record = {"case": "extended_reconstruct(%d, %d, mode), one real field, original_scale=True" % (M, TAU), "dtype": "float64",
              "generator": "tests/golden_inputs.gen_A", "processes_per_leg": rounds, "timed_calls_per_process": repeats,
              "order": "alternating fresh processes: " + ", ".join(label for label, _, _ in legs_spec), "cases": [],
              "not_measured": ["float32 fields at benchmark size", "the full-size C5 field", "more than one rank"]}
    n_entries = len(legs["this_revision"][0]["entries"])
    for i in range(n_entries):
        entry = {}
        for label, _, _ in legs_spec:
            per = [p["entries"][i] for p in legs[label]]
            entry.update({k: per[0][k] for k in ("shape", "field", "group", "output")})
            entry[label] = {"s_per_call": _stats([t for p in per for t in p["s_per_call"]]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per]}
            if label == "this_revision":
                entry[label]["stages_ms"] = [p["stages_ms"] for p in per]
        if parent:
            a, b = entry["extended_eofs_then_numpy_on_parent"], entry["this_revision"]
            pa = np.array(legs["extended_eofs_then_numpy_on_parent"][-1]["entries"][i]["probe"])
            pb = np.array(legs["this_revision"][-1]["entries"][i]["probe"])
            entry.update({"speedup_median": a["s_per_call"]["median"] / b["s_per_call"]["median"],
                          "new_max_below_baseline_min": b["s_per_call"]["max"] < a["s_per_call"]["min"],
                          "max_abs_diff_over_max_abs_field": float(np.max(np.abs(pa - pb)) /
                                                                   legs["this_revision"][-1]["entries"][i]["max_abs_field"])})
        record["cases"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process, shape, group and output")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["reconstruct", "baseline"], help="(internal) measure one leg in this process")
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
    print(json.dumps(record), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
