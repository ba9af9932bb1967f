#!/usr/bin/env python3
"""extended_eofs(12, 1, 10) of a real one-field float64 model (this revision) against the only route there was before it, run ON
THE PARENT COMMIT: numpy builds the embedded matrix Y = [X_0 | ... | X_11] on the host, then `MCA(Y).solve(n_modes=10)`,
`eofs(10)`, `pcs(10)` - the upload of Y included, the time numpy needs to build Y reported separately.  The new route is timed
from `MCA(X)` (the upload of X) to the numpy results of `extended_eofs`.

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A, float64): `small`, 480 x 5 000, and `c2`,
2920 x 10 000; M = 12, tau = 1.

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session.  A process makes one warm-up call per shape and then --repeats timed calls.  The record keeps, per shape and
leg, the seconds per call over all timed calls of all processes (median [min, max]), the stage timers of the new route
(`Handle.timings()` of one call), the same with the lag-sum kernel's LDS band switched off (XMCA_LAG_GRAM_BAND=0: plain row
reads), and the relative difference of the leading singular values of the two legs.

    python scripts/extended_eofs_bench.py --parent DIR [--rounds 3] [--repeats 3] [--out profiles/extended_eofs_bench.json]

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
K, M, TAU = 10, 12, 1
SHAPES = (("small", 480, 5000), ("c2", 2920, 10_000))


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


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
        Tp = T - (M - 1) * TAU

        def call():
            t0 = time.perf_counter()
            if kind == "extended":
                res = MCA(X).extended_eofs(M, TAU, K)
                return time.perf_counter() - t0, 0.0, res['singular_values']
            Y = np.concatenate([X[j * TAU:j * TAU + Tp] for j in range(M)], axis=1)
            t1 = time.perf_counter()
            m = MCA(Y)
            m.solve(n_modes=K)
            m.eofs(K)
            m.pcs(K)
            sv = m.singular_values(K)
            return time.perf_counter() - t0, t1 - t0, sv
        first = call()[0]
        calls = [call() for _ in range(repeats)]
        entry = {"shape": name, "field": [T, N], "warmup_call_s": first, "s_per_call": [c[0] for c in calls],
                 "build_Y_s": [c[1] for c in calls], "singular_values": [float(v) for v in calls[-1][2][:3]]}
        if kind == "extended":
            dev = _hip.default_handle()
            dev.reset_timings()
            call()
            entry["stages_ms"] = dev.timings()
        out.append(entry)
    print("LEG " + json.dumps({"repo": repo, "kind": kind, "band": os.environ.get("XMCA_LAG_GRAM_BAND", "1"), "shapes": out}), flush=True)


def trace_leg():
    """one call at C2 and nothing else: run under a kernel trace"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    from golden_inputs import gen_A
    from xmca_amd.array import MCA
    name, T, N = SHAPES[int(os.environ.get("TRACE_SHAPE", "1"))]
    res = MCA(gen_A(T, N)).extended_eofs(M, TAU, K)
    print("traced %s: leading singular value %.6e" % (name, res['singular_values'][0]), flush=True)


def _run_leg(label, repo, kind, repeats, shapes, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--repo", repo, "--repeats", str(repeats),
                        "--shapes", ",".join(shapes)], capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise SystemExit("the %s leg failed (exit %d):\n%s" % (label, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
    print("%s: %s" % (label, line[4:]), flush=True)
    return json.loads(line[4:])


def drive(parent, rounds, repeats, shapes):
    legs_spec = ([("embed_on_host_then_solve_on_parent", parent, "baseline")] if parent else []) + [("this_revision", HERE, "extended")]
    legs = {label: [] for label, _, _ in legs_spec}
    for rnd in range(rounds):
        for label, repo, kind in legs_spec:
            legs[label].append(_run_leg("round %d %s" % (rnd, label), repo, kind, repeats, shapes))
    no_band = _run_leg("plain row reads", HERE, "extended", 1, shapes, env=dict(os.environ, XMCA_LAG_GRAM_BAND="0"))
    record = {"case": "extended_eofs(%d, %d, %d), one real field" % (M, TAU, K), "dtype": "float64",
              "generator": "tests/golden_inputs.gen_A", "processes_per_leg": rounds, "timed_calls_per_process": repeats,
              "order": "alternating fresh processes: " + ", ".join(label for label, _, _ in legs_spec), "shapes": [],
              "not_measured": ["float32 fields at benchmark size", "the full-size C5 field", "more than one rank"]}
    for i, name in enumerate(n for n, *_ in SHAPES if n in shapes):
        entry = {}
        for label, _, _ in legs_spec:
            per = [p["shapes"][i] for p in legs[label]]
            entry.update({"shape": name, "field": per[0]["field"]})
            entry[label] = {"s_per_call": _stats([t for p in per for t in p["s_per_call"]]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per], "singular_values": per[-1]["singular_values"]}
            if label == "this_revision":
                entry[label]["stages_ms"] = [p["stages_ms"] for p in per]
                entry[label]["stages_ms_plain_row_reads"] = no_band["shapes"][i]["stages_ms"]
                T, Tp = per[0]["field"][0], per[0]["field"][0] - (M - 1) * TAU
                entry[label]["lag_gram_min_bytes"] = Tp * Tp * (M + 1) * 8
            else:
                entry[label]["build_Y_s"] = _stats([t for p in per for t in p["build_Y_s"]])
        if parent:
            a, b = entry["embed_on_host_then_solve_on_parent"], entry["this_revision"]
            entry.update({"speedup_median": a["s_per_call"]["median"] / b["s_per_call"]["median"],
                          "new_max_below_baseline_min": b["s_per_call"]["max"] < a["s_per_call"]["min"],
                          "singular_values_max_rel_diff": float(np.max(np.abs(np.array(a["singular_values"]) /
                                                                              np.array(b["singular_values"]) - 1)))})
        record["shapes"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process and shape")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["extended", "baseline"], help="(internal) measure one leg in this process")
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
