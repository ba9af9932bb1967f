#!/usr/bin/env python3
"""bootstrapping(n_runs, n_modes=10) of a one-field model solved with extend='theta', period=12: wall time per replicate of this
revision (replicates fitted and complexified on the device, xmca_bootstrap_runs_theta) against its parent commit (the
reference's host loop: per replicate a numpy resampling of the field, a fresh MCA - host centring, NaN scan, upload - the host
FFT of `theta_imag_parts` and one device solve).

Two shapes, both the generator of the C2 benchmark field (tests/golden_inputs.gen_A: low-rank Gaussian signal + unit noise,
float64): `small`, 480 x 5 000 (eigenproblems of 480), and `c2`, 2920 x 10 000 with few replicates per call.

The driver starts FRESH processes that alternate between the two checkouts - parent, this, parent, this, ... - so that both see
the same session (clocks, other tenants of the GPU).  A process builds the model, makes one warm-up call (workspaces, lanes, code
objects) and then --repeats timed calls of the shape's replicates under the same numpy seed; a call returns when the spectra are
on the host.  The record keeps, per shape and checkout, the seconds per replicate over all timed calls of all processes (median
[min, max]), the route the checkout took (the `resample` stage timer exists only on the device route) and the stage timers of
one timed call per replicate.  `slower_beyond_spread` says whether this revision's median exceeds the parent's by more than both
[min, max] spreads together.

    python scripts/bootstrap_theta_bench.py --parent DIR [--rounds 3] [--repeats 3] [--out profiles/bootstrap_theta_bench.json]

DIR: a checkout of the parent commit with its library built (`python -m xmca_amd.build` there).  Without --parent only this
revision is measured.  Nothing outside the two checkouts is read.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 12
SHAPES = (("small", 480, 5000, 16), ("c2", 2920, 10_000, 4))          # name, T, N, replicates per call


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def leg(repo, repeats, shapes):
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
        m = MCA(gen_A(T, N))
        t0 = time.perf_counter()
        m.solve(complexify=True, extend='theta', period=PERIOD)
        solve_s = time.perf_counter() - t0
        dev = m._device()

        def call(n):
            np.random.seed(5)
            t0 = time.perf_counter()
            spectra = m.bootstrapping(n, n_modes=10, disable_progress=True)
            return time.perf_counter() - t0, spectra
        dev.reset_timings()
        first, spectra = call(runs)
        route = "device" if "resample" in dev.timings() else "host loop"
        ts = []
        for _ in range(repeats):
            dev.reset_timings()
            ts.append(call(runs)[0] / runs)
        stages = {k: float(v) / runs for k, v in dev.timings().items()}           # (of the last timed call)
        out.append({"shape": name, "field": [T, N], "runs_per_call": runs, "route": route, "solve_s": solve_s, "warmup_call_s": first,
                    "s_per_replicate": ts, "stages_ms_per_replicate": stages, "spectrum_run0_first3": [float(v) for v in spectra[:3, 0]]})
        del m
    print("LEG " + json.dumps({"repo": repo, "shapes": out}), flush=True)


def drive(parent, rounds, repeats, shapes):
    checkouts = ([("parent", parent)] if parent else []) + [("this_revision", HERE)]
    legs = {label: [] for label, _ in checkouts}
    for rnd in range(rounds):
        for label, repo in checkouts:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--repo", repo, "--repeats", str(repeats),
                                "--shapes", ",".join(shapes)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("the %s leg failed (exit %d):\n%s" % (label, r.returncode, r.stderr[-3000:]))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1]
            legs[label].append(json.loads(line[4:]))
            print("round %d %s: %s" % (rnd, label, line[4:]), flush=True)
    record = {"case": "bootstrapping(n_runs, n_modes=10) after solve(complexify=True, extend='theta', period=%d), one field" % PERIOD,
              "dtype": "float64", "generator": "tests/golden_inputs.gen_A", "processes_per_checkout": rounds,
              "timed_calls_per_process": repeats, "order": "alternating fresh processes: " + ", ".join(label for label, _ in checkouts),
              "shapes": [],
              "not_measured": ["periods other than %d" % PERIOD, "the full-size C5 field", "more than one rank on hardware",
                               "rotated models"]}
    for i, name in enumerate(n for n, *_ in SHAPES if n in shapes):
        entry = {}
        for label, _ in checkouts:
            per = [p["shapes"][i] for p in legs[label]]
            entry.update({"shape": name, "field": per[0]["field"], "runs_per_call": per[0]["runs_per_call"]})
            entry[label] = {"route": per[0]["route"], "routes_agree": len({p["route"] for p in per}) == 1,
                            "s_per_replicate": _stats([t for p in per for t in p["s_per_replicate"]]),
                            "warmup_call_s": [p["warmup_call_s"] for p in per], "solve_s": [p["solve_s"] for p in per],
                            "stages_ms_per_replicate": per[-1]["stages_ms_per_replicate"],
                            "spectrum_run0_first3": per[-1]["spectrum_run0_first3"]}
        if parent:
            a, b = entry["parent"], entry["this_revision"]
            pa, pb = a["s_per_replicate"], b["s_per_replicate"]
            spread = (pa["max"] - pa["min"]) + (pb["max"] - pb["min"])
            sa, sb = np.array(a["spectrum_run0_first3"]), np.array(b["spectrum_run0_first3"])
            entry.update({"speedup_median": pa["median"] / pb["median"], "spread_s": spread,
                          "separated": abs(pa["median"] - pb["median"]) > spread,
                          "slower_beyond_spread": pb["median"] - pa["median"] > spread,
                          "max_rel_spectrum_diff": float(np.max(np.abs(sa - sb) / sa))})
        record["shapes"].append(entry)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="processes per checkout")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per process and shape")
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", action="store_true", help="(internal) measure one checkout in this process")
    ap.add_argument("--repo", default=HERE)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.leg:
        leg(args.repo, args.repeats, shapes)
        return
    record = drive(args.parent, args.rounds, args.repeats, shapes)
    print(json.dumps(record), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
