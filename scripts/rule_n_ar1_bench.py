#!/usr/bin/env python3
"""Throughput of rule_n with white and with red-noise (AR(1)) surrogates on one GPU, and the kernel times of the new passes.

    python scripts/rule_n_ar1_bench.py --out profiles/rule_n_ar1_bench.json [--repeats 3] [--parent-tree DIR]
        surrogates/s of `Handle.rule_n` at C4 (5000 x (20 000, 15 000), complex) and the C2-shaped EOF (2920 x 10 000), white and
        ar1, each measurement in a fresh process, white and ar1 alternating; median [min, max] over the repeats.  --parent-tree: a
        built checkout of the parent commit whose white path is measured in the same alternation.
    python scripts/rule_n_ar1_bench.py --trace-workload {c4,c2_eof,estimator}
        the work a kernel trace looks at (run it under `rocprofv3 --kernel-trace --stats -- python ...`, a run of its own): two red
        runs of the case, or the estimator beside the column sums of the same field at C2 and at c5_scaled (1200 x 41 472, float32).
    python scripts/rule_n_ar1_bench.py --kernel-stats STATS.csv --label {c4,c2_eof,estimator} --out profiles/rule_n_ar1_bench.json
        adds the kernel times of that trace, and the bytes/s they amount to, to the profile.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: T, Nx, Ny, fields, complexify, runs in the timed window
CASES = {"c4": (5000, 20000, 15000, 2, True, 12), "c2_eof": (2920, 10000, 0, 1, False, 24)}


def _phi(n, seed):
    return np.random.default_rng(seed).uniform(0.3, 0.9, n)


def child(case, noise, tree):
    sys.path.insert(0, tree)
    from xmca_amd import _hip
    T, Nx, Ny, nf, cplx, runs = CASES[case]
    h = _hip.Handle(0)
    kw = {}
    if noise == "ar1":
        kw["ar1"] = (_phi(Nx, 1), _phi(Ny, 2) if nf == 2 else None)
    n_out = min(T, Nx if nf == 1 else min(Nx, Ny))
    args = (T, Nx, Ny, nf, cplx, False, 0, 1, 1e-8)
    h.rule_n(*args, 0, 4, 1, np.float64, n_out, **kw)             # warm-up (every lane)
    t0 = time.perf_counter()
    sp, kept = h.rule_n(*args, 0, runs, 1, np.float64, n_out, **kw)      # (returns after the lanes have synchronised)
    dt = time.perf_counter() - t0
    print(json.dumps({"case": case, "noise": noise, "runs": runs, "surrogates_per_s": runs / dt, "kept": int(kept.sum()),
                      "sigma_head": [float(x) for x in sp[0][:3]]}))


def _summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def throughput(out, repeats, parent_tree):
    variants = [("white", "white", REPO), ("ar1", "ar1", REPO)]
    if parent_tree:
        variants.insert(0, ("white_parent", "white", os.path.abspath(parent_tree)))
    got = {case: {name: [] for name, _, _ in variants} for case in CASES}
    heads = {}
    for _ in range(repeats):
        for case in CASES:
            for name, noise, tree in variants:                     # alternating: parent, this tree white, this tree ar1
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, noise, "--tree", tree], capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit("measurement %s / %s failed:\n%s" % (case, name, r.stderr[-2000:]))
                rec = json.loads(r.stdout.splitlines()[-1])
                got[case][name].append(rec["surrogates_per_s"])
                heads.setdefault(case, {})[name] = rec["sigma_head"]
    profile = _load(out)
    profile["surrogates_per_s"] = {case: {name: _summary(v) for name, v in by.items()} for case, by in got.items()}
    profile["sigma_head_of_run_0"] = heads
    if parent_tree:
        profile["white_equals_parent_bits"] = {case: heads[case]["white"] == heads[case]["white_parent"] for case in CASES}
    profile["cases"] = {k: dict(zip(("T", "Nx", "Ny", "fields", "complexify", "runs"), v)) for k, v in CASES.items()}
    _store(out, profile)


def trace_workload(what):
    sys.path.insert(0, REPO)
    from xmca_amd import _hip
    h = _hip.Handle(0)
    if what in CASES:                      # two red runs: every plane is generated once and filtered once
        T, Nx, Ny, nf, cplx, _ = CASES[what]
        n_out = min(T, Nx if nf == 1 else min(Nx, Ny))
        h.rule_n(T, Nx, Ny, nf, cplx, False, 0, 1, 1e-8, 0, 2, 1, np.float64, n_out, ar1=(_phi(Nx, 1), _phi(Ny, 2) if nf == 2 else None))
        return
    # "estimator": beside the column sums of the constructor's centring, on the same resident field (C2: double, c5_scaled: float)
    for T, N, dt in ((2920, 10000, np.float64), (1200, 41472, np.float32)):
        h.set_field(0, np.random.default_rng(3).standard_normal((T, N)).astype(dt))
        h.center_field(0, N)
        h.lag1_autocorrelation(0, N)


KERNELS = ("philox_normal_kernel", "ar1_carry_kernel", "ar1_filter_kernel", "Lag1Partial", "Lag1Finish",
           "ColumnPartialSums")          # (the last three: functors of column_pass_kernel / column_finish_kernel)


def kernel_stats(path, out, label):
    """rocprofv3's kernel_stats.csv of one `--trace-workload` run -> the kernels this work adds and the ones they are compared with.
    For a rule_n case the generator and the filter saw the same planes, so their totals compare; the bytes the two filter passes move
    come from the shapes (the carry pass reads every segment but the last, the filter pass reads and writes the plane)."""
    sys.path.insert(0, REPO)
    from xmca_amd import _hip
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in KERNELS:
                if key in name:
                    tag = key + ("<float>" if "<float>" in name else "<double>" if "<double>" in name else "")
                    rows[tag] = {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "average_ns": float(r["AverageNs"]),
                                 "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
    entry = {"kernels": rows}
    if label in CASES and "ar1_filter_kernel<double>" in rows:
        T, Nx, Ny, nf, _, _ = CASES[label]
        runs, moved, plane_bytes = 2, 0.0, 0.0
        for N in (Nx, Ny)[:nf]:
            seg = _hip.ar1_segments(T, N)
            carry_rows = seg[-1][0] if len(seg) > 1 else 0
            moved += runs * 8.0 * N * (2 * T + carry_rows)
            plane_bytes += runs * 8.0 * N * T
        filt = rows["ar1_filter_kernel<double>"]["total_ns"] + rows.get("ar1_carry_kernel<double>", {"total_ns": 0.0})["total_ns"]
        gen = rows["philox_normal_kernel<double>"]["total_ns"]
        entry.update({"filter_total_ns": filt, "generator_total_ns": gen, "filter_over_generator": filt / gen,
                      "filter_bytes_moved": moved, "filter_bytes_per_s": moved / (filt * 1e-9),
                      "generator_bytes_written": plane_bytes, "segments": {str(N): len(_hip.ar1_segments(T, N)) for N in (Nx, Ny)[:nf]}})
    profile = _load(out)
    profile.setdefault("kernel_trace", {})[label] = entry
    _store(out, profile)


def _load(out):
    if out and os.path.exists(out):
        with open(out) as f:
            return json.load(f)
    return {}


def _store(out, profile):
    text = json.dumps(profile, indent=1, sort_keys=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("CASE", "NOISE"))
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tree")
    ap.add_argument("--trace-workload", choices=sorted(CASES) + ["estimator"])
    ap.add_argument("--kernel-stats")
    ap.add_argument("--label", default="trace")
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.tree)
    elif a.trace_workload:
        trace_workload(a.trace_workload)
    elif a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out, a.label)
    else:
        throughput(a.out, a.repeats, a.parent_tree)
