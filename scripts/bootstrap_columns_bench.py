#!/usr/bin/env python3
"""bootstrapping(n_runs, n_modes=10, axis=1) at C2 (T = 2920 x N = 10 000 float64, tests/golden_inputs.make_input("c2_full")):
wall time per replicate, unrotated and after rotate(10).

The script measures the checkout it is pointed at (--repo, default: the one it lies in) and is meant to be run twice: on this
commit (column replicates on the device, xmca_bootstrap_runs_columns) and on its parent (the reference's host loop: per
replicate a numpy fancy index of the field, a fresh MCA - host centering, NaN scan, upload - and one device solve).  The parent
is the baseline.  Each leg: one warm-up call, then --repeats timed calls of --runs replicates under the same numpy seed; a call
returns after the spectra are on the host.  `path` says which route the checkout took (the `resample` stage timer of the
handle).  --merge PARENT.json THIS.json [--trace DIR] writes the record profiles/bootstrap_columns_bench_c2.json: per leg the
parent's and this commit's seconds per replicate (min / median / max over the repeats), the speed-up of the medians and
`separated` - whether the medians differ by more than the two min-max spreads together - and, from one
`rocprofv3 --kernel-trace --memory-copy-trace --stats` run of --trace-target, the column gather next to a device-to-device copy of
the same byte count (a replicate with no side resampled copies the working field with hipMemcpyDtoD).

    python scripts/bootstrap_columns_bench.py [--repo DIR] [--runs 8] [--repeats 5] [--out FILE]
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python scripts/bootstrap_columns_bench.py --trace-target
    python scripts/bootstrap_columns_bench.py --merge PARENT.json THIS.json --trace DIR --out profiles/bootstrap_columns_bench_c2.json
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def _import(repo):
    sys.path.insert(0, repo)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from golden_inputs import make_input
    from xmca_amd.array import MCA
    return make_input, MCA


def measure(repo, runs, repeats):
    make_input, MCA = _import(repo)
    X = make_input("c2_full")[0]
    legs = []
    for name, rot in (("c2_unrotated", None), ("c2_rot10", 10)):
        m = MCA(X)
        m.solve()
        if rot:
            m.rotate(rot)
        dev = m._device()

        def call(n):
            np.random.seed(5)
            t0 = time.perf_counter()
            out = m.bootstrapping(n, n_modes=10, axis=1, disable_progress=True)
            return time.perf_counter() - t0, out
        dev.reset_timings()
        first, out = call(2)                                   # warm-up: workspaces, lanes, code objects
        path = "device" if "resample" in dev.timings() else "host loop"
        ts = [call(runs)[0] / runs for _ in range(repeats)]
        legs.append({"leg": name, "path": path, "runs_per_call": runs, "warmup_call_s": first, "s_per_replicate": _stats(ts),
                     "spectrum_run0_first3": [float(v) for v in out[:3, 0]]})
        print(json.dumps(legs[-1]), flush=True)
        del m
    return {"case": "bootstrapping(n_runs, n_modes=10, axis=1) at C2", "field": list(X.shape), "dtype": str(X.dtype), "legs": legs}


def trace_target(repo):
    """what the rocprofv3 run executes: 4 column replicates (the gather), then 4 replicates with no side resampled (the copy)"""
    make_input, MCA = _import(repo)
    m = MCA(make_input("c2_full")[0])
    m.solve()
    np.random.seed(5)
    m.bootstrapping(4, n_modes=10, axis=1, disable_progress=True)
    m.bootstrapping(4, n_modes=10, axis=1, on_left=False, disable_progress=True)


def read_trace(folder, field_bytes):
    """rows of the stats tables that name the gather kernel and device-to-device copies"""
    rows = []
    for path in sorted(glob.glob(os.path.join(folder, "**", "*stats*.csv"), recursive=True)):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                if "gather_concat_columns" in name or "DEVICE_TO_DEVICE" in name.upper() or "copybuffer" in name.lower():
                    rows.append({"table": os.path.basename(path), **{k: row[k] for k in row if k in (
                        "Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage")}})
    out = {"field_bytes": field_bytes, "rows": rows}
    gather = [r for r in rows if "gather_concat_columns" in r["Name"]]
    copies = [r for r in rows if "gather_concat_columns" not in r["Name"]]
    if gather:
        out["gather_avg_ms"] = float(gather[0]["AverageNs"]) / 1e6
        out["gather_gb_per_s_read_plus_write"] = 2 * field_bytes / float(gather[0]["AverageNs"])
    if gather and copies:
        # the copy of the whole field is the slowest device-to-device row (index uploads and small copies are not D2D)
        copy = max(copies, key=lambda r: float(r["AverageNs"]))
        out["dtod_copy_avg_ms"] = float(copy["AverageNs"]) / 1e6
        out["gather_over_copy"] = float(gather[0]["AverageNs"]) / float(copy["AverageNs"])
    if not gather:
        out["gather_avg_ms"] = out["gather_over_copy"] = "NOT MEASURED"
    return out


def merge(parent_file, this_file, trace_dir):
    parent, this = (json.load(open(f)) for f in (parent_file, this_file))
    legs = []
    for a, b in zip(parent["legs"], this["legs"]):
        pa, pb = a["s_per_replicate"], b["s_per_replicate"]
        legs.append({"leg": a["leg"], "runs_per_call": b["runs_per_call"],
                     "parent": {"path": a["path"], "s_per_replicate": pa, "warmup_call_s": a["warmup_call_s"]},
                     "this_commit": {"path": b["path"], "s_per_replicate": pb, "warmup_call_s": b["warmup_call_s"]},
                     "speedup_median": pa["median"] / pb["median"],
                     "spread_s": (pa["max"] - pa["min"]) + (pb["max"] - pb["min"]),
                     "separated": pa["median"] - pb["median"] > (pa["max"] - pa["min"]) + (pb["max"] - pb["min"]),
                     "max_rel_spectrum_diff": float(np.max(np.abs(np.array(a["spectrum_run0_first3"]) - np.array(b["spectrum_run0_first3"]))
                                                           / np.array(a["spectrum_run0_first3"])))})
    rec = {"case": this["case"], "field": this["field"], "dtype": this["dtype"], "legs": legs}
    field_bytes = int(np.prod(this["field"])) * 8
    if trace_dir:
        rec["gather_kernel"] = read_trace(trace_dir, field_bytes)
        g = rec["gather_kernel"].get("gather_avg_ms")
        if isinstance(g, float):
            rec["gather_kernel"]["share_of_a_replicate_unrotated"] = g / 1e3 / legs[0]["this_commit"]["s_per_replicate"]["median"]
    else:
        rec["gather_kernel"] = {"gather_avg_ms": "NOT MEASURED", "dtod_copy_avg_ms": "NOT MEASURED", "gather_over_copy": "NOT MEASURED",
                                "share_of_a_replicate_unrotated": "NOT MEASURED"}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=HERE)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-target", action="store_true")
    ap.add_argument("--merge", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_target:
        trace_target(args.repo)
        return
    res = merge(args.merge[0], args.merge[1], args.trace) if args.merge else measure(args.repo, args.runs, args.repeats)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
