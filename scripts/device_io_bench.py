#!/usr/bin/env python3
"""A field that starts as a tensor on the GPU, results wanted as tensors on the GPU: what the workflow costs through the class.

With tensor input and `output='torch'` (this commit) the field is copied on the device by `xmca_set_field_strided` and the
field-sized results are written on the device.  A commit without them (detected: `_hip.Handle.set_field_strided` is missing) can
only go the long way - `MCA(x.cpu().numpy())`, `torch.from_numpy(result).to(device)` - and that is what this file times there: the
same file runs on both, one process per commit, and `--merge` puts the runs of a session side by side.

Cases: C2 (2920 x 10 000 float64, tests/golden_inputs.gen_A) and c5_scaled (1200 x 144 x 288 float32 with masked grid points).
Legs, timed between two `torch.cuda.synchronize()`: constructor + solve(), rotate(10), eofs(10), reconstructed_fields(10),
predict(x_new) (x_new: 365 new time steps on the GPU) and homogeneous_patterns(10).  The whole workflow is repeated; the first
pass is reported apart.  With the device routes present, the copy kernel alone (hipEvents around it, `ingest_strided` of the
handle's timers) for the stride regimes at C2 size, in GB/s of bytes read + written, next to torch's own device-to-device copy.

    python scripts/device_io_bench.py [--repeats 7] [--cases c2,c5_scaled] [--out FILE]
    python scripts/device_io_bench.py --merge OUT label=FILE [label=FILE ...]
    python scripts/device_io_bench.py --workflow          # one C2 workflow and nothing else (for a memory-copy trace)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from golden_inputs import gen_A, gen_C  # noqa: E402
from xmca_amd import _hip  # noqa: E402
from xmca_amd.array import MCA  # noqa: E402

DEVICE_IO = hasattr(_hip.Handle, "set_field_strided")
DEV = torch.device("cuda", 0)
LEGS = ["ctor_solve", "rotate_10", "eofs_10", "reconstructed_fields_10", "predict", "homogeneous_patterns_10"]


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts)}


def _to_gpu(result):
    """the long way back: every array of a getter's result uploaded"""
    if isinstance(result, tuple):
        return tuple(_to_gpu(r) for r in result)
    return {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in result.items()}


def _workflow(h, x, x_new):
    """one pass; returns ({leg: seconds}, the results of the getters)"""
    t, out = {}, {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t[name] = time.perf_counter() - t0
        return res

    def build():
        m = MCA(x, handle=h) if DEVICE_IO else MCA(x.cpu().numpy(), handle=h)
        m.solve()
        return m
    m = timed("ctor_solve", build)
    timed("rotate_10", lambda: m.rotate(10))
    out["eofs_10"] = timed("eofs_10", lambda: _to_gpu(m.eofs(10)))
    out["reconstructed_fields_10"] = timed("reconstructed_fields_10", lambda: _to_gpu(m.reconstructed_fields(10)))
    out["predict"] = timed("predict", lambda: _to_gpu(m.predict(left=x_new if DEVICE_IO else x_new.cpu().numpy())))
    out["homogeneous_patterns_10"] = timed("homogeneous_patterns_10", lambda: _to_gpu(m.homogeneous_patterns(10)))
    assert all(v.device.type == "cuda" for r in out.values() for d in (r if isinstance(r, tuple) else (r,)) for v in d.values())
    return t, out


def _case(name):
    if name == "c2":
        X = gen_A()
    else:
        X = gen_C(1200, 144, 288).copy()
        X[:, 3:7, 10:20] = np.nan                    # land points: masked columns
    x = torch.from_numpy(X).to(DEV)
    x_new = (x[:365] * 1.25 + 0.5).contiguous()
    return x, x_new


def _run_case(name, repeats):
    x, x_new = _case(name)
    h = _hip.Handle(0)
    first, _ = _workflow(h, x, x_new)
    ts = {leg: [] for leg in LEGS}
    for _ in range(repeats):
        t, out = _workflow(h, x, x_new)
        for leg in LEGS:
            ts[leg].append(t[leg])
    check = {leg: float(torch.nan_to_num(r[0]["left"] if isinstance(r, tuple) else r["left"]).abs().double().sum().item())
             for leg, r in out.items()}
    res = {"case": name, "shape": list(x.shape), "dtype": str(x.dtype), "first_s": first, "legs_s": {leg: _stats(v) for leg, v in ts.items()},
           "abs_sum_of_left_result": check}
    print(json.dumps(res), flush=True)
    return res


def _ingest_alone(repeats):
    """the copy kernel of xmca_set_field_strided at C2 size, float64, per stride regime"""
    T, N = 2920, 10000
    g = torch.Generator(device=DEV).manual_seed(1)
    layouts = {
        "rows_contiguous": lambda: torch.randn((T, N), generator=g, dtype=torch.float64, device=DEV),
        "rows_padded_misaligned (big[:, 3:3+N], odd pitch)": lambda: torch.randn((T, N + 7), generator=g, dtype=torch.float64, device=DEV)[:, 3:3 + N],
        "transpose (space-major parent, .T)": lambda: torch.randn((N, T), generator=g, dtype=torch.float64, device=DEV).T,
        "gather (big[::2, ::3])": lambda: torch.randn((2 * T, 3 * N), generator=g, dtype=torch.float64, device=DEV)[::2, ::3],
    }
    from xmca_amd.array import _device_view
    h = _hip.Handle(0)
    nbytes = 2.0 * T * N * 8
    out = {}
    for name, make in layouts.items():
        view = make()
        dv = _device_view(view)
        torch.cuda.synchronize()
        h.set_field_strided(0, dv)                    # (allocates the resident buffer)
        ms = []
        for _ in range(repeats):
            h.reset_timings()
            h.set_field_strided(0, dv)
            ms.append(h.timings()["ingest_strided"])
        dst = torch.empty((T, N), dtype=torch.float64, device=DEV)
        tms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(view)
            b.record()
            torch.cuda.synchronize()
            tms.append(a.elapsed_time(b))
        out[name] = {"regime": _hip.ingest_regime(T, N, dv.stride_t, dv.stride_n), "kernel_ms": _stats(ms),
                     "GBps_median": nbytes / (np.median(ms) * 1e-3) / 1e9, "GBps_min_max": [nbytes / (max(ms) * 1e-3) / 1e9, nbytes / (min(ms) * 1e-3) / 1e9],
                     "torch_copy_ms": _stats(tms), "torch_copy_GBps_median": nbytes / (np.median(tms) * 1e-3) / 1e9}
        del view, dst
    print(json.dumps({"ingest_alone": out}), flush=True)
    return out


def _merge(out_path, labelled):
    runs = []
    for item in labelled:
        label, path = item.split("=", 1)
        with open(path) as fh:
            r = json.loads(fh.readline())
        r["label"] = label
        runs.append(r)
    summary = {}
    for r in runs:
        side = "device_io" if r["device_io"] else "parent_long_way"
        for c in r["cases"]:
            for leg, s in c["legs_s"].items():
                e = summary.setdefault(c["case"], {}).setdefault(leg, {}).setdefault(side, [])
                e.append({"run": r["label"], "median_ms": 1e3 * s["median"], "min_ms": 1e3 * s["min"], "max_ms": 1e3 * s["max"]})
    for legs in summary.values():
        for leg, sides in legs.items():
            for side in list(sides):
                v = sides[side]
                sides[side] = {"median_ms": float(np.median([x["median_ms"] for x in v])), "min_ms": min(x["min_ms"] for x in v),
                               "max_ms": max(x["max_ms"] for x in v), "runs": v}
            if len(sides) == 2:
                p, d = sides["parent_long_way"], sides["device_io"]
                sides["inside_parent_spread"] = bool(p["min_ms"] <= d["median_ms"] <= p["max_ms"])
                sides["faster_than_parent_min"] = bool(d["median_ms"] < p["min_ms"])
    res = {"case": "device io bench: a GPU tensor in, GPU tensors out; parent = MCA(x.cpu().numpy()) and torch.from_numpy(result).to(device)",
           "order_of_runs": [r["label"] for r in runs], "summary_ms": summary,
           "ingest_alone": next((r["ingest_alone"] for r in runs if r.get("ingest_alone")), None),
           "not_measured": "full-size C5 (1200 x 720 x 1440 float32)", "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="c2,c5_scaled")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--workflow", action="store_true")
    args = ap.parse_args()
    if args.merge:
        return _merge(args.merge[0], args.merge[1:])
    if args.workflow:
        x, x_new = _case("c2")
        torch.cuda.synchronize()
        print(json.dumps({"workflow": "c2", "device_io": DEVICE_IO, "legs_s": _workflow(_hip.Handle(0), x, x_new)[0]}), flush=True)
        return
    cases = [_run_case(name, args.repeats) for name in args.cases.split(",")]
    res = {"device_io": DEVICE_IO, "repeats": args.repeats, "cases": cases, "ingest_alone": _ingest_alone(args.repeats) if DEVICE_IO else None}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
