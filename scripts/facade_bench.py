#!/usr/bin/env python3
"""The tutorial sequence through the xarray facade, `xMCA(da); apply_coslat(); solve(); rotate(10); predict(da);
reconstructed_fields(10)`, timed call by call.

Shapes: C2 as (2920, 100, 100) float64 with lat in [-80, 80] (tests/golden_inputs.gen_A), and c5_scaled, the float32 stand-in
of the 0.25 degree grid, (1200, 144, 288) with float32 `lat` coordinates - so that the weights do not change the dtype - and a
block of masked grid points (gen_C).  `xarray` is the real package where it can be imported, tests/fake_xarray otherwise
(recorded as `xarray`).  Legs per shape, wall clock of the calls as a user makes them (every one returns host data):

    ctor_coslat_solve   xMCA(da), apply_coslat(), solve() - a new model per call
    rotate10            rotate(10) on the last of those models
    predict_train       predict(da)
    reconstruct10       reconstructed_fields(10)

The first call of each leg is the warm-up, then --repeats timed calls (at least 7): min / median / max and the calls themselves.
The script runs unchanged on an older revision of the package (`--package DIR`: the tree to import `xmca_amd` from), so two
revisions can be run alternately in one session and merged:

    python scripts/facade_bench.py --out new_1.json
    python scripts/facade_bench.py --package ../parent --out parent_1.json          (and again, alternating)
    python scripts/facade_bench.py --merge new_1.json new_2.json --against parent_1.json parent_2.json --out profiles/facade_bench_c2.json

The merge pools the calls of each side per leg (median, min-max spread) and marks a leg `outside_parent_spread` when this
revision's median lies outside the other's [min, max].
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("ctor_coslat_solve", "rotate10", "predict_train", "reconstruct10")


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts), "calls_s": [round(t, 6) for t in ts]}


def _timed(fn, repeats):
    out = fn()                                   # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def _shape_legs(name, xr, xMCA, values, lat, repeats):
    T, ny, nx = values.shape
    da = xr.DataArray(values, dims=['time', 'lat', 'lon'],
                      coords={'time': np.arange(T), 'lat': lat, 'lon': np.linspace(0, 357.5, nx).astype(lat.dtype)})

    def build():
        xm = xMCA(da)
        xm.apply_coslat()
        xm.solve()
        return xm

    res = {"shape": name, "dims": [T, ny, nx], "dtype": str(values.dtype), "lat_dtype": str(lat.dtype), "legs": {}}
    xm, ts = _timed(build, repeats)
    res["legs"]["ctor_coslat_solve"] = _stats(ts)
    res["field_stayed_on_device"] = bool(getattr(xm, "_store_is_raw", False))
    _, ts = _timed(lambda: xm.rotate(10), repeats)
    res["legs"]["rotate10"] = _stats(ts)
    route = getattr(xm, "_transform_vectors", None)
    res["transforms_on_device"] = bool(route is not None and route('left') is not None)
    _, ts = _timed(lambda: xm.predict(da), repeats)
    res["legs"]["predict_train"] = _stats(ts)
    _, ts = _timed(lambda: xm.reconstructed_fields(10), repeats)
    res["legs"]["reconstruct10"] = _stats(ts)
    for leg in LEGS:
        print(json.dumps({"shape": name, "leg": leg, **{k: v for k, v in res["legs"][leg].items() if k != "calls_s"}}), flush=True)
    return res


def _run(args):
    package = os.path.abspath(args.package) if args.package else REPO
    sys.path.insert(0, package)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    try:
        import xarray as xr
        which = "xarray " + getattr(xr, "__version__", "?")
    except Exception:
        sys.path.insert(0, os.path.join(REPO, "tests", "fake_xarray"))
        import xarray as xr
        which = "tests/fake_xarray"
    from golden_inputs import gen_A, gen_C
    import xmca_amd
    from xmca_amd.xarray import xMCA
    assert os.path.dirname(os.path.dirname(os.path.abspath(xmca_amd.__file__))) == package, xmca_amd.__file__
    repeats = max(7, args.repeats)
    shapes = []
    if "c2" in args.shapes:
        shapes.append(_shape_legs("c2", xr, xMCA, gen_A().reshape(2920, 100, 100), np.linspace(-80.0, 80.0, 100), repeats))
    if "c5_scaled" in args.shapes:
        C = gen_C(1200, 144, 288).copy()
        C[:, 3:7, 10:20] = np.nan                    # land points: masked columns
        shapes.append(_shape_legs("c5_scaled", xr, xMCA, C, np.linspace(-80.0, 80.0, 144).astype(np.float32), repeats))
    return {"case": "facade bench: xMCA(da); apply_coslat(); solve(); rotate(10); predict(da); reconstructed_fields(10)",
            "package": os.path.relpath(package, REPO), "xarray": which, "repeats": repeats, "shapes": shapes}


def _pool(files):
    runs = [json.load(open(f)) for f in files]
    pooled = {}
    for run in runs:
        for shape in run["shapes"]:
            for leg, st in shape["legs"].items():
                pooled.setdefault(shape["shape"], {}).setdefault(leg, []).extend(st["calls_s"])
    flags = {s["shape"]: {k: s[k] for k in ("dims", "dtype", "lat_dtype", "field_stayed_on_device", "transforms_on_device")}
             for s in runs[0]["shapes"]}
    return runs, pooled, flags


def _merge(args):
    runs, new, flags = _pool(args.merge)
    _, old, old_flags = _pool(args.against)
    shapes = []
    for name in new:
        legs = {}
        for leg in LEGS:
            a, b = _stats(new[name][leg]), _stats(old[name][leg])
            for st in (a, b):
                del st["calls_s"]
            legs[leg] = {"this": a, "parent": b, "parent_over_this_median": b["median"] / a["median"],
                         "outside_parent_spread": not (b["min"] <= a["median"] <= b["max"])}
        shapes.append({"shape": name, **flags[name], "parent_field_stayed_on_device": old_flags[name]["field_stayed_on_device"],
                       "parent_transforms_on_device": old_flags[name]["transforms_on_device"], "legs": legs})
    return {"case": runs[0]["case"], "xarray": runs[0]["xarray"], "runs_per_side": [len(args.merge), len(args.against)],
            "order": "alternating processes in one session, this revision first", "seconds": True,
            "not_measured": ["the full-size C5 field (1200 x 720 x 1440)", "time-dependent and dtype-promoting weights (host route, unchanged)",
                             "fields(original_scale=True)", "the real xarray package when `xarray` says tests/fake_xarray"],
            "shapes": shapes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", nargs="+", default=["c2", "c5_scaled"], choices=["c2", "c5_scaled"])
    ap.add_argument("--package", default=None, help="tree to import xmca_amd from (default: this one)")
    ap.add_argument("--merge", nargs="+", default=None, help="result files of this revision to pool")
    ap.add_argument("--against", nargs="+", default=None, help="result files of the other revision")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.against:
            ap.error("--merge needs --against")
        res = _merge(args)
    else:
        res = _run(args)
    line = json.dumps(res)
    if args.merge:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
