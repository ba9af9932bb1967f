#!/usr/bin/env python3
"""`solve(n_modes=10)` against `solve()` (+ `truncate(10)`), at C2 (2920 x 10 000 float64, tests/golden_inputs.gen_A) and at
c5_scaled (1200 x 41 472 float32, gen_C): wall clock of the calls on a model whose field is resident on the device
(`preprocess='device'`), and the device memory the result holds.

One process measures one side, so that two revisions can be run alternately in one session and merged:

    python scripts/partial_solve_bench.py --side full --package ../parent --out parent_1.json    (solve(), the parent's tree)
    python scripts/partial_solve_bench.py --side partial --out new_1.json                         (solve(n_modes=10))
    ... and again, alternating ...
    python scripts/partial_solve_bench.py --merge new_*.json --against parent_*.json --out profiles/partial_solve_bench.json

Legs (the first call of each is the warm-up, then --repeats timed calls, at least 7; medians and [min, max] over the pooled calls):
    solve            solve() | solve(n_modes=10)
    solve_truncate   solve(); truncate(10)   (side full only: truncate fetches every vector to the host)
    solve_rotate     solve() | solve(n_modes=10), then rotate(10)
`result_kib`: the resident vector planes after solve (`Device.result_info()`; T x N x itemsize for a tree that has no such call).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10


def _stats(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "n": len(ts), "calls_s": [round(t, 6) for t in ts]}


def _timed(fn, repeats):
    fn()                                         # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def _shape(name, MCA, field, side, repeats):
    m = MCA(field, preprocess="device")
    kw = {"n_modes": K} if side == "partial" else {}
    legs = {"solve": _stats(_timed(lambda: m.solve(**kw), repeats))}
    dev = m._device()
    T, N = field.shape[0], int(np.prod(field.shape[1:]))
    info = dev.solve_info()[0]
    if hasattr(dev, "result_info"):
        kib = dev.result_info()["vector_kib"][0]
    else:
        kib = -(-T * N * field.dtype.itemsize // 1024)
    if side == "full":
        def solve_truncate():
            m.solve()
            m.truncate(K)
        legs["solve_truncate"] = _stats(_timed(solve_truncate, repeats))

    def solve_rotate():
        m.solve(**kw)
        m.rotate(K)
    legs["solve_rotate"] = _stats(_timed(solve_rotate, repeats))
    for leg, st in legs.items():
        print(json.dumps({"shape": name, "side": side, "leg": leg, **{k: v for k, v in st.items() if k != "calls_s"}}), flush=True)
    return {"shape": name, "dims": [T, N], "dtype": str(field.dtype), "legs": legs, "result_kib": int(kib),
            "n_eigvec": info.get("n_eigvec"), "tridiag": info.get("tridiag")}


def _run(args):
    package = os.path.abspath(args.package) if args.package else REPO
    sys.path.insert(0, package)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from golden_inputs import gen_A, gen_C
    import xmca_amd
    from xmca_amd.array import MCA
    assert os.path.dirname(os.path.dirname(os.path.abspath(xmca_amd.__file__))) == package, xmca_amd.__file__
    repeats = max(7, args.repeats)
    shapes = []
    if "c2" in args.shapes:
        shapes.append(_shape("c2", MCA, gen_A(), args.side, repeats))
    if "c5_scaled" in args.shapes:
        shapes.append(_shape("c5_scaled", MCA, gen_C(1200, 144, 288), args.side, repeats))
    return {"side": args.side, "package": os.path.relpath(package, REPO), "repeats": repeats, "shapes": shapes}


def _pool(files):
    pooled, meta = {}, {}
    for f in files:
        for shape in json.load(open(f))["shapes"]:
            meta[shape["shape"]] = {k: shape[k] for k in ("dims", "dtype", "result_kib", "n_eigvec", "tridiag")}
            for leg, st in shape["legs"].items():
                pooled.setdefault(shape["shape"], {}).setdefault(leg, []).extend(st["calls_s"])
    return pooled, meta


def _merge(args):
    sides = {"partial": _pool(args.merge), "full_parent": _pool(args.against)}
    shapes = []
    for name in sides["partial"][0]:
        entry = {"shape": name, "legs": {}}
        for side, (pooled, meta) in sides.items():
            entry.setdefault("result", {})[side] = meta[name]
            for leg, calls in pooled[name].items():
                st = _stats(calls)
                del st["calls_s"]
                entry["legs"].setdefault(leg, {})[side] = {k: (round(v * 1e3, 3) if k != "n" else v) for k, v in st.items()}
        shapes.append(entry)
    return {"case": "solve(n_modes=10) against solve() [+ truncate(10)] of the parent, processes alternating in one session; ms",
            "files": {"partial": [os.path.basename(f) for f in args.merge], "full_parent": [os.path.basename(f) for f in args.against]},
            "shapes": shapes}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", choices=("full", "partial"), default="partial")
    ap.add_argument("--package", help="tree to import xmca_amd from (default: this one)")
    ap.add_argument("--shapes", nargs="+", default=["c2", "c5_scaled"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--against", nargs="+")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "partial_solve_bench.json"))
    args = ap.parse_args()
    res = _merge(args) if args.merge else _run(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
