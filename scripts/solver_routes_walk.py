"""Seeded walk over every route of Solver (csrc/solver.h), for same-bits comparisons of two builds of the library.

    python scripts/solver_routes_walk.py run --lib xmca_amd/libxmca_hip.so --out out/walk_a
    python scripts/solver_routes_walk.py compare out/walk_parent out/walk_parent2 out/walk_child --json out/walk.json

`run` starts one fresh process per combination of the route switches (they are read once per process), with XMCA_TRACE=solve.
Every process walks the same cases - one field dual / primal, two fields in all four wide / narrow pairings with all, some
and no vectors, a spectrum graded over five decades (refine_weak_block, refine_by_deflation), an odd prime T (Fourier
reduction by GEMM), each real and complexified, float32 and float64; then solve(extend='exp'), rule_n and bootstrapping,
rotated and not - and writes every returned array to <out>/<switches>/<case>.npy, the solver's trace lines and, per case, the
stage names and the eigensolver's route flags to <out>/<switches>/routes.txt.  A process that fails ends the walk.
`compare` takes the first directory as the reference run, the second as its repeat and the third as the candidate, and
compares the arrays byte for byte (NaN included) and the text records case by case (trace lines of one case as a sorted
list: the lanes of a replicate call print concurrently)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWITCHES = [
    {},
    {"XMCA_CHOLESKY_FACTOR": "0"},
    {"XMCA_ONE_SIDED": "0"},
    {"XMCA_CHOLESKY": "0"},
    {"XMCA_ONE_SIDED": "0", "XMCA_CHOLESKY": "0"},
    {"XMCA_ANALYTIC": "0"},
    {"XMCA_ANALYTIC": "0", "XMCA_ONE_SIDED": "0"},
    {"XMCA_ANALYTIC": "0", "XMCA_CHOLESKY_FACTOR": "0"},
    {"XMCA_DEFLATE_BELOW": "0"},
]


def switches_name(sw):
    return "_".join("%s=%s" % (k[5:].lower(), v) for k, v in sorted(sw.items())) or "default"


def coupled(rng, T, Nx, Ny, k=5):
    pcs = rng.standard_normal((T, k)) * (8.0 * 0.7 ** np.arange(k))
    left = pcs @ rng.standard_normal((k, Nx)) + 0.5 * rng.standard_normal((T, Nx))
    right = pcs @ rng.standard_normal((k, Ny)) + 0.5 * rng.standard_normal((T, Ny))
    return left, right


def graded(rng, T, N, decades):
    """as scripts/deflation_probe.py: variances graded over 2 * decades"""
    def field(shift, n):
        x = np.linspace(0, 1, n)
        modes = np.cos(np.pi * (np.arange(T)[:, None] + shift) * x[None, :])
        return (rng.standard_normal((T, T)) * np.logspace(0, -decades, T)) @ modes
    return field(0.0, N), field(0.3, N - 50)


def center(x):
    return np.ascontiguousarray(x - x.mean(axis=0))


def walk(out_dir):
    from xmca_amd import _hip
    from xmca_amd.array import MCA
    h = _hip.Handle(0)
    routes = open(os.path.join(out_dir, "routes.txt"), "w")

    def begin(case):
        sys.stderr.write("== case %s\n" % case)
        sys.stderr.flush()
        h.reset_timings()

    def save(case, name, a):
        np.save(os.path.join(out_dir, (case + "/" + name).replace("/", "__") + ".npy"), np.asarray(a))

    def handle_case(case, fields, cplx, n_vec):
        begin(case)
        for side, f in enumerate(fields):
            h.set_field(side, f)
        if cplx:
            h.complexify(fields[0].shape[0])
        rank = h.solve(len(fields), n_vec)
        save(case, "sigma", h.singular_values(rank))
        n = rank if n_vec < 0 else min(n_vec, rank)
        for side, f in enumerate(fields):
            if n > 0:
                save(case, "vectors%d" % side, h.vectors(side, n, f.shape[1], np.float64))
        routes.write("%s: rank %d stages %s evd %s\n" % (case, rank, ",".join(h.timings().keys()), json.dumps(h.solve_info())))
        if cplx:
            h.decomplexify()

    rng = np.random.default_rng(2026)
    T = 96
    wide_a, wide_b = coupled(rng, T, 400, 260)
    narrow_a, narrow_b = coupled(rng, T, 60, 50)
    odd_a, odd_b = coupled(rng, 97, 300, 210)
    grad_a, grad_b = graded(rng, 120, 300, 5)
    sets = {
        "one_dual": (wide_a,), "one_primal": (narrow_a,),
        "wide_wide": (wide_a, wide_b), "wide_narrow": (wide_a, narrow_b), "narrow_wide": (narrow_a, wide_b),
        "narrow_narrow": (narrow_a, narrow_b), "odd_T": (odd_a, odd_b), "one_odd_T": (odd_a,), "graded": (grad_a, grad_b),
    }
    for dtype in (np.float64, np.float32):
        for name, fields in sets.items():
            fields = [center(f).astype(dtype) for f in fields]
            for cplx in (False, True):
                for n_vec in ((-1, 6, 0) if name in ("wide_wide", "odd_T") else (-1, 0)):
                    handle_case("solve/%s/%s/%s/n_vec%d" % (np.dtype(dtype).name, name, "complex" if cplx else "real", n_vec), fields, cplx, n_vec)

    # through the class: extend='exp', rule_n and bootstrapping (ReplicateRunner's choice of route), rotated and not
    def model_case(case, fields, complexify, extend=False, rotate=0, dtype=np.float64, boot=True):
        begin(case)
        m = MCA(*[f.astype(dtype) for f in fields], handle=h)
        m.solve(complexify=complexify, extend=extend, period=12)
        if rotate:
            m.rotate(rotate, power=1)
        save(case, "svals", m.singular_values())
        for key in m._keys:
            save(case, "V/" + key, m._V[key])
        save(case, "rule_n", m.rule_n(3, seed=7, dtype=dtype))
        if boot:
            np.random.seed(5)
            save(case, "boot", m.bootstrapping(3, n_modes=8, on_left=True, on_right=len(fields) == 2))
        routes.write("%s: stages %s\n" % (case, ",".join(h.timings().keys())))

    model_case("model/extend_exp", (wide_a, wide_b), True, extend='exp')
    model_case("model/extend_exp_f32", (wide_a, wide_b), True, extend='exp', dtype=np.float32)
    for dtype in (np.float64, np.float32):
        dn = np.dtype(dtype).name
        for name in ("one_dual", "wide_wide", "wide_narrow", "narrow_narrow") if dtype == np.float64 else ("wide_wide",):
            for cplx in (False, True):
                for rot in (0, 4):
                    model_case("model/%s/%s/%s/%s" % (dn, name, "complex" if cplx else "real", "rotated" if rot else "unrotated"),
                               sets[name], cplx, rotate=rot, dtype=dtype)
    routes.close()


def run(lib, out):
    for sw in SWITCHES:
        d = os.path.join(out, switches_name(sw))
        os.makedirs(d, exist_ok=True)
        env = dict(os.environ, XMCA_TRACE="solve", **sw)
        cmd = [sys.executable, os.path.abspath(__file__), "walk", "--out", d] + (["--lib", lib] if lib else [])
        p = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, text=True, timeout=600)
        with open(os.path.join(d, "trace.txt"), "w") as f:
            f.writelines(l + "\n" for l in p.stderr.splitlines() if l.startswith("== case") or l.startswith("[xmca solve]"))
        print("%s: exit %d, %d arrays" % (switches_name(sw), p.returncode, len([x for x in os.listdir(d) if x.endswith(".npy")])), flush=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            sys.exit(1)                      # nothing more is started on the device after a failure


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def by_case(text):
    """the lines of each case, sorted: the lanes of a rule_n / bootstrap call print their trace lines concurrently"""
    cases, cur = [], []
    for line in text.splitlines():
        if line.startswith("== case"):
            cases.append(sorted(cur))
            cur = []
        cur.append(line)
    return cases + [sorted(cur)]


def compare(ref, repeat, cand, json_path):
    outputs, excluded, differ, text_differ = [], [], [], []
    for sw in sorted(os.listdir(ref)):
        for name in sorted(os.listdir(os.path.join(ref, sw))):
            paths = [os.path.join(d, sw, name) for d in (ref, repeat, cand)]
            if name.endswith(".txt"):
                texts = [by_case(open(p).read()) for p in paths]
                if not (texts[0] == texts[1] == texts[2]):
                    text_differ.append(sw + ":" + name)
                continue
            a, b, c = (np.load(p) for p in paths)
            key = sw + ":" + name[:-4].replace("__", "/")
            if not same(a, b):
                excluded.append(key)             # the reference build does not reproduce this output itself
                continue
            outputs.append(key)
            if not same(a, c):
                differ.append(key)
        for d in (repeat, cand):
            extra = set(os.listdir(os.path.join(d, sw))) ^ set(os.listdir(os.path.join(ref, sw)))
            if extra:
                differ.append("%s: file sets differ (%s)" % (sw, ", ".join(sorted(extra))))
    rec = {"n_outputs": len(outputs) + len(excluded), "reference_equals_its_repeat": len(outputs), "excluded_not_reproducible": excluded,
           "candidate_equals_reference": len(outputs) - len([d for d in differ if "file sets" not in d]), "candidate_differs": differ,
           "routes_and_trace_files_that_differ": text_differ, "switch_combinations": sorted(os.listdir(ref))}
    print(json.dumps({k: v for k, v in rec.items()}, indent=1))
    if json_path:
        with open(json_path, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if not differ and not text_differ and len(excluded) <= 0.05 * rec["n_outputs"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "walk", "compare"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.mode == "compare":
        sys.exit(compare(a.dirs[0], a.dirs[1], a.dirs[2], a.json))
    if a.lib:
        from xmca_amd import build as _build
        _build.LIB = os.path.abspath(a.lib)      # the library this process binds (xmca_amd._hip.library_path)
    if a.mode == "run":
        run(os.path.abspath(a.lib) if a.lib else None, a.out)
    else:
        walk(a.out)
