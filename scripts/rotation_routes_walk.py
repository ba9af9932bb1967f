"""Seeded walk over every route of Rotator (csrc/solver.h), for same-bits comparisons of two builds of the library.

    python scripts/rotation_routes_walk.py run --lib xmca_amd/libxmca_hip.so --out out/rot_a
    python scripts/rotation_routes_walk.py compare out/rot_parent out/rot_parent2 out/rot_child --json out/rot_walk.json

`run` starts one fresh process per set of the rotation switches, with XMCA_TRACE=rot,giveup.  Every process walks the same
cases: Handle.rotate_loadings on the fourth-moment route (real, p <= 12; short and long grids), the persistent loop (real
p > 12, complex; tiles resident in LDS and not) and the GEMM-based route (real p = 70, complex p = 52), each with
varimax_only, power 1 and 4, n_left = N and N // 3, one case with gamma = 0.3; a loop that does not converge and a zero row
(the only two cases that may raise: error and last_iters); MCA.rotate straight after solve() for a float64 field, a float32 field and two complexified fields;
rule_n and bootstrapping, rotated, on two lanes.  It writes R, Phi, B, both norms and n_iter to <out>/<switches>/<case>.npy,
the trace lines to <out>/<switches>/trace.txt and the give-up counter around every case to <out>/<switches>/giveups.txt.  A
process that fails ends the walk.
`compare` takes the first directory as the reference run, the second as its repeat and the third as the candidate: arrays
byte for byte (NaN included), trace lines case by case as sorted lists (the lanes of a replicate call print concurrently).
Cases during which the give-up counter moved outside the TEST_GIVEUP set (another process held CUs) are named in the record."""
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
    {"XMCA_VARIMAX_PERSIST": "0"},
    {"XMCA_VARIMAX_TEST_GIVEUP": "7"},
    {"XMCA_ROT_TWO_STAGE": "0"},
    {"XMCA_ROT_TWO_STAGE": "1"},
]


def switches_name(sw):
    return "_".join("%s=%s" % (k[5:].lower(), v) for k, v in sorted(sw.items())) or "default"


def loadings(rng, N, p, cplx):
    """as scripts/rot_bench.py: one bump per mode over noise, mixed by a random orthogonal / unitary matrix"""
    L = 0.2 * rng.standard_normal((N, p))
    w = N // p
    for j in range(p):
        L[j * w:(j + 1) * w, j] += np.hanning(w) * (3 - 0.02 * j)
    if cplx:
        L = L * np.exp(1j * rng.uniform(0, 0.5, (N, 1))) + 0.05j * rng.standard_normal((N, p))
        Q, _ = np.linalg.qr(rng.standard_normal((p, p)) + 1j * rng.standard_normal((p, p)))
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    return L @ Q


def coupled(rng, T, Nx, Ny, k=5):
    pcs = rng.standard_normal((T, k)) * (8.0 * 0.7 ** np.arange(k))
    left = pcs @ rng.standard_normal((k, Nx)) + 0.5 * rng.standard_normal((T, Nx))
    right = pcs @ rng.standard_normal((k, Ny)) + 0.5 * rng.standard_normal((T, Ny))
    return left, right


def walk(out_dir):
    from xmca_amd import _hip
    from xmca_amd.array import MCA
    h = _hip.Handle(0)
    lib = _hip.load_library()
    giveups = open(os.path.join(out_dir, "giveups.txt"), "w")

    def case(name, fn):
        sys.stderr.write("== case %s\n" % name)
        sys.stderr.flush()
        before = int(lib.xmca_persistent_giveups())
        try:
            out = fn()
        except (RuntimeError, np.linalg.LinAlgError) as e:           # the library's own errors (no convergence, NaN) are results;
            out = {"error": np.array([type(e).__name__, str(h.last_iters)])}    # anything else ends the walk
        for key, a in out.items():
            if a is not None:
                np.save(os.path.join(out_dir, (name + "/" + key).replace("/", "__") + ".npy"), np.asarray(a))
        giveups.write("%s: %d -> %d\n" % (name, before, int(lib.xmca_persistent_giveups())))

    def rotate_loadings(L, **kw):
        return lambda: h.rotate_loadings(L, want_B=True, **kw)

    rng = np.random.default_rng(2027)
    shapes = [(p, N, False) for p in (2, 5, 12, 13, 17, 40, 64) for N in (300, 70000)]
    shapes += [(p, N, True) for p in (4, 10, 20, 48) for N in (600, 20000)]
    shapes += [(70, 600, False), (52, 600, True)]
    for p, N, cplx in shapes:
        L = loadings(rng, N, p, cplx)
        tag = "loadings/%s/p%d/N%d" % ("complex" if cplx else "real", p, N)
        case(tag + "/varimax_only", rotate_loadings(L, n_left=N, varimax_only=True))
        for power in (1, 4):
            for n_left in (N, N // 3):
                case(tag + "/power%d/n_left%d" % (power, n_left), rotate_loadings(L, n_left=n_left, power=power))
    case("loadings/real/p17/N300/gamma0.3", rotate_loadings(loadings(rng, 300, 17, False), n_left=100, power=2, gamma=0.3))
    # complex white noise: the reference needs 2760 iterations (> 1000), tests/golden_inputs.py loadings_noconv
    r1 = np.random.default_rng(1)
    case("loadings/noconv", rotate_loadings(r1.standard_normal((1000, 20)) + 1j * r1.standard_normal((1000, 20)), n_left=1000, power=4))
    Z = loadings(rng, 300, 5, False)
    Z[17] = 0.0
    case("loadings/zero_row", rotate_loadings(Z, n_left=300))

    # MCA.rotate straight after solve(): the loadings are built on the device from the resident vectors (xmca_rotate_solved)
    left, right = coupled(rng, 96, 400, 260)

    def model(fields, complexify, n_rot, power, dtype=np.float64):
        def fn():
            m = MCA(*[f.astype(dtype) for f in fields], handle=h)
            m.solve(complexify=complexify)
            m.rotate(n_rot, power=power)
            return {"R": m._rotation_matrix, "Phi": m._correlation_matrix, "norm_left": m._norm["left"], "norm_right": m._norm["right"],
                    "n_iter": m._varimax_iterations}
        return fn

    case("model/one_f64", model((left,), False, 6, 2))
    case("model/one_f32", model((left,), False, 6, 2, np.float32))
    case("model/two_complex", model((left, right), True, 4, 2))
    case("model/two_complex_varimax", model((left, right), True, 5, 1))

    # replicate runners, rotated, two lanes
    def replicates(boot):
        def fn():
            m = MCA(left, right, handle=h)
            m.solve(complexify=False)
            m.rotate(4, power=2)
            if boot:
                np.random.seed(5)
                return {"boot": m.bootstrapping(4, n_modes=4, on_left=True, on_right=True)}
            return {"rule_n": m.rule_n(4, seed=7)}
        return fn

    case("replicates/rule_n", replicates(False))
    case("replicates/bootstrapping", replicates(True))
    giveups.close()


def run(lib, out):
    for sw in SWITCHES:
        d = os.path.join(out, switches_name(sw))
        os.makedirs(d, exist_ok=True)
        env = dict(os.environ, XMCA_TRACE="rot,giveup", XMCA_RULE_N_LANES="2", **sw)
        cmd = [sys.executable, os.path.abspath(__file__), "walk", "--out", d] + (["--lib", lib] if lib else [])
        p = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, text=True, timeout=600)
        with open(os.path.join(d, "trace.txt"), "w") as f:
            f.writelines(l + "\n" for l in p.stderr.splitlines() if l.startswith(("== case", "[xmca varimax]", "xmca: varimax")))
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


def moved_giveups(path):
    """cases of giveups.txt during which the counter moved"""
    moved = []
    for line in open(path):
        name, counts = line.rsplit(": ", 1)
        before, after = counts.split(" -> ")
        if int(before) != int(after):
            moved.append(name)
    return moved


EXPECTED_ERRORS = ("loadings__noconv__error.npy", "loadings__zero_row__error.npy")     # every other case must return


def compare(ref, repeat, cand, json_path):
    outputs, differ, text_differ, disturbed = [], [], [], []
    for sw in sorted(os.listdir(ref)):
        for d, who in ((ref, "reference"), (repeat, "repeat"), (cand, "candidate")):
            extra = set(os.listdir(os.path.join(d, sw))) ^ set(os.listdir(os.path.join(ref, sw)))
            if extra:
                differ.append("%s: file sets differ (%s)" % (sw, ", ".join(sorted(extra))))
            if "test_giveup" not in sw:
                disturbed += ["%s:%s (%s)" % (sw, c, who) for c in moved_giveups(os.path.join(d, sw, "giveups.txt"))]
        for name in sorted(os.listdir(os.path.join(ref, sw))):
            paths = [os.path.join(d, sw, name) for d in (ref, repeat, cand)]
            if not all(os.path.exists(p) for p in paths):
                continue                                  # (named above: the file sets differ)
            if name.endswith("__error.npy") and name not in EXPECTED_ERRORS:
                differ.append("%s:%s raises: %s" % (sw, name[:-4].replace("__", "/"), " ".join(np.load(paths[0]))))
            if name == "trace.txt":
                texts = [by_case(open(p).read()) for p in paths]
                if not (texts[0] == texts[1] == texts[2]):
                    text_differ.append(sw + ":" + name)
            elif name == "giveups.txt":
                if "test_giveup" in sw and not (open(paths[0]).read() == open(paths[1]).read() == open(paths[2]).read()):
                    text_differ.append(sw + ":" + name)
            else:
                a, b, c = (np.load(p) for p in paths)
                key = sw + ":" + name[:-4].replace("__", "/")
                outputs.append(key)
                if not (same(a, b) and same(a, c)):
                    differ.append(key + (" (the reference does not reproduce itself)" if not same(a, b) else ""))
    rec = {"n_arrays": len(outputs), "identical_in_all_three_runs": len(outputs) - len([d for d in differ if "file sets" not in d]),
           "differ": differ, "trace_or_giveup_files_that_differ": text_differ,
           "cases_during_which_the_giveup_counter_moved_outside_test_giveup": disturbed, "switch_sets": sorted(os.listdir(ref))}
    print(json.dumps(rec, indent=1))
    if json_path:
        with open(json_path, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if not differ and not text_differ else 1


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
