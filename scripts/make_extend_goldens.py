#!/usr/bin/env python3
"""Golden vectors of solve(complexify=True, extend='exp') from the REAL reference -> tests/golden/extend_exp_cases.npz.

Run (needs the reference checkout that oracle/make_goldens.py imports; no GPU):
    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python scripts/make_extend_goldens.py

Every case is stored under "<case>/<key>" keys: the inputs' description (name, rows, period), singular values, the leading
vectors and PCs (a per-mode phase is free: the tests align it), and where a case rotates the rotated variance and R; the two
bootstrap cases hold `bootstrapping(3, n_modes=4, ...)` of the reference under np.random.seed(5).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle.make_goldens import import_reference  # noqa: E402
from golden_inputs import GOLDEN_DIR, make_input  # noqa: E402

N_KEEP = 4

# name: (input, rows (None = all), fields kept (1 / 2), period, rotate (n_rot, power) or None)
SOLVE_CASES = {
    "wide_both": ("wide_both", None, 2, 12, None),
    "wide_left": ("wide_both", None, 1, 12, None),
    "small_both": ("small_both", None, 2, 12, None),
    "wide_odd": ("wide_both", 63, 2, 6, None),
    "sst_prcp_p1": ("sst_prcp", None, 2, 1, None),
    "sst_prcp_p6": ("sst_prcp", None, 2, 6, None),
    "sst_prcp_p12": ("sst_prcp", None, 2, 12, None),
    "wide_rot": ("wide_both", None, 2, 12, (4, 1)),
}

# name: (input, fields kept, period, rotate or None, bootstrapping keywords)
BOOT_CASES = {
    "boot_small": ("small_both", 2, 12, None, dict(on_left=True, on_right=True, block_size=2)),
    "boot_wide_rot": ("wide_both", 2, 12, (4, 1), dict(on_left=True, on_right=False, block_size=1)),
}


def case_fields(inp, rows, n_fields):
    fields = make_input(inp)[:n_fields]
    if rows is not None:
        fields = tuple(f[:rows] for f in fields)
    return fields


def solve_case(MCA, inp, rows, n_fields, period, rot):
    m = MCA(*case_fields(inp, rows, n_fields))
    m.solve(complexify=True, extend='exp', period=period)
    out = {"singular_values": np.asarray(m._singular_values[:N_KEEP]),
           "input": np.asarray(inp), "period": np.asarray(period), "rows": np.asarray(-1 if rows is None else rows), "n_fields": np.asarray(n_fields)}
    pcs = m.pcs(N_KEEP, rotated=False)
    for k in m._V:
        out["V_" + k] = m._V[k][:, :N_KEEP]
        out["pcs_" + k] = pcs[k]
    if rot:
        m.rotate(*rot)
        out["rot_variance"] = np.asarray(m._variance)
        out["R"] = np.asarray(m._rotation_matrix)
        out["rot"] = np.asarray(rot)
    return out


def boot_case(MCA, inp, n_fields, period, rot, kw):
    m = MCA(*case_fields(inp, None, n_fields))
    m.solve(complexify=True, extend='exp', period=period)
    if rot:
        m.rotate(*rot)
    np.random.seed(5)
    out = m.bootstrapping(3, n_modes=4, disable_progress=True, **kw)
    return np.asarray(out)


def main():
    MCA, _, _ = import_reference()
    out = {}
    for name, (inp, rows, n_fields, period, rot) in SOLVE_CASES.items():
        for key, val in solve_case(MCA, inp, rows, n_fields, period, rot).items():
            out[name + "/" + key] = val
        print("solve", name, out[name + "/singular_values"][:3], out[name + "/V_left"].dtype, flush=True)
    for name, (inp, n_fields, period, rot, kw) in BOOT_CASES.items():
        out[name + "/bootstrap"] = boot_case(MCA, inp, n_fields, period, rot, kw)
        out[name + "/input"] = np.asarray(inp)
        print("bootstrap", name, out[name + "/bootstrap"].shape, flush=True)
    dst = os.path.join(GOLDEN_DIR, "extend_exp_cases.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%.3f MB)" % (dst, os.path.getsize(dst) / 1e6))


if __name__ == "__main__":
    main()
