"""Goldens of `bootstrapping(axis=1)`: the REAL reference's `MCA.bootstrapping(3, n_modes=4, axis=1, ...)` under `np.random.seed(5)`
(xmca/array.py:1813-1952, tools/array.py:91-138) for the cases of tests/test_gpu_bootstrap_columns.py
-> tests/golden/bootstrap_columns_cases.npz (one 4 x 3 float64 array per case).

    python scripts/make_bootstrap_columns_goldens.py

Needs the reference checkout that oracle/make_goldens.py imports; the tests read only the .npz.  Every case must complete
without a dropped run (a dropped run is a zero column) - the script refuses to write otherwise.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from golden_inputs import GOLDEN_DIR, make_input  # noqa: E402

# tag, input, single field, solve kwargs, rotation, bootstrapping kwargs  (keep in sync with tests/test_gpu_bootstrap_columns.py)
CASES = [
    ("small_b2", "small_both", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=2)),
    ("small_b3_seam", "small_both", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=3)),
    ("wide_rot_left", "wide_both", False, dict(complexify=False), (5, 2), dict(on_left=True, on_right=False, block_size=1)),
    ("wide_single_cplx", "wide_both", True, dict(complexify=True), None,
     dict(on_left=True, on_right=False, block_size=4, replace=False)),
    ("wide_cplx_rot_right", "wide_both", False, dict(complexify=True), (4, 1), dict(on_left=False, on_right=True, block_size=1)),
    ("mixed_b5", "mixed_both", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=5)),
    ("mixed_cplx_rot_both", "mixed_both", False, dict(complexify=True), (4, 1), dict(on_left=True, on_right=True, block_size=1)),
    ("wide_f32_both", "wide_both_f32", False, dict(complexify=False), None, dict(on_left=True, on_right=True, block_size=1)),
    ("wide_exp_left", "wide_both", False, dict(complexify=True, extend='exp', period=12), None,
     dict(on_left=True, on_right=False, block_size=1)),
    ("sst_iterative", "sst_prcp", False, dict(complexify=False), None,
     dict(on_left=True, on_right=True, block_size=1, strategy='iterative')),
]


def reference_case(MCA, inp, single, solve_kw, rot, kw):
    fields = make_input(inp)
    if single:
        fields = fields[:1]
    m = MCA(*fields)
    m.solve(**solve_kw)
    if rot:
        m.rotate(*rot)
    np.random.seed(5)
    return m.bootstrapping(3, n_modes=4, axis=1, disable_progress=True, **kw)


def main():
    from oracle.make_goldens import import_reference
    MCA, _, _ = import_reference()
    out = {}
    for tag, inp, single, solve_kw, rot, kw in CASES:
        out[tag] = np.asarray(reference_case(MCA, inp, single, solve_kw, rot, kw), dtype=np.float64)
        assert out[tag].shape == (4, 3) and np.all(out[tag] != 0.0), (tag, out[tag])      # no dropped run
        print(tag, out[tag].shape, "max %.6g" % np.abs(out[tag]).max())
    dst = os.path.join(GOLDEN_DIR, "bootstrap_columns_cases.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%d bytes)" % (dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
