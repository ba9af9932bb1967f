#!/usr/bin/env python3
"""Accuracy of `solve(n_modes=k)` on the planted inputs of tests/test_gpu_partial_solve.py, written to
profiles/partial_solve_accuracy.json: per case and k, the error of the FULL solve against oracle/ref_numpy.py (float64 SVD)
on phase-aligned eofs(k) / pcs(k), the difference between the partial and the full solve on the same quantities, the
orthonormality defect max |V^H V - I| of the k vectors of either, the eigenvectors each solve formed and whether the values
of the two agree to the bit.  The tests allow the partial solve 4 x the full solve's error (never less than the tolerance of
the config tests for the dtype); this file is what those bounds looked like when it was written."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import partial_solve_cases as cases                         # noqa: E402
from partial_solve_cases import mode_error, orth_defect    # noqa: E402
from xmca_amd import _hip                                   # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "partial_solve_accuracy.json")
    hip = _hip.default_handle(0)
    rows = []
    for name, case in cases.ALL_CASES.items():
        for k in case[5]:
            r = cases.run_case(hip, name, k)
            row = {"case": name, "T": r["T"], "N": list(r["Ns"]), "complexify": r["cplx"], "dtype": str(r["dtype"]), "k": k,
                   "n_eigvec_full": r["full_info"][0]["n_eigvec"], "n_eigvec_partial": r["part_info"][0]["n_eigvec"],
                   "full_by_tridiagonal_route": bool(r["full_info"][0]["tridiag"]),
                   "values_bit_equal": bool(np.array_equal(r["part_state"]["singular_values"], r["full_state"]["singular_values"])),
                   "result_kib_full": r["full_result"]["vector_kib"], "result_kib_partial": r["part_result"]["vector_kib"]}
            for key in r["keys"]:
                for what in ("eofs", "pcs"):
                    row["%s_%s_full_vs_oracle" % (what, key)] = mode_error(np.asarray(r["full_" + what][key]), r["oracle_" + what][key])
                    row["%s_%s_partial_vs_full" % (what, key)] = mode_error(np.asarray(r["part_" + what][key]), np.asarray(r["full_" + what][key]))
                row["orth_%s_full" % key] = orth_defect(r["full_eofs"][key])
                row["orth_%s_partial" % key] = orth_defect(r["part_eofs"][key])
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        json.dump({"case": "solve(n_modes=k) against solve() and the float64 oracle, planted inputs (tests/partial_solve_cases.py)",
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
