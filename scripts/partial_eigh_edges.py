"""Figures behind the bars of tests/test_gpu_partial_eigh.py -> profiles/partial_eigh_edges.json (needs an MI355X)

    python scripts/partial_eigh_edges.py [--out FILE]

Per case of tests/partial_eigh_cases.py, on the same matrix: the call with n_lead (route, eigenvalue / orthonormality /
residual / projector / single-vector figures as the test measures them), the call without n_lead cut to the same k columns
(the full stage, or the sweeps where it hands over), and LAPACK's own figures - orthonormality and residual of
numpy.linalg.eigh, and its eigenvalue error against the spectrum the matrix was built from where the case states one."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import partial_eigh_cases as E   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "partial_eigh_edges.json"))
    args = ap.parse_args()
    from xmca_amd import _hip
    hip = _hip.default_handle(0)
    full, out = {}, {}
    for case in E.CASES:
        if case.vec_min_n is None:
            os.environ.pop("XMCA_TRIDIAG_VEC_MIN_N", None)
        else:
            os.environ["XMCA_TRIDIAG_VEC_MIN_N"] = case.vec_min_n
        A = E.matrix(case)
        lam_ref, U_ref, res_ref = E.reference(case)
        nrm = float(np.max(np.abs(lam_ref)))
        k = case.k
        lam, U = hip.eigh(A, n_lead=k)
        info = dict(hip.last_eigh_info)
        row = {"n": int(A.shape[0]), "k": k, "complex": bool(np.iscomplexobj(A)), "hard": case.hard, "route_free": case.route_free,
               "bars": list(E.bars(case)), "lead": dict(E.measure(A, lam_ref, U_ref, res_ref, lam, U, case.hard), tridiag=info["tridiag"],
                                                        n_eigvec=info["n_eigvec"], guard_rows_clean=info["guard_rows_clean"])}
        if case.matrix not in full:
            full[case.matrix] = hip.eigh(A) + (hip.last_eigh_info["tridiag"],)
        lam_f, U_f, tri_f = full[case.matrix]
        row["full"] = dict(E.measure(A, lam_ref, U_ref, res_ref, lam_f, U_f[:, :k], case.hard), tridiag=tri_f)
        Vk = U_ref[:, :k]
        row["lapack"] = {"orth": float(np.max(np.abs(Vk.conj().T @ Vk - np.eye(k)))), "res": res_ref}
        if case.spectrum is not None:
            row["lapack"]["eig"] = float(np.max(np.abs(lam_ref - case.spectrum)) / nrm)
        out[case.name] = row
        print(case.name, json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
