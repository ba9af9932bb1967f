"""SHA-256 of what `Handle.tridiag_vectors` returns on every vector case of tests/tridiag_stage_cases.py, on one partial call
(nev < n, padded ldy) and on one large order with twist indices on both sides of the hand-over row of `trd_twisted_kernel`
(n = 1500, a permuted ramp with e = 0.01: every vector sits at the row of its own diagonal entry).  Run on two builds on the same
machine and combined, the two lists say whether a change to the kernel that only moves its loads keeps the bits of the planes
(used for the two variants recorded in DESIGN.md 9; neither is in the source).

    python scripts/sturm_twist_bits.py --root TREE --out list.json       # TREE: the checkout whose xmca_amd is loaded (default: this one)
    python scripts/sturm_twist_bits.py --combine parent.json this.json --out both.json
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def large_case():
    n = 1500
    d = np.random.default_rng(1500).permutation(np.arange(1.0, n + 1.0))
    e = np.full(n - 1, 0.01)
    lam = np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
    return d, e, np.sort(lam)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def hashes(root):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, root)
    import tridiag_stage_cases as C
    from xmca_amd import _hip
    h = _hip.Handle(0)
    out = {}
    for name in C.names(vectors=True):
        c = C.case(name)
        out[name] = digest(h.tridiag_vectors(c.d, c.e, C.lam_for_vectors(name)))
    c = C.case("random_n130")
    plane = np.random.default_rng(65).standard_normal((c.n, 70))
    out["random_n130_partial_nev65_ldy70"] = digest(h.tridiag_vectors(c.d, c.e, C.lam_for_vectors(c.name)[c.n - 65:], out=plane))
    d, e, lam = large_case()
    Y = h.tridiag_vectors(d, e, lam)
    twist = np.argmax(np.abs(Y), axis=0)                         # (the row of the largest component: where the vector sits)
    out["permuted_ramp_n1500_e_0.01"] = digest(Y)
    out["permuted_ramp_n1500_e_0.01_input"] = digest(np.concatenate((d, e, lam)))
    h = ((1500 // 2 + 32) // 64) * 64                            # a multiple of the 64-row chunk next to n / 2
    return out, {"n": 1500, "hand_over_row": h, "vectors_sitting_below_it": int(np.count_nonzero(twist < h)),
                 "vectors_sitting_from_it_on": int(np.count_nonzero(twist >= h))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=REPO)
    ap.add_argument("--combine", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        parent, this = (json.load(open(p)) for p in args.combine)
        doc = {"what": "sha256 of the float64 planes Handle.tridiag_vectors returns, parent commit and this build in one visit",
               "large_case": this["large_case"], "parent": parent["hashes"], "this": this["hashes"],
               "differing": sorted(k for k in set(parent["hashes"]) | set(this["hashes"]) if parent["hashes"].get(k) != this["hashes"].get(k))}
    else:
        hs, large = hashes(os.path.abspath(args.root))
        doc = {"hashes": hs, "large_case": large}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc.get("differing", sorted(doc.get("hashes", {}))), indent=None))


if __name__ == "__main__":
    main()
