"""Reference noise and device bound of the Promax tail tests (tests/test_gpu_promax_edges.py) -> profiles/promax_tail_accuracy.json

    python scripts/promax_tail_accuracy.py                  # CPU only: stop margins, conditioning, reference noise, bound
    python scripts/promax_tail_accuracy.py --device         # + the largest device deviation per case (needs an MI355X)
    python scripts/promax_tail_accuracy.py --out FILE

CPU part (no GPU needed).  For every case of oracle/promax_edges.py:
  * the oracle's stopping ratio at the stop iteration (<= 0.7 tol) and one iteration earlier (>= 1.3 tol): the tests assert the
    iteration count for equality;
  * the tail of ref_numpy.promax from the oracle's Varimax result, once in float64 and once with the four N-sized sums and the
    column maxima in np.longdouble: the largest relative difference of R, Phi, B, norm_left, norm_right is the reference's own
    noise.  Device bound = 100 x the largest noise over the cases, at least 1e-13, and no case may push it beyond 1e-10.
The script exits with status 1 if a case misses its stop margin or the conditioning cap.

Device part: the tail recomputed in float64 from the device's own Varimax result against the full device call."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import promax_edges as E   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "promax_tail_accuracy.json"))
    args = ap.parse_args()

    cases = [(c, E.edge_loadings) for c in E.CASES] + [(E.SLOW_CASE, E.wide_loadings)]
    per_case, worst, ok = {}, 0.0, True
    refs = {}
    for case, gen in cases:
        ref = refs[case] = E.oracle_case(case, gen)
        at, before = E.stop_margin(ref["ratios"])
        noise, cond = E.tail_noise(ref["Bv"], ref["Rv"], case[3], case[4])
        in_bound = gen is E.edge_loadings            # the slow input is no case of the tail comparison
        if in_bound:
            worst = max(worst, noise)
        clear = E.stop_is_clear(ref["ratios"])
        ok = ok and clear
        h = np.sqrt(np.sum(np.abs(ref["A"]) ** 2, axis=1))
        per_case[E.case_id(case)] = {"seed": case[5], "inputs": gen.__name__, "varimax_iterations": ref["n_iter"],
                                     "stop_ratio_over_tol": at, "previous_ratio_over_tol": before, "stop_margin_ok": clear,
                                     "cond_XhX": cond, "smallest_row_norm": float(h.min()), "reference_noise": noise,
                                     "in_bound": in_bound}
        print("%-28s %3d iterations  stop %.3f tol  before %.3f tol  cond %.2f  noise %.2e%s" %
              (E.case_id(case), ref["n_iter"], at, before, cond, noise, "" if clear else "   <- stop margin missed"), flush=True)
    bound = E.tail_bound(worst)
    print("largest reference noise %.3e -> device bound %s" % (worst, "none: above the cap of %g" % E.TAIL_CAP if bound is None else "%.3e" % bound))
    ok = ok and bound is not None
    doc = {"case": "Promax tail of the fused rotation routes (rot_accum_kernel MODE 2 / 3, rot_reduce_partials_kernel, finish_promax) "
                   "against the tail of oracle/ref_numpy.promax evaluated on the device's own Varimax result",
           "source": "scripts/promax_tail_accuracy.py; asserted by tests/test_gpu_promax_edges.py",
           "measure": "max |a - b| / max |b| over R, Phi, B, norm_left, norm_right",
           "reference_noise": "float64 tail vs. tail with X^H X, X^H P, both block Grams and the column maxima in np.longdouble (CPU)",
           "largest_reference_noise": worst, "margin": E.TAIL_MARGIN, "floor": E.TAIL_FLOOR, "cap": E.TAIL_CAP,
           "device_bound": bound, "stop_tolerance": E.TOL_STOP, "per_case": per_case}

    if args.device:
        from xmca_amd import _hip
        hip = _hip.default_handle(0)
        worst_dev = 0.0
        for case, gen in cases:
            n, p, cplx, power, n_left, _ = case
            A = refs[case]["A"]
            full = hip.rotate_loadings(A, n_left, power, tol=E.TOL_STOP, want_B=True)
            v = hip.rotate_loadings(A, n_left, varimax_only=True, want_B=True)
            tail = E.promax_tail(v["B"], v["R"], power, n_left)
            errs = {k: E.rel(full[k], tail[i]) for i, k in enumerate(E.TAIL_NAMES)}
            full_errs = {k: E.rel(full[k], refs[case][k]) for k in E.TAIL_NAMES}
            dev = max(errs.values())
            worst_dev = max(worst_dev, dev)
            per_case[E.case_id(case)].update({"device_iterations": full["n_iter"], "device_tail_deviation": dev,
                                              "device_tail_deviation_by_output": errs, "device_full_path_deviation": full_errs})
            print("%-28s device: %3d iterations  tail %.2e  full path %.2e" % (E.case_id(case), full["n_iter"], dev, max(full_errs.values())),
                  flush=True)
        doc["largest_device_tail_deviation"] = worst_dev
        doc["library_version"] = hip._lib.xmca_version().decode()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
