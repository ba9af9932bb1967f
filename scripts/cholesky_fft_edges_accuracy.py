"""Room under the bars of the Cholesky / FFT edge tests (tests/test_gpu_cholesky_fft_edges.py) -> profiles/cholesky_fft_edges_accuracy.json

    python scripts/cholesky_fft_edges_accuracy.py                  # CPU only: the reference and model figures
    python scripts/cholesky_fft_edges_accuracy.py --device         # + runs the test file on an MI355X and records its figures
    python scripts/cholesky_fft_edges_accuracy.py --figures FILE   # + figures a run of the test file left (XMCA_CHOL_FFT_EDGES_RECORD=FILE)

CPU part: the Cholesky sizes and the edges they reach at 256 compute units; the backward error of numpy.linalg.cholesky on the
Wishart and graded inputs at those sizes; per FFT length the error of the float64 Stockham model and of pocketfft against the
long-double transform, and what a root of radix 7 wrong in its 13th digit costs.  Device part: per group of tests the largest
device figure, the reference figure and the bar, as the tests measured and derived them."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import kernel_edges as K   # noqa: E402


def cholesky_figures(cus=256):
    plan = K.cholesky_sizes(cus)
    out = {"compute_units": cus, "sizes": plan["sizes"], "edges": plan["edges"], "skipped": plan["skipped"], "lapack_backward_error": {}}
    for cplx in (False, True):
        for kind, make in (("wishart", K.wishart), ("graded", K.graded)):
            worst = 0.0
            for n in plan["sizes"]:
                A = make(n, cplx)
                worst = max(worst, K.chol_backward_error(K.lapack_upper(A), A))
            out["lapack_backward_error"]["%s/%s" % (kind, "complex" if cplx else "real")] = worst
            print("cholesky %s %s: lapack %.2e" % (kind, "complex" if cplx else "real", worst), flush=True)
    return out


def fft_figures():
    rc, rs = K.FFT_ROOTS[7]
    wrong = dict(K.FFT_ROOTS)
    wrong[7] = (rc, (rs[0], 0.78183148246812980871) + rs[2:])
    out = {}
    for n in sorted(set(K.FFT_LENGTHS)):
        row = {"stockham_model": 0.0, "pocketfft": 0.0, "present_bar": K.fft_present_bar(n)}
        for cplx in (True, False):
            for sign in (-1, 1):
                x = K.fft_input(3, n, cplx)
                truth = K.fft_truth(x, sign)
                ref = np.fft.fft(x) if sign < 0 else np.conj(np.fft.fft(np.conj(x)))
                row["stockham_model"] = max(row["stockham_model"], K.fft_error(K.stockham(x, sign), truth))
                row["pocketfft"] = max(row["pocketfft"], K.fft_error(ref, truth))
                if 7 in K.fft_plan(n):
                    row["root_of_7_wrong_in_13th_digit"] = max(row.get("root_of_7_wrong_in_13th_digit", 0.0),
                                                               K.fft_error(K.stockham(x, sign, roots=wrong), truth))
        row["model_over_pocketfft"] = row["stockham_model"] / row["pocketfft"]
        out[str(n)] = row
        print("fft %5d " % n + "  ".join("%s %.2e" % kv for kv in row.items()), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--figures")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cholesky_fft_edges_accuracy.json"))
    args = ap.parse_args()
    doc = {"case": "csrc/cholesky.h, csrc/chol64.h and csrc/fft.h at their panel, slice, stride and option edges; the analytic frame above them",
           "source": "scripts/cholesky_fft_edges_accuracy.py; asserted by tests/test_gpu_cholesky_fft_edges.py and tests/test_kernel_edges_oracle.py",
           "measure": "cholesky: max |R^H R - A| / max diag(A) (forward: max |R - R_lapack| / max |R_lapack|); fft: max |y - truth| / max |truth|, "
                      "truth = scipy.fft on long double; analytic: relative error of sigma, max |v - v_ref| / max |v_ref| of the separated modes",
           "bars": {"cholesky_backward": "min(1e-13, 10 x largest lapack figure of the real / complex group)", "cholesky_forward": 1e-11,
                    "fft": "min(3 x max(stockham model, pocketfft) on the same input, 1e-13 sqrt(n) log2(n + 1))",
                    "analytic_sigma": 1e-10, "analytic_vectors": 1e-8},
           "cpu_cholesky": cholesky_figures(), "cpu_fft": fft_figures()}
    figures = args.figures
    rc = 0
    if args.device:
        figures = os.path.join(tempfile.mkdtemp(), "figures.json")
        rc = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_gpu_cholesky_fft_edges.py"), "-q"],
                            env=dict(os.environ, XMCA_CHOL_FFT_EDGES_RECORD=figures)).returncode
    if figures:
        with open(figures) as f:
            flat = json.load(f)
        dev = {}
        for key, v in sorted(flat.items()):
            group, _, case = key.partition("/")
            dev.setdefault(group, {})[case] = v
        doc["mi355x_device_reference_bar"] = dev
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
