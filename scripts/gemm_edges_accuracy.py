"""Room under the bars of the GEMM edge tests (tests/test_gpu_gemm_edges.py) -> profiles/gemm_edges_accuracy.json

    python scripts/gemm_edges_accuracy.py                      # CPU only: the model's figures for the X3 shapes
    python scripts/gemm_edges_accuracy.py --device             # + runs the test file on an MI355X and records its figures
    python scripts/gemm_edges_accuracy.py --figures FILE       # + figures a run of the test file left (XMCA_GEMM_EDGES_RECORD=FILE)

CPU part: for every X3 shape of oracle/bf16x3_model.py and the piece-revealing operands, error over max(|A| @ |B|) of the
six-term product with exact sums and with float32 sums of 16 and of 8 products at a time, and of each mutation (a term left out, al paired with bl).
Device part: the largest error over scale per group of tests and operand type, as the tests measured it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import bf16x3_model as X   # noqa: E402


def model_figures():
    out = {}
    for shape, gram in [(s, False) for s in X.X3_SHAPES] + [(s, True) for s in X.X3_GRAM_SHAPES]:
        A, B = X.x3_operands(shape, gram)
        row = {"six_terms_exact_sums": X.error(X.x3_product(A, B), A, B),
               "six_terms_float32_sums_of_16": X.error(X.x3_product(A, B, group=16), A, B),
               "six_terms_float32_sums_of_8_as_the_device": X.error(X.x3_product(A, B, group=X.MFMA_GROUP), A, B)}
        for name, terms in X.MUTATIONS.items():
            row[name] = X.error(X.x3_product(A, B, terms), A, B)
        out[X.case_id(shape, gram)] = row
        print("%-18s " % X.case_id(shape, gram) + "  ".join("%s %.2e" % kv for kv in row.items()), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--figures")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gemm_edges_accuracy.json"))
    args = ap.parse_args()
    doc = {"case": "csrc/gemm.h at its staging, slice, split-K and epilogue edges against float64 products of the same operands",
           "source": "scripts/gemm_edges_accuracy.py; asserted by tests/test_gpu_gemm_edges.py and tests/test_bf16x3_model.py",
           "measure": "max |C - ref| / max(|A| @ |B|), times the scales of the epilogue; float32_slices_rel_to_result: over max |ref|; "
                      "float32_result_ulps: float32 units in the last place",
           "bars": {"float64": 1e-13, "float32": X.BAR, "float32_slices_rel_to_result": 5e-7, "x3_against_plain_f32_path": 1e-6,
                    "float32_result_ulps": 1.0},
           "cpu_model_x3_shapes": model_figures()}
    figures = args.figures
    rc = 0
    if args.device:
        figures = os.path.join(tempfile.mkdtemp(), "figures.json")
        rc = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_gpu_gemm_edges.py"), "-q"],
                            env=dict(os.environ, XMCA_GEMM_EDGES_RECORD=figures)).returncode
    if figures:
        with open(figures) as f:
            flat = json.load(f)
        dev = {}
        for key, v in sorted(flat.items()):
            group, dtype = key.split("/")
            dev.setdefault(group, {})[dtype] = v
        doc["mi355x_largest_error_over_scale"] = dev
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
