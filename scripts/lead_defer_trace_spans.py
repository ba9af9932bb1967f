"""Spans of the C2 step behind the tridiagonal reduction, from a rocprofv3 --kernel-trace CSV of bench.py:

    python scripts/lead_defer_trace_spans.py <kernel_trace.csv> [label]

Per step (the last `--last` ones): from the end of the last trd_resident_kernel link to the start of varimax_moment_kernel, to
the end of the back-projection (the longest gemm_kernel launch behind the reduction) and to the end of the rotation loop; and
the span from the first gemm_kernel behind the reduction (the back-transformation) to the start of the S = Z^H Z product's
successor trd_orth_kernel.  Times in microseconds."""
import csv
import sys


def rows(path):
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            out.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    out.sort()
    return out


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else path
    last = 3
    k = rows(path)
    trd = [i for i, r in enumerate(k) if "trd_resident_kernel" in r[2]]
    # a chain of links ends where the next link is more than 2 ms away
    ends = [i for n, i in enumerate(trd) if n + 1 == len(trd) or k[trd[n + 1]][0] - k[i][1] > 2_000_000]
    starts = [trd[0]] + [trd[n + 1] for n, i in enumerate(trd[:-1]) if k[trd[n + 1]][0] - k[i][1] > 2_000_000]
    print("## %s: last %d steps; us from the end of the last trd_resident_kernel link" % (label, last))
    for n in range(max(0, len(ends) - last), len(ends)):
        t0 = k[ends[n]][1]
        t1 = k[starts[n + 1]][0] if n + 1 < len(starts) else t0 + 20_000_000
        win = [r for r in k[ends[n] + 1:] if r[0] < t1]
        vm = [r for r in win if "varimax_moment_kernel" in r[2]]
        orth = [r for r in win if "trd_orth_kernel" in r[2]]
        gemm = [r for r in win if "gemm_kernel" in r[2] and (not vm or r[0] < vm[0][1])]
        lead = [r for r in win if "lead_rows_kernel" in r[2]]
        tw = [r for r in win if "trd_twisted_kernel" in r[2]]
        if tw:                                   # (the compact-WY factors run beside the Sturm and twisted kernels: not the back-transformation)
            gemm = [r for r in gemm if r[0] >= tw[0][1]]
        if not vm or not gemm or not orth:
            continue
        bp = max(gemm, key=lambda r: r[1] - r[0])
        us = lambda t: (t - t0) / 1000.0
        print("  varimax_moment_kernel start %8.1f  end %8.1f | back-projection gemm start %8.1f end %8.1f (%.1f) | "
              "back-transformation first gemm start %8.1f -> trd_orth_kernel start %8.1f (%.1f)%s"
              % (us(vm[0][0]), us(vm[0][1]), us(bp[0]), us(bp[1]), (bp[1] - bp[0]) / 1000.0, us(gemm[0][0]), us(orth[0][0]),
                 (orth[0][0] - gemm[0][0]) / 1000.0,
                 "".join(" | lead_rows %.1f" % ((r[1] - r[0]) / 1000.0) for r in lead)))
        if "--list" in sys.argv and n + 1 == len(ends):          # every launch of the last step behind the reduction
            for r in win:
                print("    %9.1f %9.1f %8.1f  %s" % (us(r[0]), us(r[1]), (r[1] - r[0]) / 1000.0, r[2][:90]))


if __name__ == "__main__":
    main()
