"""The Sturm and twisted-vector stage of the C2 step from a rocprofv3 --kernel-trace CSV of bench.py:

    python scripts/sturm_twist_trace.py <kernel_trace.csv> [label] [--steps K]

Over the last K steps (default 20: the timed ones): mean, smallest and largest duration of `trd_bisect_kernel` and
`trd_twisted_kernel`, and the span from the end of the last `trd_resident_kernel` link of a step to the start of the first
back-transformation GEMM (the first `gemm_kernel` behind `trd_twisted_kernel`).  Times in microseconds.  Steps are told apart as
scripts/lead_defer_trace_spans.py does it."""
import sys

from lead_defer_trace_spans import rows


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else path
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 20
    k = rows(path)
    trd = [i for i, r in enumerate(k) if "trd_resident_kernel" in r[2]]
    ends = [i for n, i in enumerate(trd) if n + 1 == len(trd) or k[trd[n + 1]][0] - k[i][1] > 2_000_000]
    starts = [trd[0]] + [trd[n + 1] for n, i in enumerate(trd[:-1]) if k[trd[n + 1]][0] - k[i][1] > 2_000_000]
    bis, tw, span = [], [], []
    for n in range(max(0, len(ends) - steps), len(ends)):
        t0 = k[ends[n]][1]
        t1 = k[starts[n + 1]][0] if n + 1 < len(starts) else t0 + 20_000_000
        win = [r for r in k[ends[n] + 1:] if r[0] < t1]
        b = [r for r in win if "trd_bisect_kernel" in r[2]]
        t = [r for r in win if "trd_twisted_kernel" in r[2]]
        if not b or not t:
            continue
        g = [r for r in win if "gemm_kernel" in r[2] and r[0] >= t[0][1]]
        bis.append((b[0][1] - b[0][0]) / 1000.0)
        tw.append((t[0][1] - t[0][0]) / 1000.0)
        if g:
            span.append((g[0][0] - t0) / 1000.0)
    fmt = lambda v: "mean %7.1f  min %7.1f  max %7.1f" % (sum(v) / len(v), min(v), max(v)) if v else "none"
    print("## %s: %d steps, us" % (label, len(bis)))
    print("  trd_bisect_kernel                                     %s" % fmt(bis))
    print("  trd_twisted_kernel                                    %s" % fmt(tw))
    print("  end of the reduction -> first back-transformation GEMM %s" % fmt(span))


if __name__ == "__main__":
    main()
