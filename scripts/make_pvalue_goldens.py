"""Truth for the p-value kernel (xmca_pearson_pvalues): tests/golden/pvalue_truth.npz.

    python scripts/make_pvalue_goldens.py

p = 2 I_x(a, a), a = n_obs / 2 - 1, x = (1 - |r|) / 2, from mpmath at 60 digits (the incomplete beta integral by its
hypergeometric series; a second evaluation at 90 digits must agree to 1e-30), rounded to double.  Per n_obs about 100 values of
r: uniform in (0, 1), 1 - 10^-k (k = 2..15), 10^-k (k = 1..12), both signs, each taken as the double it is stored as.

  main group   n_obs, r, p          truth >= 1e-290: what the accuracy bound of tests/test_gpu_patterns.py is checked on
  tail group   tail_n_obs, tail_r, tail_p   truth < 1e-290 (down to an exact 0 in double)
  log_norm_n_obs, log_norm          -ln a - ln B(a, a) per n_obs, the constant the host passes to the kernel

Before the file is written, scipy.special.betainc - the function behind the reference's `pearsonr` - is checked against the
truth on the main group: within the kernel's bound plus scipy's own error (1e-12 relative for p >= 1e-250, 1e-8 below).
Needs mpmath; the tests only read the file."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "pvalue_truth.npz")
N_OBS = [3, 4, 5, 8, 60, 300, 1200, 2920, 5000]
TAIL_BELOW = 1e-290


def bound(a, r, p):
    """64 eps (1 + a |ln(x (1 - x))|) p: the absolute error allowed at truth p (issue: the error of exp(L) is that of L)"""
    x = (1.0 - np.abs(r)) / 2
    return 64 * 2.0 ** -52 * (1 + a * np.abs(np.log(x) + np.log1p(-x))) * p


def r_values(rng):
    u = rng.uniform(0.0, 1.0, 24)
    near_one = 1.0 - 10.0 ** -np.arange(2, 16)
    near_zero = 10.0 ** -np.arange(1, 13)
    r = np.concatenate([u, near_one, near_zero])
    return np.concatenate([r, -r])


def truth(mp, r, n_obs, dps):
    mp.mp.dps = dps
    a = mp.mpf(n_obs) / 2 - 1
    x = (1 - abs(mp.mpf(float(r)))) / 2
    return 2 * mp.betainc(a, a, 0, x, regularized=True)


def main():
    import mpmath as mp
    import scipy.special
    rng = np.random.default_rng(20261016)
    main_rows, tail_rows, norms = [], [], []
    for n_obs in N_OBS:
        mp.mp.dps = 60
        a = mp.mpf(n_obs) / 2 - 1
        norms.append(float(-mp.log(a) - mp.log(mp.beta(a, a))))
        for r in r_values(rng):
            t = truth(mp, r, n_obs, 60)
            t2 = truth(mp, r, n_obs, 90)
            assert t2 == 0 or abs(t - t2) <= mp.mpf(10) ** -30 * t2, (n_obs, r)
            row = (n_obs, float(r), float(t))
            (main_rows if t >= TAIL_BELOW else tail_rows).append(row)
        print("n_obs %5d: main %3d, tail %3d" % (n_obs, sum(m[0] == n_obs for m in main_rows), sum(m[0] == n_obs for m in tail_rows)),
              flush=True)
    n, r, p = (np.array(c) for c in zip(*main_rows))
    tn, tr, tp = (np.array(c) for c in zip(*tail_rows))
    a = n / 2 - 1
    ref = 2 * scipy.special.betainc(a, a, (1.0 - np.abs(r)) / 2)
    allow = bound(a, r, p) + np.where(p >= 1e-250, 1e-12, 1e-8) * p
    worst = np.max(np.abs(ref - p) / allow)
    print("scipy.special.betainc against the truth: worst error / allowance = %.3g" % worst)
    assert worst <= 1.0, "scipy disagrees with the truth"
    np.savez_compressed(OUT, n_obs=n.astype(np.int64), r=r, p=p, tail_n_obs=tn.astype(np.int64), tail_r=tr, tail_p=tp,
                        log_norm_n_obs=np.array(N_OBS, dtype=np.int64), log_norm=np.array(norms))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
