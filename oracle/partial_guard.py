"""Model of the guard at the cut of the partial eigenvector stage, written from DESIGN.md 2.10 (not from csrc/jacobi.h):

Of the n eigenvalues lam_1 >= ... >= lam_n the vectors of the k leading ones are wanted.  The set is extended to the first
k' >= k behind which BOTH rules hold for the gap g = lam_k' - lam_k'+1:

* absolute:  eps ||T|| / g <= (3/4) 0.3^2 = 0.0675, ||T|| the spectral norm, max(|lam_1|, |lam_n|);
* relative:  g / |lam_k'| > 1e-3.

At most 32 further vectors; a set of more than n / 4 vectors, or no such k' within the cap, means all n.  Bit-equal values - a
gap of at most 2.2e-16 ||T|| - among the leading k' + 1 (the set and its neighbour) send the solve to the Jacobi sweeps.

`margin` says how far the gaps behind an answer are from the thresholds they are compared with."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
LEAK = 0.75 * 0.3 ** 2          # what one Newton-Schulz step leaves of the largest defect the clean-up accepts
RELGAP = 1e-3
CAP = 32
REPEATED = 2.2e-16


def spectral_norm(lam):
    return max(abs(float(lam[0])), abs(float(lam[-1])))


def _clear_behind(lam, kp, norm):
    """both rules for a set of kp vectors: the cut lies between lam_kp and lam_kp+1 (1-based)"""
    gap = float(lam[kp - 1]) - float(lam[kp])
    if not gap > 0.0:
        return False
    absolute = EPS * norm / gap <= LEAK
    size = abs(float(lam[kp - 1]))
    relative = True if size == 0.0 else gap / size > RELGAP       # (a positive gap behind an exact zero is infinitely wide)
    return absolute and relative


def partial_count(lam, n_lead):
    """number of eigenvectors formed for n_lead wanted ones; lam: all eigenvalues, descending"""
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.size
    if n_lead < 1 or n_lead >= n:
        return n
    norm = spectral_norm(lam)
    kp = n_lead
    while kp <= n_lead + CAP and kp <= n - 1:
        if _clear_behind(lam, kp, norm):
            return kp if 4 * kp <= n else n
        kp += 1
    return n


def repeated_leading(lam, kp):
    """bit-equal eigenvalues among the leading kp + 1"""
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.size
    bound = REPEATED * spectral_norm(lam)
    return any(float(lam[i]) - float(lam[i + 1]) <= bound for i in range(min(kp, n - 1)))


def _factor(gap, thr):
    """how far a gap is from the threshold it is compared with, as a factor >= 1"""
    if gap > 0.0 and thr > 0.0:
        return max(gap / thr, thr / gap)
    return 1.0 if gap <= 0.0 and thr <= 0.0 else np.inf       # (zero against zero sits on the threshold)


def margin(lam, n_lead, full_route=False, exact_ties=False):
    """The smallest factor by which the thresholds could move before partial_count(lam, n_lead) or repeated_leading(lam, that
    count) changes: every cut the guard inspects is either clear with both rules that far inside, or closed with at least one
    rule that far outside ('relative': 1e-3 |lam_k|, 'absolute': eps ||A|| / 0.0675), and the `repeated` test has either one gap
    that far below 2.2e-16 ||A|| or every gap that far above it.  A request for more than n / 4 vectors gives n whatever the gaps are: no cut counts.
    full_route: where all n vectors are formed, the `repeated` test of the full stage - every gap of the spectrum - counts too.
    exact_ties: lam is the spectrum by construction.  Computed eigenvalues carry errors of the size of the `repeated` bound
    itself, so a tie among them may be gone in another solver's: it counts as a margin of 1 unless the values are exact."""
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.size
    norm = spectral_norm(lam)
    kp = partial_count(lam, n_lead)
    worst = np.inf
    if 1 <= n_lead < n and 4 * n_lead <= n:
        for k in range(n_lead, min(n_lead + CAP, n - 1) + 1):
            gap = float(lam[k - 1]) - float(lam[k])
            rel = (gap > RELGAP * abs(float(lam[k - 1])), _factor(gap, RELGAP * abs(float(lam[k - 1]))))
            ab = (EPS * norm <= LEAK * gap, _factor(gap, EPS * norm / LEAK))
            if rel[0] and ab[0]:
                worst = min(worst, rel[1], ab[1])
                break                                          # (the first clear cut ends the search)
            worst = min(worst, max(f for ok, f in (rel, ab) if not ok))
    if kp < n or full_route:
        # one bit-equal pair decides the test however close the other gaps are; none: every gap has to stay clear of the bound
        hit, miss = 0.0, np.inf
        for i in range(min(kp, n - 1)):
            gap, f = float(lam[i]) - float(lam[i + 1]), _factor(float(lam[i]) - float(lam[i + 1]), REPEATED * norm)
            if gap <= REPEATED * norm:
                hit = max(hit, f)
            else:
                miss = min(miss, f)
        worst = min(worst, (hit if exact_ties else 1.0) if hit > 0.0 else miss)
    return worst
