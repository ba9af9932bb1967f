"""The restated Theta extension (tests/theta_cases.py) against statsmodels itself, where it is installed - the one
check of the restatement against the package the reference calls (xmca/array.py:367-376).  Skipped without statsmodels.

alpha is not compared: statsmodels finds it with an iterative optimiser.  The forecast at statsmodels' own alpha is deterministic
arithmetic and must agree to 1e-10 relative; and the grid zoom must not find a worse alpha than the optimiser did."""
import numpy as np
import pytest

import theta_cases as tc

pytest.importorskip("statsmodels")


@pytest.mark.parametrize("T,m", [(24, 12), (25, 4), (37, 5), (48, 1), (9, 4)])
def test_restatement_agrees_with_statsmodels(T, m):
    from statsmodels.tsa.forecasting.theta import ThetaModel
    X = tc.columns(T, 12, m, seed=7 * T + m)
    ours = tc.fit(X, m)
    Z = tc.deseasonalised(X, m)
    for c in range(X.shape[1]):
        if not np.any(X[:, c]):
            continue                                   # (statsmodels does not fit a constant series)
        res = ThetaModel(X[:, c], period=m, deseasonalize=True, use_test=False).fit()
        theirs = np.asarray(res.forecast(steps=T, theta=20))
        alpha = float(res.params["alpha"])
        at_theirs = tc.fit(X[:, c:c + 1], m, alpha=np.array([alpha]))
        mine = tc.forecast(at_theirs, T, m)[:, 0]
        assert np.abs(mine - theirs).max() <= 1e-10 * np.abs(theirs).max(), (T, m, c)
        sse_theirs = tc.smooth(Z[:, c:c + 1], np.array([alpha]))[0][0]
        assert ours["sse"][c] <= sse_theirs * (1 + 1e-12), (T, m, c)
