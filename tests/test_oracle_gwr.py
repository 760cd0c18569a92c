"""The fp64 oracle's GWR series (orc_gwr_hat: predictor columns centred and scaled, Cholesky) against the 40-digit arbiter
(oracle/arbiter.py gwr_hat: the reference's raw 6 x 6 X'WX, lu_solve) at EVERY bandwidth ka = 6 .. 152 -- the distance e_k
that tests/test_gpu_gwr_matrix.py sets its per-bandwidth bar by.

Measured (golden case, one cell per ka, month 1 + i % 12, pt_norm = 0; max |oracle - arbiter| over the month's days):
Tmin 6.9e-13 degC, worst at ka = 8, 1.4e-14 from ka = 10 up; Tmax (lst_day) 2.0e-13, worst at ka = 12.  The oracle
succeeds (rc == 0) at every ka."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

import gwr_cases as gc  # noqa: E402

F64_BAR = 1e-10                                              # degC: fp64 arithmetic against 40 digits (test_gpu_kernel_matrix.py)


@pytest.fixture(scope="module")
def series(orc, golden_case):
    grid, tmin, _ = golden_case
    return gc.every_k_series(orc, grid, tmin, "tmin")


def test_arbiter_hat_row_reproduces_the_point_and_sums_to_one():
    """Known answers that do not come from the oracle: a hat row reproduces every predictor at the point (x0' (X'WX)^-1 X'W X
    = x0'), so sum z = 1 and sum z_j x_j = x0."""
    from oracle import arbiter
    rng = np.random.default_rng(3)
    X5 = rng.normal(size=(23, 5)) * (1.0, 1.0, 800.0, 30.0, 6.0) + (-110.0, 45.0, 1500.0, 40.0, 280.0)
    w = rng.uniform(0.01, 1.0, 23)
    x5 = X5.mean(axis=0) + 0.1
    z = np.array(arbiter.gwr_hat(X5, w, x5))
    assert abs(z.sum() - 1.0) < 1e-12
    assert np.abs(z @ X5 - x5).max() < 1e-9                  # (|x| ~ 1500, 152 terms of fp64 rounding)


def test_oracle_series_against_the_arbiter_at_every_bandwidth(series):
    s = series
    assert np.array_equal(s["ks"], np.arange(6, 153)) and len(np.unique(s["cells"], axis=0)) == s["ks"].size
    assert np.all(s["rc"] == 0), s["ks"][s["rc"] != 0].tolist()
    e = s["e_k"]
    print("oracle vs arbiter: worst %.3g degC at ka = %d; from ka = 10 up %.3g" % (e.max(), s["ks"][e.argmax()],
                                                                                  e[s["ks"] >= 10].max()))
    bad = np.nonzero(~(e <= F64_BAR))[0]
    assert bad.size == 0, ("ka =", s["ks"][bad].tolist(), e[bad].tolist())
