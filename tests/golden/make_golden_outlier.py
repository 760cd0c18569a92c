#!/usr/bin/env python3
"""Golden vectors of step20's outlier screen (``XvalOutlier``), made by EXECUTING the reference's source (build
container only; needs the reference tree, see make_golden.py):

    python tests/golden/make_golden_outlier.py

Executed: twx/interp/optimize.py:84-207 (``XvalOutlier``: ``__init__``, ``run_xval_stn``, ``find_xval_outliers``) on
top of the reference's own ``StationSelect`` (``make_golden.load_reference``), with real pandas.

The ONE substitution: statsmodels and patsy are not installed, so ``statsmodels.formula.api.wls`` is replaced by
``_WlsStandIn`` below -- the same policy as ``make_golden.uk_numpy`` standing in for gstat.  It parses the
``y~a+b+c+d`` formulas the slice builds, adds the intercept, drops the rows with a NaN in any formula variable (patsy's
``missing='drop'``, weights dropped with them), solves the weighted least-squares problem with ``np.linalg.lstsq`` on
``sqrt(w)``-scaled rows and columns, and its ``predict`` takes the one-row DataFrame of the left-out station (NaN in,
NaN out, as statsmodels re-inserts dropped prediction rows).  None of the fits here is rank-deficient, so ``lstsq``
and statsmodels' ``pinv`` agree to rounding.

Inputs: ``make_golden.case_inputs()`` (400 Tmin + 400 Tmax stations) perturbed as follows, per variable:
  * PLANTED outliers: one monthly normal of 4 good stations shifted by +-12 degC (ids / months / shifts stored);
  * BAD: 5 stations flagged bad (bad = 1) -- out of the pool, still left out and scored with ``stn_ids=None``;
  * PAIR: one good station moved onto another good station's coordinates (exactly co-located: each is removed from
    the other's neighbourhood, rm_zero_dist_stns);
  * NAN_LST: one good station with a NaN lst in one month (dropped from its neighbours' fits of that month, its own
    error of that month is NaN, its annual lst is the mean of the other 11 months).
Outputs (``golden_outlier_v1.npz``): the hash of the unperturbed inputs, the perturbation, the perturbed tables'
hash, ``errs[13, n]`` of every station (``stn_ids=None``), and the outlier ids of ``find_xval_outliers()`` and of
step20's call over the good stations.  The script fails if any z-score lies within 0.05 of the threshold (rounding
could then move an id).  No reference text is stored.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from topowx_amd import stationdb as sdb  # noqa: E402

THRESHOLD = 6
BW_NNGH = 100
MARGIN = 0.05
PERTURB = {  # var -> planted (good-station index, month, shift), bad indices, pair (moved, onto), NaN lst (index, month)
    "tmin": dict(planted=((17, 3, 12.0), (102, 7, -12.0), (233, 11, 12.0), (351, 1, -12.0)),
                 bad=(5, 61, 144, 290, 377), pair=(208, 207), nan_lst=(95, 6)),
    "tmax": dict(planted=((29, 5, -12.0), (150, 9, 12.0), (265, 2, -12.0), (388, 12, 12.0)),
                 bad=(12, 88, 199, 301, 366), pair=(120, 119), nan_lst=(244, 10)),
}


class _WlsStandIn(object):
    """``statsmodels.formula.api.wls(formula, data=, weights=)`` for ``'y~a+b+c+d'`` (see the module docstring)."""

    def __init__(self, formula, data, weights):
        lhs, rhs = formula.replace(" ", "").split("~")
        self.cols = rhs.split("+")
        y = np.asarray(data[lhs], np.float64)
        X = np.column_stack([np.ones(len(data))] + [np.asarray(data[c], np.float64) for c in self.cols])
        keep = np.isfinite(y) & np.isfinite(X).all(axis=1)
        self.y, self.X, self.w = y[keep], X[keep], np.asarray(weights, np.float64)[keep]

    def fit(self):
        sw = np.sqrt(self.w)
        beta = np.linalg.lstsq(self.X * sw[:, None], self.y * sw, rcond=None)[0]
        return types.SimpleNamespace(params=beta, predict=lambda df: self._predict(beta, df))

    def _predict(self, beta, df):
        X = np.column_stack([np.ones(len(df))] + [np.asarray(df[c], np.float64) for c in self.cols])
        return X @ beta


def perturbed(stn_da, var):
    """Copy of a case database with the PERTURB[var] edits; returns (db, description arrays)."""
    p = PERTURB[var]
    stns = stn_da.stns.copy()
    good = np.nonzero(np.isnan(stns[sdb.BAD]))[0]
    ids = stns[sdb.STN_ID]
    for j, m, shift in p["planted"]:
        stns[sdb.get_norm_varname(m)][good[j]] += shift
    a, b = p["pair"]
    stns[sdb.LON][good[a]], stns[sdb.LAT][good[a]] = stns[sdb.LON][good[b]], stns[sdb.LAT][good[b]]
    j, m = p["nan_lst"]
    stns[sdb.get_lst_varname(m)][good[j]] = np.nan
    stns[sdb.BAD][good[list(p["bad"])]] = 1.0
    desc = {"planted_ids": ids[good[[q[0] for q in p["planted"]]]].astype("U16"),
            "planted_mth": np.array([q[1] for q in p["planted"]], np.int32),
            "planted_shift": np.array([q[2] for q in p["planted"]]),
            "bad_ids": ids[good[list(p["bad"])]].astype("U16"),
            "pair_ids": ids[good[[a, b]]].astype("U16"),
            "nan_lst_id": np.array(ids[good[j]], "U16"), "nan_lst_mth": np.int32(m)}
    return sdb.StationSerialDataDb(stns, var, stn_da.days), desc


def zscore_margin(errs):
    import pandas as pd
    e = pd.DataFrame(errs)
    z = e.subtract(e.mean(axis=1), axis=0).divide(e.std(axis=1), axis=0).abs().values
    return float(np.nanmin(np.abs(z - THRESHOLD)))


def main():
    geo, ss, it, opt = mg.load_reference()
    import pandas as pd
    warnings.filterwarnings("ignore", category=FutureWarning)
    grid, tmin, tmax = mg.case_inputs()
    out = dict(input_hash=mg.input_hash(grid, tmin, tmax), threshold=np.float64(THRESHOLD), bw_nngh=np.int32(BW_NNGH))

    class FakeStatus(object):
        def __init__(self, *a, **k):
            pass

        def increment(self, *a):
            pass

    ns = dict(np=np, pd=pd, sm=types.SimpleNamespace(wls=_WlsStandIn), StationSelect=ss["StationSelect"],
              StatusCheck=FakeStatus, BAD=sdb.BAD, STN_ID=sdb.STN_ID, LAT=sdb.LAT, LON=sdb.LON,
              get_norm_varname=sdb.get_norm_varname, get_lst_varname=sdb.get_lst_varname)
    exec(compile(mg._slice("twx/interp/optimize.py", 84, 207), "optimize_84", "exec"), ns)
    for var, da0 in (("tmin", tmin), ("tmax", tmax)):
        da, desc = perturbed(da0, var)
        xo = ns["XvalOutlier"](da)
        ids_all = da.stn_ids
        errs = np.zeros((13, ids_all.size))
        for i, a_id in enumerate(ids_all):                       # what find_xval_outliers(None) computes (:192-196)
            errs[:, i] = xo.run_xval_stn(a_id, BW_NNGH)
        out_all = xo.find_xval_outliers(None, BW_NNGH, THRESHOLD)
        good_ids = da.stn_ids[np.isnan(da.stns[sdb.BAD])]      # step20:87
        out_good = xo.find_xval_outliers(good_ids, BW_NNGH, THRESHOLD)
        good = np.isnan(da.stns[sdb.BAD])
        m_all, m_good = zscore_margin(errs), zscore_margin(errs[:, good])
        assert min(m_all, m_good) > MARGIN, (var, m_all, m_good)
        print(var, "outliers (all):", list(out_all), "(good):", list(out_good), "z margin %.3f / %.3f" % (m_all, m_good))
        out["errs_" + var] = errs
        out["out_all_" + var] = np.asarray(out_all, "U16")
        out["out_good_" + var] = np.asarray(out_good, "U16")
        out["stns_hash_" + var] = mg.sha(np.frombuffer(da.stns.tobytes(), np.uint8))
        for k, v in desc.items():
            out["%s_%s" % (k, var)] = v
    path = os.path.join(HERE, "golden_outlier_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
