#!/usr/bin/env python3
"""Golden vectors of step14's mean / variance estimate (build container only; needs the reference tree, see
make_golden.py):

    python tests/golden/make_golden_emnorm.py

Executed: the same reference slices as make_golden_infillmat.py (its ``case_inputs``, ``load_slice`` and stubs are imported,
that maker is unchanged): one ``_InfillMatrix(...).infill()`` per target station and calendar month of the 48-station pool.
The recorder that stands in for ``r.infill_mu_sigma`` keeps the WHOLE matrix the reference assembled (station columns and
reanalysis scores).  R and ``norm`` are not available: what is recorded for the estimator is the numpy restatement
(tests/restate_emnorm.py) on the recorded matrix, NOT a result of ``em.norm``.  No reference text is stored.

Recorded per item, all 576: ``width`` and ``ncomp`` of the reference's matrix; the restatement's ``mean``, ``variance``,
``iters``, ``status`` at criterion 1e-4; the fully converged ``mean_conv`` / ``variance_conv`` (criterion 1e-12); ``d_ref_mean``
(in standard deviations of the target column) and ``d_ref_var`` (relative): the distance of the float64 restatement from the
``np.longdouble`` one; ``margin``: the smallest relative distance of an iteration's delta from the criterion; ``sd0``.
For the six ``FULL_ITEMS`` of make_golden_infillmat: the score columns.

A second, constructed pool (``cap_inputs``) drives the reference into the more-than-31-columns branch (:361-375): 36
neighbours within 75 km; neighbour c is finite on "bad day" b only when c >= b, so the widening loop ends with all 36 and
the shrink keeps every one; a disturbance common to all neighbours grows with c, so the ioa ranking follows c.  In variant 0 the target has observations
on every bad day (the matrix is cut to 31 columns, no reanalysis column); in variant 1 it is missing on the bad days above
29, which leaves those days without any observation among the 31 columns: the last column is replaced by the first
score.  Recorded per variant: width, whether the score was used, a hash of the station columns, and the restatement.

The script asserts, and fails otherwise (the remedy is another seed): both cap branches are reached; complete data gives
2 iterations; the monotone closed form holds at 1e-12; no ``d_ref`` above 1e-12; no delta within 1e-6 (relative) of the
criterion; the float64 and longdouble runs take the same number of iterations.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_infillmat as mk  # noqa: E402
import restate_emnorm as RE  # noqa: E402
from topowx_amd.dates import MONTH, get_days_metadata  # noqa: E402
from datetime import date  # noqa: E402

CRITERION, CONVERGED = 1e-4, 1e-12
D_REF_MAX, MARGIN_MIN = 1e-12, 1e-6
CAP_SEED, CAP_NNGH, CAP_BAD, CAP_DAYS = 1431, 36, 34, 420
CAP_FIRST = date(2001, 1, 1)


def cap_inputs(variant, seed=CAP_SEED):
    """(ids, lon, lat, tmin [ndays, 37] float32, days) of the constructed pool; station 0 is the target."""
    rs = np.random.RandomState(seed)
    n, nd = CAP_NNGH + 1, CAP_DAYS
    days = get_days_metadata(CAP_FIRST, date.fromordinal(CAP_FIRST.toordinal() + nd - 1))
    lon = -110.0 + np.concatenate([[0.0], 0.02 + 0.01 * np.arange(CAP_NNGH)])
    lat = np.full(n, 45.0)
    ids = np.array(["CAP%05d" % i for i in range(n)])
    sig = np.zeros(nd)
    e = rs.randn(nd) * 3.0
    for i in range(1, nd):
        sig[i] = 0.7 * sig[i - 1] + e[i]
    # a common disturbance scaled by c fixes the order of the ioa; the independent part keeps the columns from being collinear
    scale = np.concatenate([[0.0], 0.5 + 0.15 * np.arange(CAP_NNGH)])
    common = rs.randn(nd) * 1.5
    tmin = np.round(5.0 + sig[:, None] + common[:, None] * scale[None, :] + rs.randn(nd, n) * 0.4, 1)
    bad = 10 + 12 * np.arange(CAP_BAD)                           # the bad days, spread over the axis
    for b in range(CAP_BAD):
        tmin[bad[b], 1:1 + b] = np.nan                           # neighbour c (column 1 + c) is finite only when c >= b
    tmin[rs.rand(nd, n) < 0.03] = np.nan
    for b in range(CAP_BAD):                                     # the random gaps must not touch the construction
        tmin[bad[b], 1 + b:] = np.round(5.0 + sig[bad[b]] + common[bad[b]] * scale[1 + b:] + rs.randn(n - 1 - b) * 0.4, 1)
        tmin[bad[b], 0] = np.round(5.0 + sig[bad[b]], 1)
    if variant == 1:
        tmin[bad[30:], 0] = np.nan
    return ids, lon, lat, tmin.astype(np.float32), days


def estimate(x):
    """The restatement's record of one matrix."""
    a = RE.run(x, CRITERION, 1000)
    b = RE.run(x, CRITERION, 1000, dtype=np.longdouble)
    c = RE.run(x, CONVERGED, 100000)
    assert a["status"] == RE.OK and c["status"] == RE.OK, "an item did not converge: try another seed"
    assert a["iters"] == b["iters"], "float64 and longdouble stop at different iterations: try another seed"
    return dict(mean=a["mean"], variance=a["variance"], iters=a["iters"], status=a["status"], sd0=a["sd0"],
                mean_conv=c["mean"], variance_conv=c["variance"], iters_conv=c["iters"],
                d_ref_mean=float(abs(a["mean"] - b["mean_ld"]) / a["sd0"]),
                d_ref_var=float(abs(a["variance"] / b["variance_ld"] - 1)),
                margin=RE.margin(a["deltas"], CRITERION))


def known_answers():
    rs = np.random.RandomState(5)
    x = rs.randn(257, 31) @ rs.randn(31, 31) + 3.0
    r = RE.run(x, full=True)
    assert r["iters"] == 2 and abs(r["mean"] - x[:, 0].mean()) < 1e-12 and abs(r["variance"] / x[:, 0].var() - 1) < 1e-12, \
        "complete data does not give 2 iterations and the column moments"
    assert np.abs(r["sigma"] - np.cov(x.T, bias=True)).max() < 1e-10
    m = monotone_case()
    r = RE.run(m, CONVERGED, 100000)
    mean, var = monotone_closed_form(m)
    assert abs(r["mean"] - mean) < 1e-10 * abs(mean) + 1e-10 and abs(r["variance"] / var - 1) < 1e-10, "the monotone closed form fails"
    x[rs.rand(*x.shape) < 0.2] = np.nan
    a, b = RE.run(x), RE.run(x, dtype=np.longdouble)
    assert a["iters"] == b["iters"] and abs(a["mean"] - b["mean_ld"]) / a["sd0"] < D_REF_MAX
    assert abs(a["variance"] / b["variance_ld"] - 1) < D_REF_MAX


def monotone_case(n=120, nobs=70, seed=9):
    """Two columns, the second complete, the target (column 0) observed on the first ``nobs`` rows only."""
    rs = np.random.RandomState(seed)
    y = rs.randn(n) * 2.0 + 1.0
    x = 0.8 * y + rs.randn(n) * 0.7 - 3.0
    x[nobs:] = np.nan
    return np.stack([x, y], axis=1)


def monotone_closed_form(m):
    """The ML estimate of a monotone bivariate pattern (Little and Rubin 2002, section 7.2.1; Anderson 1957): regress the
    incomplete column on the complete one over the complete rows, then mean = a + b mu_y, variance = s_res + b^2 s_yy
    (all moments with divisor n)."""
    o = np.isfinite(m[:, 0])
    x, y = m[o, 0], m[o, 1]
    b = ((x - x.mean()) * (y - y.mean())).mean() / y.var()
    a = x.mean() - b * y.mean()
    res = x - a - b * y
    return a + b * m[:, 1].mean(), (res * res).mean() + b * b * m[:, 1].var()


def main():
    known_answers()
    print("known answers hold (complete data: 2 iterations; the monotone closed form; 257 x 31 against longdouble)")
    ids, lon, lat, tmin, days = mk.case_inputs()
    n, G = ids.size, 12
    log = mk._Log()
    ns = mk.load_slice(log)
    stn_da, nnr = mk._StnDa(ids, lon, lat, tmin), mk._Nnr(days.size)
    mask_all = np.ones(n, bool)
    keys = ("mean", "variance", "iters", "status", "sd0", "mean_conv", "variance_conv", "iters_conv", "d_ref_mean",
            "d_ref_var", "margin")
    rec = {k: np.zeros((n, G), np.int32 if k in ("iters", "status", "iters_conv") else np.float64) for k in keys}
    rec["width"], rec["ncomp"] = np.zeros((n, G), np.int32), np.zeros((n, G), np.int32)
    scores = {}
    t0 = time.perf_counter()
    with np.errstate(divide="raise", invalid="raise"):
        for s in range(n):
            for g in range(G):
                log.reset()
                ns["_InfillMatrix"](ids[s], stn_da, mask_all, "tmin", nnr, day_mask=days[MONTH] == g + 1).infill()
                given = np.array(log.given, np.float64)
                rec["width"][s, g], rec["ncomp"][s, g] = given.shape[1], log.ncomp
                assert given.shape[1] <= ns["MAX_COLS_NORM_IMPUTE"]
                if (s, g) in mk.FULL_ITEMS:
                    scores[(s, g)] = given[:, given.shape[1] - log.ncomp:].copy()
                with np.errstate(all="ignore"):
                    e = estimate(given)
                for k in keys:
                    rec[k][s, g] = e[k]
            print("station %d of %d, %.0f s" % (s + 1, n, time.perf_counter() - t0), flush=True)
    dm = np.abs(rec["mean"] - rec["mean_conv"]) / rec["sd0"]
    dv = np.abs(rec["variance"] / rec["variance_conv"] - 1)
    print("iterations %d .. %d (converged: up to %d); criterion 1e-4 against converged, all %d items: mean %.3g typical "
          "(median), %.3g largest, in column standard deviations; variance %.3g typical, %.3g largest, relative" % (
              rec["iters"].min(), rec["iters"].max(), rec["iters_conv"].max(), n * G, np.median(dm), dm.max(), np.median(dv),
              dv.max()))
    print("d_ref: mean %.3g, variance %.3g (largest); smallest delta margin %.3g" % (
        rec["d_ref_mean"].max(), rec["d_ref_var"].max(), rec["margin"].min()))
    assert max(rec["d_ref_mean"].max(), rec["d_ref_var"].max()) <= D_REF_MAX, "a d_ref above 1e-12: try another seed"
    assert rec["margin"].min() >= MARGIN_MIN, "a delta within 1e-6 of the criterion: try another seed"

    # the constructed pool: the more-than-31-columns branch and its zero-observation sub-branch
    cap = {}
    for variant in (0, 1):
        cids, clon, clat, ctmin, cdays = cap_inputs(variant)
        log.reset()
        cda, cnnr = mk._StnDa(cids, clon, clat, ctmin), mk._Nnr(cdays.size)
        with np.errstate(divide="raise", invalid="raise"):
            ns["_InfillMatrix"](cids[0], cda, np.ones(cids.size, bool), "tmin", cnnr, day_mask=None).infill()
        given = np.array(log.given, np.float64)
        assert log.shrink_in.shape[1] - 1 == CAP_NNGH, "the widening loop did not take all 36 neighbours: try another seed"
        assert given.shape[1] == 31, "the column cap was not reached: try another seed"
        # the ranking follows c: the station columns are the pool's columns 1 .. 30 (29 where the score replaced the last)
        pc = nnr_first_score(cnnr.m)
        used = bool(np.abs(np.abs(given[:, -1]) - np.abs(pc)).max() < 1e-9 * np.abs(pc).max())
        nst = 29 if used else 30
        assert np.array_equal(given[:, :1 + nst], ctmin[:, :1 + nst].astype(np.float64), equal_nan=True), \
            "the ioa ranking does not follow the construction: try another seed"
        assert used == (variant == 1), "the cap branches are not reached as constructed: try another seed"
        with np.errstate(all="ignore"):
            e = estimate(given)
        assert max(e["d_ref_mean"], e["d_ref_var"]) <= D_REF_MAX and e["margin"] >= MARGIN_MIN, "try another seed"
        cap[variant] = dict(e, width=given.shape[1], used_score=used, hash=mk.matrix_hash(given[:, :1 + nst]),
                            input_hash=mk.input_hash(cids, clon, clat, ctmin, cdays))
        print("cap variant %d: width %d, score used %s, %d iterations, mean %.6f variance %.6f" % (
            variant, given.shape[1], used, e["iters"], e["mean"], e["variance"]))

    out = dict(input_hash=mk.input_hash(ids, lon, lat, tmin, days), criterion=np.float64(CRITERION),
               converged_criterion=np.float64(CONVERGED), **rec)
    for (s, g), m in scores.items():
        out["scores_%d_%d" % (s, g)] = m
    for variant, c in cap.items():
        for k, v in c.items():
            out["cap%d_%s" % (variant, k)] = np.asarray(v)
    path = os.path.join(HERE, "golden_emnorm_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


def nnr_first_score(m):
    """The first principal-component score of the stub reanalysis matrix, as pca_svd(A, True, True) gives it."""
    a = m - m.mean(axis=0)
    a = a / a.std(axis=0, ddof=1)
    _, _, v = np.linalg.svd(a, full_matrices=False)
    return a @ v[0]


if __name__ == "__main__":
    main()
