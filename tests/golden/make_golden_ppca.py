#!/usr/bin/env python3
"""Golden vectors of step16's daily infill (build container only; needs the reference tree, see make_golden.py):

    python tests/golden/make_golden_ppca.py

Executed: twx/infill/infill_daily.py:42-47 (the constants), :53-436 and :520-524 (``InfillMatrixPPCA`` with ``__init__``,
``__extend_ngh_radius``, ``__merge``, ``__has_min_daily_nghs`` and ``infill`` up to the ``r.ppca_tair`` call and from
``fnl_tair`` on; the ``chk_perf`` block between them, which is out of scope and holds Python-2 ``print`` statements, is
left out and ``infill(chk_perf=False)`` is called), :599-625 (``_shrink_matrix``), with ``grt_circle_dist``, ``calc_ioa_d1``
and ``pca_svd`` as make_golden_infillmat.py loads them (its ``load_slice`` and stubs are imported, that maker is unchanged).
One ``InfillMatrixPPCA(...).infill()`` per target station and calendar month, as ``infill_daily_obs`` (:548-559) runs them.

Shims and stand-ins: ``_load_R`` does nothing; ``robjects.Matrix`` / ``FloatVector`` are identities; ``r.ppca_tair`` records
its arguments (the trimmed matrix, ``trim_ngh_norms``, ``trim_ngh_std``, the keywords) and returns zeros.  R and
``pcaMethods`` are not available: what is recorded for the estimator is the numpy restatement (tests/restate_ppca.py) on
the recorded arguments, NOT a result of ``pcaMethods``.  The station table carries ``meanMM`` / ``variMM`` fields: the
month's mean and variance of each station over its finite values (a stand-in for step14's estimates), NaN for a few
(station, month) pairs so that the eligibility mask differs between months.  Pool A has no reanalysis: its stub returns a
matrix without columns and ``pca_svd`` of that gives no scores (the reference has no such mode).  Pool B (the first
``NNR_TARGETS`` targets again) gets the seeded stand-in reanalysis of make_golden_infillmat.  No reference text is stored.

Recorded per item (pool A: target * 12 + month, then pool B likewise): the pool columns of the trimmed matrix (each
matrix column matched to its station), ``norms`` / ``stds``, ``width``, ``ncomp``, ``max_dist``; the restatement's search:
``npcs``, ``nfits``, ``iters``, ``status``, ``r2_not_reached``, the fit (standardised scale); ``d_ref``: the distance of the
float64 restatement's fit from the ``np.longdouble`` one, in target standard deviations; ``rel_margin`` / ``r2_margin``: the
smallest relative distance of any iteration's ``rel`` from the threshold and of any fit's largest R2cum from ``max_r2cum``.
For ``SCORE_ITEMS`` of pool B: the score columns.

The script refuses to write a golden in which a margin is below 1e-6, or in which the float64 and longdouble searches
differ in npcs, fits or iterations (the remedy is another seed).
"""
import os
import sys
import time
from datetime import date

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_infillmat as mk  # noqa: E402
import restate_ppca as RP  # noqa: E402
from topowx_amd.dates import MONTH, YMD, get_days_metadata  # noqa: E402

SEED = 16031
NSTN = 18
FIRST, LAST = date(1998, 1, 1), date(2001, 12, 31)
HALF = (15, 16)                       # record only the second half
NAN_NORMALS = ((3, (0, 1, 2, 3, 4, 5)), (9, (6,)))      # (station, months) without mean / variance: no neighbour there
NNR_TARGETS = 4
SCORE_ITEMS = ((0, 0), (1, 5), (2, 8), (3, 11))
MARGIN_MIN = 1e-6
NOISE_MIN, NOISE_MAX = 0.25, 2.0


def case_inputs(seed=SEED):
    """(ids, lon, lat, tmin [ndays, n] float32, days)."""
    rs = np.random.RandomState(seed)
    days = get_days_metadata(FIRST, LAST)
    nd, n = days.size, NSTN
    lon = -110.0 + 0.9 * rs.rand(n)
    lat = 45.0 + 0.6 * rs.rand(n)
    lon[17], lat[17] = -108.3, 45.9                            # alone: its first ring is thin
    ids = np.array(["PPC%05d" % i for i in range(n)])
    t = np.arange(nd)
    season = -12.0 * np.cos(2 * np.pi * (t - 15) / 365.25)

    def ar1(scale):
        reg, e = np.zeros(nd), rs.randn(nd) * scale
        for i in range(1, nd):
            reg[i] = 0.7 * reg[i - 1] + e[i]
        return reg
    factors = np.stack([ar1(3.0), ar1(1.5), ar1(1.0)], axis=1)
    load = np.concatenate([np.ones((1, n)), rs.randn(2, n) * 0.8], axis=0)
    # local noise of very different size from station to station: with equal noise the trailing eigenvalues of an item
    # coincide, a column of C shrinks to nothing and the basis of its column space is rounding noise
    noise = NOISE_MIN * (NOISE_MAX / NOISE_MIN) ** (rs.permutation(n) / (n - 1.0))
    tmin = 2.0 + season[:, None] + factors @ load + rs.randn(n)[None, :] * 2.0 + rs.randn(nd, n) * noise[None, :]
    tmin = np.round(tmin, 1)
    tmin[rs.rand(nd, n) < 0.06] = np.nan
    for s in range(2, n, 4):                                   # a gap of several months
        g0 = int(rs.randint(60, nd - 300))
        tmin[g0:g0 + int(rs.randint(70, 200)), s] = np.nan
    half = int(np.nonzero(days[YMD] == 20000101)[0][0])
    for s in HALF:
        tmin[:half, s] = np.nan
    return ids, lon, lat, tmin.astype(np.float32), days


def normals_of(tmin, days):
    """(mean, vari) [n, 12]: each station's mean and variance (divisor n) over its finite values of the month, NaN for the
    pairs of ``NAN_NORMALS``."""
    n = tmin.shape[1]
    mean, vari = np.full((n, 12), np.nan), np.full((n, 12), np.nan)
    x = tmin.astype(np.float64)
    for g in range(12):
        rows = x[days[MONTH] == g + 1]
        for s in range(n):
            v = rows[np.isfinite(rows[:, s]), s]
            if v.size > 1:
                mean[s, g], vari[s, g] = v.mean(), v.var()
    for s, months in NAN_NORMALS:
        mean[s, list(months)] = np.nan
        vari[s, list(months)] = np.nan
    return mean, vari


class _NoNnr(object):
    def __init__(self, ndays):
        self.ndays = ndays

    def get_nngh_matrix(self, lon, lat, var, utc_offset=None, nngh=4):
        return np.zeros((self.ndays, 0))


class _Rec(object):
    args = None


def load_slice(rec):
    """The namespace of make_golden_infillmat.load_slice with the slices of infill_daily.py executed on top."""
    import make_golden as mg
    log = mk._Log()
    log.reset()
    ns = mk.load_slice(log)
    pca0 = ns["pca_svd"]

    def pca(a, *args, **kw):
        if a.shape[1] == 0:                                    # pool A: no reanalysis, no scores
            return None, np.zeros((a.shape[0], 0)), np.array([1.0])
        return pca0(a, *args, **kw)

    ns["pca_svd"] = pca
    exec(compile("\n" * 41 + mg._slice("twx/infill/infill_daily.py", 42, 47), "infill_daily.py", "exec"), ns)
    body = mg._slice("twx/infill/infill_daily.py", 53, 436) + "\n" * 83 + mg._slice("twx/infill/infill_daily.py", 520, 524)
    exec(compile("\n" * 52 + body, "infill_daily.py", "exec"), ns)
    exec(compile("\n" * 598 + mg._slice("twx/infill/infill_daily.py", 599, 625), "infill_daily.py", "exec"), ns)

    class Rx(object):
        def __init__(self, n):
            self.n = n

        def rx(self, name):
            return np.zeros((1, self.n))

    class R(object):
        @staticmethod
        def ppca_tair(m, norms, stds, **kw):
            rec.args = (np.array(m, np.float64), np.array(norms, np.float64), np.array(stds, np.float64), dict(kw))
            return Rx(np.asarray(m).shape[0])

    class Robjects(object):
        Matrix = staticmethod(lambda m: m)
        FloatVector = staticmethod(lambda v: v)

    ns.update(r=R, robjects=Robjects, _load_R=lambda: None)
    return ns


def stn_table(ids, lon, lat, tmin, mean, vari):
    da = mk._StnDa(ids, lon, lat, tmin)
    dt = da.stns.dtype.descr + [("mean%02d" % m, np.float64) for m in range(1, 13)] + \
        [("vari%02d" % m, np.float64) for m in range(1, 13)]
    stns = np.empty(ids.size, dtype=dt)
    for name in da.stns.dtype.names:
        stns[name] = da.stns[name]
    for g in range(12):
        stns["mean%02d" % (g + 1)], stns["vari%02d" % (g + 1)] = mean[:, g], vari[:, g]
    da.stns, da.stn_ids = stns, stns["station_id"]
    return da


def record_item(ns, rec, stn_da, nnr, sid, g, tmin, mask):
    rec.args = None
    with np.errstate(divide="raise", invalid="raise"):
        mat = ns["InfillMatrixPPCA"](sid, stn_da, "tmin", nnr, "mean%02d" % (g + 1), "vari%02d" % (g + 1), day_mask=mask)
        mat.infill(chk_perf=False)
    m, norms, stds, kw = rec.args
    rows = tmin[mask].astype(np.float64)
    nst = sum(1 for c in range(m.shape[1]) if any(np.array_equal(m[:, c], rows[:, s], equal_nan=True)
                                                   for s in range(rows.shape[1])))
    cols = []
    for c in range(nst):
        hit = [s for s in range(rows.shape[1]) if np.array_equal(m[:, c], rows[:, s], equal_nan=True)]
        assert len(hit) == 1, "a matrix column matches %d stations: try another seed" % len(hit)
        cols.append(hit[0])
    assert np.isfinite(norms).all() and np.isfinite(stds).all()
    return dict(m=m, norms=norms, stds=stds, kw=kw, cols=np.array(cols, np.int32), ncomp=m.shape[1] - nst,
                max_dist=float(mat.max_dist))


def search_record(it):
    y = (it["m"] - it["norms"]) / it["stds"]
    kw = it["kw"]
    assert kw["npcs"] == 0
    a = RP.search(y, None, 0, kw["frac_obs"], kw["max_r2cum"], kw["convThres"])
    b = RP.search(y, None, 0, kw["frac_obs"], kw["max_r2cum"], kw["convThres"], dtype=np.longdouble)
    assert a["status"] in (RP.OK, RP.MAXITS), "an item ended with status %d: try another seed" % a["status"]
    assert (a["npcs"], a["nfits"], a["iters"], a["status"]) == (b["npcs"], b["nfits"], b["iters"], b["status"]), \
        "float64 and longdouble searches differ: try another seed"
    return dict(npcs=a["npcs"], nfits=a["nfits"], iters=a["iters"], status=a["status"], r2_not_reached=a["r2_not_reached"],
                fit=a["fit"], d_ref=float(np.abs(a["fit"] - np.asarray(b["fit_ld"], np.float64)).max()),
                rel_margin=RP.margin(a["all_rels"], kw["convThres"]), r2_margin=RP.margin(a["r2max"], kw["max_r2cum"]),
                threshold=kw["convThres"], max_r2cum=kw["max_r2cum"], frac_obs=kw["frac_obs"])


def main():
    ids, lon, lat, tmin, days = case_inputs()
    mean, vari = normals_of(tmin, days)
    n, nd = ids.size, days.size
    rec = _Rec()
    ns = load_slice(rec)
    stn_da = stn_table(ids, lon, lat, tmin, mean, vari)
    masks = [days[MONTH] == g + 1 for g in range(12)]
    items = []
    t0 = time.perf_counter()
    for pool, nnr, targets in (("A", _NoNnr(nd), range(n)), ("B", mk._Nnr(nd), range(NNR_TARGETS))):
        for s in targets:
            for g in range(12):
                if not np.isfinite(mean[s, g]):
                    continue                                    # a target without normals is not infilled that month
                it = record_item(ns, rec, stn_da, nnr, ids[s], g, tmin, masks[g])
                it.update(search_record(it), pool=pool, t=s, g=g)
                items.append(it)
            print("pool %s station %d, %.0f s" % (pool, s, time.perf_counter() - t0), flush=True)
    ni = len(items)
    rel_m, r2_m = min(i["rel_margin"] for i in items), min(i["r2_margin"] for i in items)
    print("%d items; widths %d .. %d; npcs %d .. %d; fits up to %d; iterations %d .. %d; r2_not_reached %d; d_ref up to "
          "%.3g; margins: rel %.3g, R2cum %.3g" % (
              ni, min(i["m"].shape[1] for i in items), max(i["m"].shape[1] for i in items),
              min(i["npcs"] for i in items), max(i["npcs"] for i in items), max(i["nfits"] for i in items),
              min(i["iters"] for i in items), max(i["iters"] for i in items), sum(i["r2_not_reached"] for i in items),
              max(i["d_ref"] for i in items), rel_m, r2_m))
    assert rel_m >= MARGIN_MIN and r2_m >= MARGIN_MIN, "a rel or an R2cum within 1e-6 of its bound: try another seed"
    assert any(i["ncomp"] > 0 for i in items) and len({i["max_dist"] for i in items}) > 1
    assert len({i["m"].shape[1] for i in items}) > 2 and any(i["nfits"] > 1 for i in items)

    def csr(key, dt):
        off = np.concatenate([[0], np.cumsum([len(i[key]) for i in items])]).astype(np.int64)
        return off, np.concatenate([np.asarray(i[key], dt) for i in items])
    col_off, cols = csr("cols", np.int32)
    par_off, norms = csr("norms", np.float64)
    _, stds = csr("stds", np.float64)
    fit_off, fit = csr("fit", np.float64)
    out = dict(input_hash=mk.input_hash(ids, lon, lat, tmin, days), seed=np.int32(SEED),
               pool=np.array([i["pool"] for i in items]), target=np.array([i["t"] for i in items], np.int32),
               month=np.array([i["g"] for i in items], np.int32), col_off=col_off, cols=cols, par_off=par_off, norms=norms,
               stds=stds, fit_off=fit_off, fit=fit, width=np.array([i["m"].shape[1] for i in items], np.int32))
    for k, dt in (("ncomp", np.int32), ("max_dist", np.float64), ("npcs", np.int32), ("nfits", np.int32), ("iters", np.int32),
                  ("status", np.int32), ("r2_not_reached", bool), ("d_ref", np.float64), ("rel_margin", np.float64),
                  ("r2_margin", np.float64), ("threshold", np.float64), ("max_r2cum", np.float64), ("frac_obs", np.float64)):
        out[k] = np.array([i[k] for i in items], dt)
    for i in items:
        if i["pool"] == "B" and (i["t"], i["g"]) in SCORE_ITEMS:
            out["scores_%d_%d" % (i["t"], i["g"])] = i["m"][:, i["m"].shape[1] - i["ncomp"]:]
    path = os.path.join(HERE, "golden_ppca_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
