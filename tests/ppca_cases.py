"""Shared by tests/test_ppca_host.py and tests/test_gpu_ppca.py: the golden pool of make_golden_ppca.py, a random pool, the
restatement's record of a matrix and the neighbour matrices from the numpy restatement (no GPU)."""
import datetime as dt
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_ppca as RP  # noqa: E402

D_REF_MAX, MARGIN_MIN = 1e-12, 1e-6
RANDOM_SEED, RANDOM_NSTN, RANDOM_TARGETS = 5, 80, (0, 41)


def load_gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_ppca_v1.npz"))


def gold_pool(gold):
    """(pool, mean, vari) of the golden: regenerated and pinned by the golden's input hash."""
    import make_golden_infillmat as mk
    import make_golden_ppca as mg
    ids, lon, lat, tmin, days = mg.case_inputs()
    assert mk.input_hash(ids, lon, lat, tmin, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    from topowx_amd.qa import StationObsPool
    mean, vari = mg.normals_of(tmin, days)
    return StationObsPool(ids, lon, lat, tmin, tmin + 10, days), mean, vari


def random_pool(seed=RANDOM_SEED, n=RANDOM_NSTN):
    """80 stations x 3 years, station-dependent noise, 8 % missing, gaps: (pool, mean, vari)."""
    from topowx_amd.dates import MONTH, get_days_metadata
    from topowx_amd.qa import StationObsPool
    rs = np.random.RandomState(seed)
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2003, 12, 31))
    nd = days.size
    lon, lat = -110.0 + 2.0 * rs.rand(n), 45.0 + 1.5 * rs.rand(n)
    t = np.arange(nd)
    fac = np.zeros((nd, 4))
    e = rs.randn(nd, 4) * np.array([3.0, 1.5, 1.0, 0.7])
    for i in range(1, nd):
        fac[i] = 0.7 * fac[i - 1] + e[i]
    load = np.concatenate([np.ones((1, n)), rs.randn(3, n) * 0.8], axis=0)
    noise = 0.25 * 8.0 ** (rs.permutation(n) / (n - 1.0))
    tmin = 2.0 - 12.0 * np.cos(2 * np.pi * (t - 15) / 365.25)[:, None] + fac @ load + rs.randn(n)[None, :] * 2.0 + \
        rs.randn(nd, n) * noise[None, :]
    tmin = np.round(tmin, 1)
    tmin[rs.rand(nd, n) < 0.08] = np.nan
    for s in range(3, n, 7):
        g0 = int(rs.randint(30, nd - 200))
        tmin[g0:g0 + int(rs.randint(40, 150)), s] = np.nan
    tmin = tmin.astype(np.float32)
    mean, vari = np.full((n, 12), np.nan), np.full((n, 12), np.nan)
    for g in range(12):
        rows = tmin[days[MONTH] == g + 1].astype(np.float64)
        for s in range(n):
            v = rows[np.isfinite(rows[:, s]), s]
            if v.size > 1:
                mean[s, g], vari[s, g] = v.mean(), v.var()
    mean[5, :4] = np.nan                                          # eligibility differs between months
    ids = np.array(["RND%05d" % i for i in range(n)])
    return StationObsPool(ids, lon, lat, tmin, tmin + 10, days), mean, vari


def want_search(y, **kw):
    """The restatement's search on a standardised matrix with ``d_ref`` (inf when float64 and longdouble decide differently),
    ``rel_margin`` and ``r2_margin``."""
    thr, mx = kw.get("threshold", 1e-5), kw.get("max_r2cum", 0.99)
    with np.errstate(all="ignore"):
        a = RP.search(y, **kw)
        b = RP.search(y, dtype=np.longdouble, **kw)
    a["d_ref"] = np.inf
    if (a["npcs"], a["nfits"], a["iters"], a["status"]) == (b["npcs"], b["nfits"], b["iters"], b["status"]):
        a["d_ref"] = float(np.abs(a["fit"] - np.asarray(b["fit_ld"], np.float64)).max()) if a["status"] in (0, 20) else 0.0
    a["rel_margin"], a["r2_margin"] = RP.margin(a["all_rels"], thr), RP.margin(a["r2max"], mx)
    return a


def left_out(w):
    return w["d_ref"] > D_REF_MAX or w["rel_margin"] < MARGIN_MIN or w["r2_margin"] < MARGIN_MIN


def host_matrices(pool, mask, targets, months):
    """An ``InfillMatrices`` of the months ``months`` (renumbered 0 ..) from the numpy restatement of the matrix builder."""
    import restate_infillmat as RI
    from topowx_amd.dates import MONTH
    from topowx_amd.infill import InfillMatrices
    month = np.asarray(pool.days[MONTH], np.int64) - 1
    grp = np.full(month.size, -1, np.int8)
    for k, g in enumerate(months):
        grp[month == g] = k
    res = RI.run(pool.lon, pool.lat, pool.tmin, mask, np.asarray(targets), grp)
    full = dict(rounds=1)
    full.update({k: res[k] for k in ("status", "nnghs", "max_dist", "off", "idx", "ioa", "dist", "nlap", "nlap_stn", "keep")})
    return InfillMatrices(pool, "tmin", pool.ids[np.asarray(targets)], np.asarray(targets, np.int32), grp, len(months), full,
                          res["nthres_all"], res["nthres_target_por"], 3)
