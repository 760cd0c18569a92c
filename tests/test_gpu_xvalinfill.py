"""GPU: step15, the cross-validation of the infill (``twxxv_holdout`` / ``twxxv_infill_matrix`` / ``twxxv_score``;
``topowx_amd.infill.XvalInfill``; ``python -m topowx_amd.step15``).

Exact, because derived and not measured: the hold-out is integer logic; the exclusion only removes one station from a
target's rings; the batched chain hands the same kernels the same values as the parent's functions do on a pool copy
with one masked column, and no sum of any kernel depends on what else is in the batch.  A difference there is a leak
between targets, never a tolerance to widen.

Bounded: ``bias`` / ``mae`` of ``twxxv_score`` against a float64 numpy restatement, whose summation order differs from the
kernel's.  The bound is the project's own for a different but fixed order (``chkperf_cases``): the larger of 100 x the
restatement's own float64-versus-longdouble distance and N 2^-52."""
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib
from topowx_amd.dates import MONTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chkperf_cases as CC  # noqa: E402
import xvalinfill_cases as XC  # noqa: E402

pytestmark = pytest.mark.gpu
VARYEXPLAIN = 0.75                 # the facade pool's ppca_varyexplain, as tests/test_gpu_chkperf.py sets it
CSR = ("off", "idx", "ioa", "dist", "nlap", "nlap_stn", "keep")


# ---- 1. the hold-out ----
@pytest.mark.parametrize("ndays", XC.HOLD_NDAYS)
def test_holdout_smallest_shapes(ndays):
    rows = XC.holdout_rows(ndays)
    idx = np.arange(len(rows), dtype=np.int32)[::-1].copy()         # the rows in another order than the table's
    for nkeep in XC.holdout_nkeeps(rows):
        tm = {}
        got = _qalib.holdout(rows, idx, nkeep, timing=tm)
        assert np.isfinite(tm["xv_holdout_kernel_ms"]) and tm["xv_holdout_kernel_ms"] >= 0
        held, train, nheld, nfin = XC.want_holdout(rows[idx], nkeep)
        assert np.array_equal(got["held"], held), (ndays, nkeep)
        assert got["train_obs"].tobytes() == train.tobytes(), (ndays, nkeep)
        assert np.array_equal(got["nheld"], nheld) and np.array_equal(got["nfinite"], nfin), (ndays, nkeep)
        if nkeep == 0:
            assert not held.any()


# ---- 2. the exclusion changes nothing else ----
@pytest.fixture(scope="module")
def infill_case():
    import make_golden_infillmat as mk
    from topowx_amd.infill import item_thresholds
    ids, lon, lat, tmin, days = mk.case_inputs()
    obs = np.ascontiguousarray(tmin.T)
    group = (np.asarray(days[MONTH]) - 1).astype(np.int8)
    nall, npor = item_thresholds(obs, group, 12)
    n = ids.size
    args = dict(lon=lon, lat=lat, obs=obs, ymd=np.asarray(days["YMD"]), eligible=np.ones(n, bool),
                target_idx=np.arange(n, dtype=np.int32), group=group, nthres_all=nall, nthres_target_por=npor)
    return args, _qalib.infill_matrix(**args)


def _same(a, b):
    return [k for k in ("status", "nnghs", "max_dist") + CSR if a[k].tobytes() != b[k].tobytes()]


def test_exclusion_of_nothing_is_the_old_entry(infill_case):
    args, old = infill_case
    tm = {}
    new = _qalib.infill_matrix(exclude_idx=np.full(args["lon"].size, -1, np.int32), timing=tm, **args)
    assert _same(old, new) == [] and new["rounds"] == old["rounds"]
    times = [k for k in tm if k.endswith("_ms")]
    assert len(times) >= 4 and all(np.isfinite(tm[k]) and tm[k] >= 0 for k in times), tm


def test_exclusion_of_one_station_per_target(infill_case):
    args, old = infill_case
    n = args["lon"].size
    first = old["idx"][old["off"][np.arange(n) * 12]]               # each target's best-ranked station of January
    assert (first != np.arange(n)).all()
    new = _qalib.infill_matrix(exclude_idx=first, **args)
    changed = 0
    for t in range(n):
        elig = np.ones(n, bool)
        elig[first[t]] = False
        one = _qalib.infill_matrix(**dict(args, eligible=elig, target_idx=np.array([t], np.int32),
                                          nthres_target_por=args["nthres_target_por"][t:t + 1]))
        a, b = new["off"][t * 12], new["off"][(t + 1) * 12]
        for k in ("status", "nnghs", "max_dist"):
            assert new[k][t].tobytes() == one[k][0].tobytes(), (k, t)
        assert np.array_equal(new["off"][t * 12:(t + 1) * 12 + 1] - a, one["off"]), t
        for k in CSR[1:]:
            assert new[k][a:b].tobytes() == one[k].tobytes(), (k, t)
        assert first[t] not in new["idx"][a:b]
        changed += new["idx"][a:b].tobytes() != old["idx"][old["off"][t * 12]:old["off"][(t + 1) * 12]].tobytes()
    assert changed == n


def test_the_colocated_twin_stays_a_neighbour():
    """Station 1 stands where station 0 does (distance 0).  Excluding station 2 from target 0 leaves the twin in the first
    ring; excluding the twin leaves station 2."""
    rs = np.random.RandomState(5)
    n, nd = 7, 90
    sig = rs.randn(nd) * 5
    obs = np.round(sig[None, :] + rs.randn(n, nd), 1).astype(np.float32)
    lon, lat = -110.0 + 0.1 * np.arange(n), np.full(n, 45.0)
    lon[1] = lon[0]
    from topowx_amd.dates import get_days_metadata
    import datetime as dt
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2001, 1, 1) + dt.timedelta(days=nd - 1))
    args = dict(lon=lon, lat=lat, obs=obs, ymd=np.asarray(days["YMD"]), eligible=np.ones(n, bool),
                target_idx=np.array([0, 0], np.int32), group=np.zeros(nd, np.int8), nthres_all=np.array([60], np.int32),
                nthres_target_por=np.array([[60], [60]], np.int32))
    r = _qalib.infill_matrix(exclude_idx=np.array([2, 1], np.int32), **args)
    assert (r["status"] == _qalib.IF_OK).all()
    a, b = r["idx"][r["off"][0]:r["off"][1]], r["idx"][r["off"][1]:r["off"][2]]
    assert 1 in a and 2 not in a and 2 in b and 1 not in b
    assert r["dist"][r["off"][0]:r["off"][1]][a == 1][0] == 0.0
    with pytest.raises(_qalib.QaError, match="exclude index"):
        _qalib.infill_matrix(exclude_idx=np.array([n, -1], np.int32), **args)
    with pytest.raises(_qalib.QaError, match="exclude index"):
        _qalib.infill_matrix(exclude_idx=np.array([0, -2], np.int32), **args)


# ---- 3. isolation: all appended targets in one call against the parent code on a masked copy, one target at a time ----
def _isolation(pool, mask, cols, ntrain_yrs):
    from topowx_amd.infill import XvalInfill, build_infill_matrices
    n = pool.ids.size
    xv = XvalInfill(pool, "tmin", None, np.zeros((n, 12)), np.zeros((n, 12)), pool.ids[list(cols)], ntrain_yrs)
    held = XC.held_masks(pool, "tmin", cols, xv.nkeep)
    assert np.array_equal(xv.stn_xval_masks, held)
    ext, app_ids, xcols, never = xv.extended_pool()
    assert np.array_equal(xcols, cols) and ext.ids.size == n + len(cols) and never.sum() == len(cols)
    got = build_infill_matrices(ext, "tmin", app_ids, np.concatenate([mask, np.ones(len(cols), bool)]), None, 3,
                                exclude_cols=xcols, never_neighbour=never)
    assert got.idx.size == 0 or got.idx.max() < n                   # an appended row is nobody's neighbour
    month = np.asarray(pool.days[MONTH]) - 1
    for t, c in enumerate(cols):
        one = build_infill_matrices(XC.masked_copy(pool, "tmin", c, held[t]), "tmin", [pool.ids[c]], mask, None, 3)
        ok, where = XC.ranked_equal(got, t, one, 0)
        assert ok, (int(c), where)
        train_fin = np.isfinite(pool.tmin[:, c]) & ~held[t]
        empty = np.array([not train_fin[month == g].any() for g in range(12)])
        assert np.array_equal(got.status[t] == _qalib.IF_NO_TARGET_OBS, empty), int(c)
    return got, held


def test_isolation_on_the_golden_pool():
    import make_golden_infillmat as mk
    from topowx_amd.qa import StationObsPool
    ids, lon, lat, tmin, days = mk.case_inputs()
    pool = StationObsPool(ids, lon, lat, tmin, tmin + 10, days)
    cols = np.array([3, 5, 32, 30, 31, 44], np.int32)               # 5 / 32 near copies; 30 / 31 each other's best candidate
    mask = np.ones(ids.size, bool)
    mask[7] = False
    got, held = _isolation(pool, mask, cols, 4)                     # 1461 of 2922 days: about half of a record is held
    assert (got.status == _qalib.IF_OK).sum() >= 12 * 4 and 0.3 < held[0].mean() < 0.6
    # two cross-validation stations that see each other's FULL record
    r = got.ranked(3, 0)
    assert 31 in r["idx"] and got.ranked(4, 0)["idx"].tolist().count(30) == 1
    got, held = _isolation(pool, mask, cols, 40 / 365.25)           # nkeep 40: most months have no training day
    assert (got.status == _qalib.IF_NO_TARGET_OBS).sum() >= 9 * len(cols)
    assert (got.status != _qalib.IF_NO_TARGET_OBS).any()


def test_isolation_on_the_facade_pool():
    pool, mean, vari = CC.facade_pool()
    cols = np.array(XC.FACADE_XVAL, np.int32)
    got, _ = _isolation(pool, np.isfinite(mean[:, 0]), cols, XC.FACADE_NTRAIN_YRS)
    assert (got.status == _qalib.IF_OK).all()
    assert 2 in got.ranked(0, 0)["idx"] and 1 in got.ranked(1, 0)["idx"]
    _isolation(pool, np.isfinite(mean[:, 0]), cols, 40 / 365.25)


# ---- 4. the score ----
@pytest.mark.parametrize("n", CC.GRID_N)
def test_score(n):
    infill, obs, held, group = XC.score_series(n)
    tm = {}
    got = _qalib.xval_score(infill, obs, held, group, timing=tm)
    assert np.isfinite(tm["xv_score_kernel_ms"]) and tm["xv_score_kernel_ms"] >= 0
    again = _qalib.xval_score(infill, obs, held, group)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    wn, wb, wm, woo, wio = XC.want_score(infill, obs, held, group)
    _, lb, lm, _, _ = XC.want_score(infill, obs, held, group, np.longdouble)
    assert np.array_equal(got["n"], wn[:, 12]) and np.array_equal(got["group_n"], wn[:, :12])
    assert got["obs_out"].tobytes() == woo.tobytes() and got["infill_out"].tobytes() == wio.tobytes()
    assert wn[1].sum() == 0 and np.isnan(got["bias"][1]) and np.isnan(got["group_mae"][1]).all()
    if n >= 64:
        assert wn[0, 12] > 0 and wn[2, 3] == 0 and wn[2, 12] > 0 and wn[3, 7] == wn[3, 12] > 0
    gb = np.concatenate([got["group_bias"], got["bias"][:, None]], axis=1)
    gm = np.concatenate([got["group_mae"], got["mae"][:, None]], axis=1)
    assert np.array_equal(np.isnan(gb), wn == 0) and np.array_equal(np.isnan(gm), wn == 0)
    use = wn > 0
    for name, g, w, l in (("bias", gb, wb, lb), ("mae", gm, wm, lm)):
        tol = np.maximum(CC.FACTOR * np.abs(w[use] - l[use]).astype(np.float64), n * CC.U)
        err = np.abs(g[use] - w[use])
        print("N %d %s: max error %.3g, smallest bound %.3g" % (n, name, err.max() if err.size else 0.0,
                                                                 tol.min() if tol.size else 0.0))
        assert (err <= tol).all(), (n, name)


# ---- 5. the whole chain ----
@pytest.fixture(scope="module")
def chain():
    from topowx_amd.infill import XvalInfill, XvalInfillParams
    pool, mean, vari = CC.facade_pool()
    params = XvalInfillParams(None, 3, 4, 0.99, True, 0, 0.5, VARYEXPLAIN, False)
    ids = pool.ids[list(XC.FACADE_XVAL)]
    xv = XvalInfill(pool, "tmin", params, mean, vari, ids, XC.FACADE_NTRAIN_YRS)
    mean0, vari0 = mean.copy(), vari.copy()
    res = xv.run_all()
    assert np.array_equal(xv.mean, mean0, equal_nan=True) and np.array_equal(xv.vari, vari0, equal_nan=True)
    return pool, mean, vari, xv, res


def test_whole_chain_equals_the_parent_chain_station_by_station(chain):
    from topowx_amd.infill import build_infill_matrices, estimate_mean_variance, infill_daily
    pool, mean, vari, xv, res = chain
    cols = np.array(XC.FACADE_XVAL)
    assert xv.nkeep == 730 and list(xv.mths) == list(range(1, 13))
    held = XC.held_masks(pool, "tmin", cols, 730)
    assert np.array_equal(res.held, held) and np.array_equal(xv.stn_xval_masks, held)
    assert np.array_equal(res.nheld, held.sum(axis=1)) and (0.4 < held.mean(axis=1)).all()
    # nothing of this case is left out: every matrix is ok and every month fitted
    # (the station of the damped group stops its EM at maxits: an estimate all the same, and the same one in both chains)
    assert (res.daily.matrix_status == _qalib.IF_OK).all() and np.isin(res.em_status, (_qalib.EM_OK, _qalib.EM_MAXITS)).all()
    assert (res.em_status[:3] == _qalib.EM_OK).all() and np.isfinite(res.em_mean).all() and (res.em_variance > 0).all()
    assert np.isin(res.daily.status, (_qalib.PP_OK, _qalib.PP_MAXITS)).all()
    for t, c in enumerate(cols):
        cp = XC.masked_copy(pool, "tmin", c, held[t])
        sid = pool.ids[c]
        est = estimate_mean_variance(build_infill_matrices(cp, "tmin", [sid], np.isfinite(mean[:, 0]), None, 3))
        assert res.em_mean[t].tobytes() == est.mean[0].tobytes(), sid
        assert res.em_variance[t].tobytes() == est.variance[0].tobytes(), sid
        assert np.array_equal(res.em_status[t], est.status[0])
        m2, v2 = mean.copy(), vari.copy()
        m2[c], v2[c] = est.mean[0], est.variance[0]
        d = infill_daily(cp, "tmin", [sid], m2, v2, ppca_varyexplain=VARYEXPLAIN, chk_perf=True)
        for k in ("status", "matrix_status", "attempt", "nattempts", "npcs", "ncols", "nonoptimal", "reasons"):
            assert np.array_equal(getattr(res.daily, k)[t], getattr(d, k)[0]), (sid, k)
        assert res.daily.infill_tair[t].tobytes() == d.infill_tair[0].tobytes(), sid
        assert res.infill_tair[t][held[t]].tobytes() == d.infill_tair[0][held[t]].astype(np.float32).tobytes(), sid
    # off the held days both series are NaN, on them the observation is the pool's
    assert np.array_equal(np.isnan(res.obs_tair), ~held)
    assert np.array_equal(np.isnan(res.infill_tair), ~held)
    for t, c in enumerate(cols):
        assert np.array_equal(res.obs_tair[t][held[t]], pool.tmin[held[t], c])
    w = XC.want_score(res.daily.infill_tair, np.ascontiguousarray(pool.tmin.T[cols]), held,
                      (np.asarray(pool.days[MONTH]) - 1).astype(np.int8))
    assert np.array_equal(res.n, w[0][:, 12]) and np.array_equal(res.month_n, w[0][:, :12])
    assert np.allclose(res.bias, w[1][:, 12], rtol=0, atol=1e-12) and np.allclose(res.mae, w[2][:, 12], rtol=0, atol=1e-12)
    assert np.allclose(res.month_mae, w[2][:, :12], rtol=0, atol=1e-12)
    print("MAE %s BIAS %s" % (np.round(res.mae, 3), np.round(res.bias, 3)))


def test_run_xval_equals_its_row_of_run_all(chain):
    pool, mean, vari, xv, res = chain
    for t in (1, 3):
        o, f = xv.run_xval(xv.stn_ids[t])
        assert o.tobytes() == res.obs_tair[t].tobytes() and f.tobytes() == res.infill_tair[t].tobytes()
    with pytest.raises(KeyError):
        xv.run_xval(pool.ids[0])


# ---- 6. the command line ----
from spatial_cases import FORMATS  # noqa: E402


@pytest.fixture(scope="module")
def step15_inputs(tmp_path_factory, chain):
    pool, mean, vari, xv, res = chain
    d = tmp_path_factory.mktemp("step15")
    normals = str(d / "normals.npz")
    np.savez(normals, ids=pool.ids, mean_tmin=mean, variance_tmin=vari, mean_tmax=mean + 10.0, variance_tmax=vari)
    idfile = str(d / "ids.txt")
    with open(idfile, "w") as f:
        f.write("\n".join(xv.stn_ids) + "\n")
    return d, normals, idfile


@pytest.mark.parametrize("fmt", FORMATS)
def test_step15_command_line(fmt, step15_inputs, chain, capsys):
    from topowx_amd import ncio, step15
    from topowx_amd import stationdb as sdb
    pool, mean, vari, xv, res = chain
    d, normals, idfile = step15_inputs
    n = pool.ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = pool.ids, pool.lon, pool.lat, 1000.0
    db = str(d / ("all_%s.nc" % fmt))
    ncio.create_quick_db(db, stns, pool.days, [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                                               ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")], format=fmt)
    ds = ncio.open_dataset(db, "a")
    for name, a in (("tmin", pool.tmin), ("tmax", pool.tmax)):
        v = ds.variables[name]
        v.missing_value = np.float32(ncio.FILL_F4)
        v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
    ds.close()
    out, rep = str(d / ("xval_%s.nc" % fmt)), str(d / ("xval_%s.npz" % fmt))
    rc = step15.main(["--db", db, "--normals", normals, "--xval-stnids", idfile, "--out", out, "--report", rep,
                      "--ntrain-yrs", str(XC.FACADE_NTRAIN_YRS), "--ppca-varyexplain", str(VARYEXPLAIN), "--format", fmt])
    text = capsys.readouterr().out
    assert rc == 0
    line = json.loads([k for k in text.splitlines() if k.startswith("{")][-1])
    assert line["stations"] == len(xv.stn_ids) and line["step"] == "step15_xval_infill" and line["nkeep"] == 730
    assert line["tmin"]["held"] == int(res.nheld.sum()) and line["tmin"]["scored"] == int(res.n.sum())
    assert text.count("MAE: ") == 2 * len(xv.stn_ids)
    assert "WRITER|%s|tmin|MAE: %.2f|BIAS: %.2f" % (xv.stn_ids[0], res.mae[0], res.bias[0]) in text
    assert ncio.file_format(out) == fmt
    z = np.load(rep)
    assert np.array_equal(z["mae_tmin"], res.mae) and np.array_equal(z["held_tmin"], res.held)
    assert z["ids"].tolist() == list(xv.stn_ids)
    ds = ncio.open_dataset(out, "r")
    try:
        assert list(ncio._read_ids(ds.variables["station_id"])) == list(xv.stn_ids)
        fill = np.float32(ncio.FILL_F4)
        for name, want in (("obs_tmin", res.obs_tair), ("infilled_tmin", res.infill_tair)):
            raw = np.asarray(np.ma.getdata(ds.variables[name][:]), np.float32)
            assert raw.shape == want.T.shape and ds.variables[name].dtype == np.float32
            assert np.array_equal(raw == fill, np.isnan(want.T)), name                 # fill values where NaN was
            assert raw[raw != fill].tobytes() == want.T[~np.isnan(want.T)].tobytes(), name
        for v in ("tmin", "tmax"):
            o = np.asarray(np.ma.getdata(ds.variables["obs_" + v][:]), np.float32)
            f = np.asarray(np.ma.getdata(ds.variables["infilled_" + v][:]), np.float32)
            assert np.array_equal(o == fill, f == fill) and np.array_equal(o != fill, z["held_" + v].T & (f != fill))
            assert (o != fill).sum() == z["n_" + v].sum() > 0
    finally:
        ds.close()
    # an unknown id: exit status 1
    bad = str(d / "bad_ids.txt")
    with open(bad, "w") as f:
        f.write("%s\nNOBODY\n" % xv.stn_ids[0])
    assert step15.main(["--db", db, "--normals", normals, "--xval-stnids", bad, "--out", str(d / "x.nc")]) == 1
    assert step15.main(["--db", str(d / "missing.nc"), "--normals", normals, "--xval-stnids", idfile,
                        "--out", str(d / "x.nc")]) == 1


# ---- the executed reference (tests/golden/make_golden_xvalinfill.py) ----
def test_golden_masks_and_lists_of_both_stages():
    """The hold-out and, from ONE batched call per stage, the ranked stations of every cross-validation station and month
    equal the executed reference's (``_InfillMatrix`` / ``InfillMatrixPPCA`` under ``tair_mask``): stations, nnghs and max_dist
    exactly, ioa within the 1e-10 of DESIGN.md section 16."""
    from topowx_amd.infill import XvalInfill, build_infill_matrices
    from topowx_amd.infill.infill_daily import month_mask_groups
    from topowx_amd.qa import StationObsPool
    gold = XC.load_gold()
    ids, lon, lat, tmin, days = XC.gold_case(gold)
    pool = StationObsPool(ids, lon, lat, tmin, tmin + 10, days)
    xval = gold["xval"]
    xv = XvalInfill(pool, "tmin", None, gold["mean"], gold["vari"], ids[xval], float(gold["ntrain_yrs"]))
    assert xv.nkeep == int(gold["nkeep"]) and np.array_equal(xv.stn_xval_masks, XC.gold_held(gold))
    ext, app_ids, cols, never = xv.extended_pool()
    nx = len(xval)
    month = np.asarray(days[MONTH]) - 1

    def compare(m, stage, months, renumbered):
        worst = 0.0
        for t in range(nx):
            off, idx, ioa, dist, nnghs, maxd = XC.gold_lists(gold, stage, t)
            for g in months:
                k = renumbered[g]
                r = m.ranked(t, k)
                a = slice(off[g], off[g + 1])
                assert m.status[t, k] == _qalib.IF_OK and np.array_equal(r["idx"], idx[a]), (stage, t, g)
                assert m.nnghs[t, k] == nnghs[g] and m.max_dist[t, k] == maxd[g], (stage, t, g)
                worst = max(worst, float(np.abs(r["ioa"] - ioa[a]).max()))
        return worst
    m1 = build_infill_matrices(ext, "tmin", app_ids, np.concatenate([xv.ngh_stn_mask, np.zeros(nx, bool)]), None, 3,
                               exclude_cols=cols, never_neighbour=never)
    worst = compare(m1, 1, range(12), {g: g for g in range(12)})
    mean = np.concatenate([gold["mean"], [gold["entered_mean_%d" % t] for t in range(nx)]])
    vari = np.concatenate([gold["vari"], [gold["entered_vari_%d" % t] for t in range(nx)]])
    groups = month_mask_groups(mean, vari, never)
    assert len(groups) == len(month_mask_groups(gold["mean"], gold["vari"])) > 1
    for mask, months in groups:
        grp = np.where(np.isin(month, months), month, -1).astype(np.int8)
        m2 = build_infill_matrices(ext, "tmin", app_ids, mask, grp, 3, exclude_cols=cols, never_neighbour=never)
        worst = max(worst, compare(m2, 2, months, {g: g for g in months}))
    print("max |ioa - golden| %.3g" % worst)
    assert worst <= 1e-10
