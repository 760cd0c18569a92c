"""GPU: step20's outlier screen (``XvalOutlier`` on libtwxqa) against the executed-reference golden
(tests/golden/make_golden_outlier.py) and the numpy restatement (tests/outlier_restatement.py), its failure modes,
and the step20 driver end to end on NetCDF-4 station databases."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd import ncio, synth
from topowx_amd import stationdb as sdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

TOL = 1e-7          # degC; the formulations differ in their roundings only (~1e-11)
PLANT = {"tmin": ((100, 2, 11.0), (700, 8, -13.0), (1500, 12, 12.0)),
         "tmax": ((300, 4, 12.0), (1200, 6, -11.0), (1900, 10, 13.0))}


def planted_db(var, n=2000, seed=21, plant=None):
    """A synthetic database with one monthly normal of a few stations shifted by >= 11 degC."""
    db = synth.make_stations((40.0, 46.0, -112.0, -104.0), n, seed, var)
    for i, m, shift in (PLANT[var] if plant is None else plant):
        db.stns[sdb.get_norm_varname(m)][i] += shift
    return db


def planted_ids(db, var):
    return sorted(db.stn_ids[i] for i, _, _ in PLANT[var])


def _cmp(got, want):
    """got [n, 13] from the GPU, want [13, n]: identical NaN positions, largest difference."""
    want = np.asarray(want).T
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return float(np.nanmax(np.abs(got - want)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_outlier_v1.npz"))


@pytest.fixture(scope="module")
def cases(gold):
    import make_golden as mg
    import make_golden_outlier as mgo
    grid, tmin, tmax = mg.case_inputs()
    assert mg.input_hash(grid, tmin, tmax) == str(gold["input_hash"])
    return {var: mgo.perturbed(da, var)[0] for var, da in (("tmin", tmin), ("tmax", tmax))}


@pytest.mark.parametrize("var", ("tmin", "tmax"))
def test_golden_errs_and_ids(gold, cases, var):
    from topowx_amd.interp.optimize import XvalOutlier
    db = cases[var]
    xo = XvalOutlier(db)
    try:
        errs = xo.run_xval_many(db.stn_ids, int(gold["bw_nngh"]))
        d = _cmp(errs, gold["errs_" + var])
        print("%s: max |GPU - golden| = %.3g degC" % (var, d))
        assert d < TOL, d
        thr = float(gold["threshold"])
        assert xo.find_xval_outliers(None, int(gold["bw_nngh"]), thr).tolist() == gold["out_all_" + var].tolist()
        good = db.stn_ids[np.isnan(db.stns[sdb.BAD])]
        assert xo.find_xval_outliers(good, int(gold["bw_nngh"]), thr).tolist() == gold["out_good_" + var].tolist()
    finally:
        xo.close()


@pytest.mark.parametrize("var", ("tmin", "tmax"))
def test_synthetic_2000_against_restatement(orc, var):
    import outlier_restatement as R
    from topowx_amd.interp.optimize import XvalOutlier
    db = planted_db(var)
    want, st = R.xval_errs(orc, db)
    assert (st == 0).all()
    xo = XvalOutlier(db)
    try:
        got, gst = xo.run_xval_many(db.stn_ids, raise_on_error=False)
        assert (gst == 0).all()
        d = _cmp(got, want)
        print("%s: max |GPU - restatement| = %.3g degC over %d stations" % (var, d, db.stn_ids.size))
        assert d < TOL, d
        assert sorted(xo.find_xval_outliers().tolist()) == planted_ids(db, var)
    finally:
        xo.close()


def test_single_station_is_its_batch_row_bit_for_bit(cases):
    from topowx_amd.interp.optimize import XvalOutlier
    db = cases["tmin"]
    xo = XvalOutlier(db)
    try:
        ids = db.stn_ids
        many = xo.run_xval_many(ids)
        again = xo.run_xval_many(ids)
        assert np.array_equal(many.view(np.uint64), again.view(np.uint64))
        assert np.isfinite(xo.last_timing["wls_kernel_ms"]) and xo.last_timing["wls_kernel_ms"] >= 0
        for r in (0, 17, 95, 208, ids.size - 1):
            one = xo.run_xval_stn(ids[r])
            assert one.shape == (13,)
            assert np.array_equal(one.view(np.uint64), many[r].view(np.uint64)), ids[r]
    finally:
        xo.close()


def test_left_out_bad_station_matches_restatement(orc, cases, gold):
    import outlier_restatement as R
    from topowx_amd.interp.optimize import XvalOutlier
    db = cases["tmax"]
    bad = db.stn_ids[~np.isnan(db.stns[sdb.BAD])]
    assert bad.tolist() == sorted(gold["bad_ids_tmax"].tolist())
    want, _ = R.xval_errs(orc, db, bad)
    xo = XvalOutlier(db)
    try:
        got = xo.run_xval_many(bad)
    finally:
        xo.close()
    assert _cmp(got, want) < TOL
    assert np.isfinite(got).all()


def test_constant_lst_month_is_singular_for_that_target_only():
    from topowx_amd.interp.optimize import XvalOutlier
    db = planted_db("tmin", n=600, seed=5, plant=())
    db.stns[sdb.get_lst_varname(5)] = 3.0
    xo = XvalOutlier(db)
    try:
        err, st = xo.run_xval_many(db.stn_ids, raise_on_error=False)
        assert (st[:, 4] == 4).all() and np.isnan(err[:, 4]).all()
        others = np.delete(np.arange(13), 4)
        assert (st[:, others] == 0).all() and np.isfinite(err[:, others]).all()
        e2 = xo.run_xval_many(db.stn_ids)                       # a singular system does not raise
        assert np.array_equal(np.isnan(e2), np.isnan(err))
        out = xo.find_xval_outliers()
        assert isinstance(out, np.ndarray)
    finally:
        xo.close()


def test_too_few_stations():
    from topowx_amd.interp.optimize import XvalOutlier
    db = planted_db("tmin", n=60, seed=9, plant=())
    db.stns[sdb.BAD][:10] = 1.0                                  # 50 good stations, bw_nngh 100
    xo = XvalOutlier(db)
    try:
        with pytest.raises(IndexError):
            xo.run_xval_stn(db.stn_ids[20])
        with pytest.raises(IndexError):
            xo.find_xval_outliers()
        err, st = xo.run_xval_many(db.stn_ids, raise_on_error=False)
        assert (st == 1).all() and np.isnan(err).all()
        # a smaller neighbourhood works on the same pool
        assert np.isfinite(xo.run_xval_many(db.stn_ids, bw_nngh=30)).all()
    finally:
        xo.close()


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _step20_stage(db):
    """The table as step20 sees it: no optim_nnghs* / vario_* columns yet (steps 21 and 22 add them)."""
    drop = {namer(m) for key, namer in sdb.MONTHLY_FIELDS if key not in ("lst", "norm") for m in range(1, 13)}
    names = [n for n in db.stns.dtype.names if n not in drop]
    stns = np.empty(db.stns.size, [(n, db.stns.dtype[n]) for n in names])
    for n in names:
        stns[n] = db.stns[n]
    return sdb.StationSerialDataDb(stns, db.var_name, db.days)


def test_step20_end_to_end(tmp_path, capsys):
    from topowx_amd import step20
    if ncio.default_format() != "NETCDF4":
        pytest.fail("libhdf5 must be loadable on the GPU machine (NetCDF-4 station databases)")
    paths, want = {}, set()
    for var in ("tmin", "tmax"):
        db = planted_db(var)
        db.stns[sdb.BAD][[5, 6]] = 1.0                           # already bad before this stage: stay bad, not screened
        paths[var] = str(tmp_path / ("serial_%s.nc" % var))
        ncio.write_station_db(paths[var], _step20_stage(db), format="NETCDF4")
        want |= set(planted_ids(db, var))
    before = {v: _sha(p) for v, p in paths.items()}
    argv = ["--tmin", paths["tmin"], "--tmax", paths["tmax"], "--nnghs", "100", "--zscore", "6"]
    assert step20.main(argv + ["--dry-run"]) == 0
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines()]
    assert [r["var"] for r in lines] == ["tmin", "tmax"] and all(r["stations"] == 1998 for r in lines)
    assert set(lines[0]["outliers"]) | set(lines[1]["outliers"]) == want
    assert {v: _sha(p) for v, p in paths.items()} == before      # --dry-run writes nothing
    assert step20.main(argv) == 0
    capsys.readouterr()
    for var in ("tmin", "tmax"):
        da = sdb.StationSerialDataDb(paths[var], var)
        try:
            flagged = set(da.stn_ids[~np.isnan(da.stns[sdb.BAD])].tolist())
        finally:
            da.close()
        assert flagged == want | {"S0000005", "S0000006"}, var
