"""CPU: step20's outlier screen without a GPU -- the numpy restatement against the executed-reference golden
(tests/golden/make_golden_outlier.py), the z-score rule, ``set_bad_stations`` on both containers, and the hash of the
kernel sources libtwxqa must not change."""
import datetime as dt
import os
import sys

import numpy as np
import pytest

from topowx_amd import ncio, synth
from topowx_amd import stationdb as sdb
from topowx_amd.dates import get_days_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
VARS = ("tmin", "tmax")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_outlier_v1.npz"))


@pytest.fixture(scope="module")
def cases(gold):
    import make_golden as mg
    import make_golden_outlier as mgo
    grid, tmin, tmax = mg.case_inputs()
    assert mg.input_hash(grid, tmin, tmax) == str(gold["input_hash"])
    out = {}
    for var, da in (("tmin", tmin), ("tmax", tmax)):
        db, _ = mgo.perturbed(da, var)
        assert mg.sha(np.frombuffer(db.stns.tobytes(), np.uint8)) == str(gold["stns_hash_" + var])
        out[var] = db
    return out


@pytest.mark.parametrize("var", VARS)
def test_restatement_matches_golden(gold, cases, orc, var):
    import outlier_restatement as R
    errs, st = R.xval_errs(orc, cases[var], k=int(gold["bw_nngh"]))
    want = gold["errs_" + var]
    assert (st == 0).all()
    assert np.array_equal(np.isnan(errs), np.isnan(want))
    assert np.nanmax(np.abs(errs - want)) < 1e-9
    # the perturbation shows where it should: the NaN-lst month of that station and nowhere else
    db = cases[var]
    r = db.stn_idxs[str(gold["nan_lst_id_" + var])]
    assert np.argwhere(np.isnan(want)).tolist() == [[int(gold["nan_lst_mth_" + var]) - 1, r]]


@pytest.mark.parametrize("var", VARS)
def test_outlier_ids_reproduce_golden(gold, cases, var):
    from topowx_amd.interp.optimize import outlier_ids
    db = cases[var]
    errs = gold["errs_" + var]
    thr = float(gold["threshold"])
    got = outlier_ids(errs, db.stn_ids, thr)
    assert got.tolist() == gold["out_all_" + var].tolist()
    good = np.isnan(db.stns[sdb.BAD])
    assert outlier_ids(errs[:, good], db.stn_ids[good], thr).tolist() == gold["out_good_" + var].tolist()
    # the planted stations are what the screen finds
    assert sorted(got.tolist()) == sorted(gold["planted_ids_" + var].tolist())


def test_outlier_ids_pandas_edge_cases():
    from topowx_amd.interp.optimize import outlier_ids
    ids = np.array(["a", "b", "c", "d", "e", "f", "g", "h"])
    e = np.zeros((13, 8))
    e[:] = np.linspace(-1, 1, 8)
    e[4, 5] = 40.0                    # one target far out
    e[7, :] = np.nan                  # a target without a value: never an outlier
    e[9, 2] = np.nan                  # NaN skipped in mean and std
    e[11, :7] = np.nan                # one value: std NaN (ddof=1) -> no z-score
    e[12, :] = 3.0                    # zero spread: 0 / 0 -> NaN, not an outlier
    assert outlier_ids(e, ids, 2.0).tolist() == ["f"]
    assert outlier_ids(e, ids, 100.0).tolist() == []
    with pytest.raises(ValueError):
        outlier_ids(e, ids[:3], 2.0)


def _db(n=40):
    days = get_days_metadata(dt.date(1981, 1, 1), dt.date(1981, 1, 10))
    return synth.make_stations((40.0, 42.0, -110.0, -108.0), n, 5, "tmin", days, with_obs=True)


def _flags(path):
    da = sdb.StationSerialDataDb(path, "tmin")
    try:
        return sorted(da.stn_ids[~np.isnan(da.stns[sdb.BAD])].tolist())
    finally:
        da.close()


@pytest.mark.parametrize("fmt", ncio.FORMATS)
def test_set_bad_stations_round_trip(tmp_path, fmt):
    from topowx_amd.step20 import set_bad_stations
    if fmt == "NETCDF4" and ncio.default_format() != "NETCDF4":
        pytest.skip("libhdf5 not loadable here")
    db = _db()
    ids = db.stn_ids
    path = str(tmp_path / ("serial_tmin_%s.nc" % fmt))
    ncio.write_station_db(path, db, format=fmt)
    assert _flags(path) == []
    da = sdb.StationSerialDataDb(path, "tmin", mode="r+")
    set_bad_stations(da, [ids[3], "NOT_AN_ID", ids[7]], reset=False)     # unknown ids are ignored
    assert sorted(da.stn_ids[~np.isnan(da.stns[sdb.BAD])].tolist()) == [ids[3], ids[7]]   # the table follows
    da.close()
    assert _flags(path) == [ids[3], ids[7]]
    da = sdb.StationSerialDataDb(path, "tmin", mode="r+")
    set_bad_stations(da, [ids[11]], reset=False)
    da.close()
    assert _flags(path) == [ids[3], ids[7], ids[11]]
    da = sdb.StationSerialDataDb(path, "tmin", mode="r+")
    set_bad_stations(da, [ids[1]], reset=True)
    da.close()
    assert _flags(path) == [ids[1]]
    # an open dataset, as the reference passes ``stnda.ds``
    ds = ncio.open_dataset(path, "a")
    set_bad_stations(ds, np.array([ids[2], "ZZZ"]), reset=False)
    ds.close()
    assert _flags(path) == [ids[1], ids[2]]
    ds = ncio.open_dataset(path, "a")
    set_bad_stations(ds, [], reset=True)
    ds.close()
    assert _flags(path) == []


@pytest.mark.parametrize("fmt", ncio.FORMATS)
def test_set_bad_stations_creates_flag(tmp_path, fmt):
    """A database without a ``bad`` variable gets the reference's i1 flag (fill 0 = okay)."""
    from topowx_amd.step20 import set_bad_stations
    if fmt == "NETCDF4" and ncio.default_format() != "NETCDF4":
        pytest.skip("libhdf5 not loadable here")
    db = _db(12)
    names = [n for n in db.stns.dtype.names if n != sdb.BAD]
    stns = np.empty(db.stns.size, [(n, db.stns.dtype[n]) for n in names])
    for n in names:
        stns[n] = db.stns[n]
    path = str(tmp_path / ("nobad_%s.nc" % fmt))
    ncio.write_station_db(path, sdb.StationSerialDataDb(stns, "tmin", db.days, db.var), format=fmt)
    da = sdb.StationSerialDataDb(path, "tmin", mode="r+")
    set_bad_stations(da, [db.stn_ids[4]])
    da.close()
    assert _flags(path) == [db.stn_ids[4]]
    ds = ncio.open_dataset(path, "r")
    try:
        assert np.dtype(ds.variables[sdb.BAD].dtype) == np.int8
    finally:
        ds.close()


def test_in_memory_set_bad_stations():
    from topowx_amd.step20 import set_bad_stations
    db = _db(10)
    set_bad_stations(db, [db.stn_ids[2], "X"], reset=False)
    assert np.nonzero(~np.isnan(db.stns[sdb.BAD]))[0].tolist() == [2]
    set_bad_stations(db, [db.stn_ids[5]])
    assert np.nonzero(~np.isnan(db.stns[sdb.BAD]))[0].tolist() == [5]


def test_step20_cli_refuses_unopenable_and_unsorted(tmp_path, capsys):
    from topowx_amd import step20
    db = _db(10)
    good = str(tmp_path / "ok.nc")
    ncio.write_station_db(good, db, format="NETCDF3_64BIT")
    assert step20.main(["--tmin", str(tmp_path / "missing.nc"), "--tmax", good]) == 1
    bad = str(tmp_path / "unsorted.nc")
    ncio.write_station_db(bad, db, format="NETCDF3_64BIT")
    ds = ncio.open_dataset(bad, "a")                     # ids in descending order: not a sorted station table
    ds.variables[sdb.STN_ID][:] = ds.variables[sdb.STN_ID][:][::-1]
    ds.close()
    assert step20.main(["--tmin", good, "--tmax", bad, "--dry-run"]) == 1
    assert "cannot open" in capsys.readouterr().err


def test_xvaloutlier_not_exported():
    import topowx_amd.interp as ti
    from topowx_amd.interp import optimize
    assert hasattr(optimize, "XvalOutlier") and "XvalOutlier" not in ti.__all__ and not hasattr(ti, "XvalOutlier")


def test_qa_library_is_built_with_its_kernel():
    """build.sh writes libtwxqa.so and its resource table (no build in this checkout: skipped, as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    import ctypes
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.EXPORTS:
        assert hasattr(lib, name)
    import isa_resources
    table = isa_resources.parse(res)
    assert "k_outlier_wls" in table


def test_qa_header_matches_binding():
    import re
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxqa_\w+)\s*\(", h))) == sorted(_qalib.EXPORTS)
    for name, val in (("TWXQA_NTARGET", _qalib.NTARGET), ("TWXQA_PT_STRIDE", _qalib.PT_STRIDE),
                      ("TWXQA_MAX_K", _qalib.MAX_K)):
        assert re.search(r"#define %s %d\b" % (name, val), h), name


def test_kernel_sources_hash_unchanged():
    """libtwxqa lives outside topowx_amd/csrc and include/twx.h: the hash the committed profiles carry still holds."""
    import kernel_hash
    assert kernel_hash.kernel_sources_sha16() == "051aca46034c8c88"      # (rcp_nr1's second Newton step: twx_vario.h)
