"""GPU: step05 / step09-11 -- the kernels of ``twxhm_obs_cnt``, ``twxhm_monthly_means``, ``twxhm_tobs_shift`` and
``twxhm_homog_daily`` against the executed-reference golden (tests/golden/make_golden_homog.py) and, on seeded shapes, against
the numpy restatement (tests/restate_homog.py) the maker proved bit-equal to the reference; then the Python layer and the
four command lines end to end through temporary files in both containers.

Every comparison is exact: integers equal, float32 and float64 outputs BIT FOR BIT, NaN positions included.  ``delta`` has
no counterpart in the reference (it adds month by month); the fixture's is the restatement's, whose homogenised days the
maker compared with the reference's.
"""
import datetime as dt
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import homog_cases as HC  # noqa: E402
import restate_homog as RH  # noqa: E402

from topowx_amd import _qalib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return HC.load_fixture()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
    bad = got.view(u) != want.view(u)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def run_all(c, workspace_bytes=0, first_day=None, last_day=None):
    """The four entries on a case of ``HC.random_case``'s keys."""
    nd = c["obs"].shape[1]
    a, b = (0 if first_day is None else first_day), (nd - 1 if last_day is None else last_day)
    tm = {}
    out = dict(cnt=_qalib.obs_cnt(c["obs"], c["month"], a, b, workspace_bytes=workspace_bytes, timing=tm))
    out["mean"], out["miss"] = _qalib.monthly_means(c["obs"], c["mth_first"], c["mth_ndays"], 9, workspace_bytes=workspace_bytes,
                                                    timing=tm)
    out["shift"], out["nshift"] = _qalib.tobs_shift(c["obs"], c["tobs"], workspace_bytes=workspace_bytes, timing=tm)
    out.update(_qalib.homog_daily(c["obs"], c["mth_mean"], c["mth_miss"], c["pha"], c["mth_ymd"], c["mth_first"],
                                  c["mth_ndays"], c["adj_off"], c["adj_start"], c["adj_end"], c["adj"],
                                  workspace_bytes=workspace_bytes, timing=tm))
    times = [k + "_kernel_ms" for k in _qalib.HM_KERNELS] + ["hm_upload_ms", "hm_download_ms"]
    assert tm["hm_calls"] == 4 and all(np.isfinite(tm[k]) and tm[k] >= 0 for k in times), tm
    return out


def want_all(c, first_day=None, last_day=None):
    nd = c["obs"].shape[1]
    a, b = (0 if first_day is None else first_day), (nd - 1 if last_day is None else last_day)
    out = dict(cnt=RH.obs_cnt(c["obs"], c["month"], a, b))
    out["mean"], out["miss"] = RH.monthly_means(c["obs"], c["mth_first"], c["mth_ndays"], 9)
    out["shift"], out["nshift"] = RH.tobs_shift(c["obs"], c["tobs"])
    out.update(RH.homog_daily(c["obs"], c["mth_mean"], c["mth_miss"], c["pha"], c["mth_ymd"], c["mth_first"], c["mth_ndays"],
                              c["adj_off"], c["adj_start"], c["adj_end"], c["adj"]))
    return out


def same_all(got, want, what):
    for k in ("cnt", "miss", "nshift", "status", "nchanged", "mean", "shift", "delta", "out"):
        same_bits(got[k], want[k], (what, k))


def test_fixture_every_station(gold):
    nd = gold["year"].size
    for v in ("tmin", "tmax"):
        same_bits(_qalib.obs_cnt(gold["raw_" + v], gold["month"], 0, nd - 1), gold["cnt_" + v], "cnt_" + v)
    shifted, nshift = _qalib.tobs_shift(gold["obs_tmax"], gold["tobs"])
    same_bits(shifted, gold["tobs_tmax"], "shifted tmax")
    same_bits(nshift, gold["tobs_nshift"], "nshift")
    assert set(nshift.tolist()) >= {0, 1, 2}
    again = _qalib.tobs_shift(gold["obs_tmax"], gold["tobs"])
    assert again[0].tobytes() == shifted.tobytes() and again[1].tobytes() == nshift.tobytes()
    fids = gold["fmt_ids"]
    for v, rows in (("tmin", gold["obs_tmin"]), ("tmax", gold["tobs_tmax"])):
        mean, miss = _qalib.monthly_means(rows, gold["mth_first"], gold["mth_ndays"], 9)
        same_bits(mean, gold["mth_mean_" + v], "mth_mean_" + v)
        same_bits(miss, gold["mth_miss_" + v], "mth_miss_" + v)
        m2, s2 = _qalib.monthly_means(rows, gold["mth_first"], gold["mth_ndays"], 9)
        assert m2.tobytes() == mean.tobytes() and s2.tobytes() == miss.tobytes()
        off, st, en, ad = HC.adj_csr(fids, gold["adj_ids_" + v], gold["adj_start_" + v], gold["adj_end_" + v], gold["adj_" + v])
        args = (rows, gold["mth_mean_" + v], gold["mth_miss_" + v], gold["pha_" + v], gold["mth_ymd"], gold["mth_first"],
                gold["mth_ndays"], off, st, en, ad)
        r = _qalib.homog_daily(*args)
        assert (r["status"] == _qalib.HM_OK).all()
        same_bits(r["nchanged"], gold["nchanged_" + v], "nchanged_" + v)
        same_bits(r["delta"], gold["delta_" + v], "delta_" + v)
        same_bits(r["out"], gold["homog_" + v], "homog_" + v)
        r2 = _qalib.homog_daily(*args)
        assert all(r2[k].tobytes() == r[k].tobytes() for k in ("delta", "out", "status", "nchanged"))
    # the max_miss of None
    mean, miss = _qalib.monthly_means(gold["obs_tmin"], gold["mth_first"], gold["mth_ndays"], None)
    want = RH.monthly_means(gold["obs_tmin"], gold["mth_first"], gold["mth_ndays"], None)
    same_bits(mean, want[0], "mean, no threshold")
    assert np.isnan(mean).sum() < np.isnan(gold["mth_mean_tmin"]).sum()


SHAPES = [(1, dt.date(1980, 2, 1), dt.date(1980, 2, 28)),            # 28 days, one month
          (2, dt.date(1981, 1, 1), dt.date(1981, 2, 28)),            # 59 days
          (50, dt.date(1980, 1, 1), dt.date(1980, 12, 31)),          # 366 days
          (51, dt.date(1979, 1, 1), dt.date(1984, 12, 31)),          # the six-year axis
          (257, dt.date(1983, 3, 5), dt.date(1985, 2, 3))]           # starting and ending inside a month


@pytest.mark.parametrize("ns,start,end", SHAPES, ids=["1x28", "2x59", "50x366", "51x2192", "257x702"])
def test_seeded_shapes(ns, start, end):
    c = HC.random_case(100 + ns, ns, start, end)
    nd = c["obs"].shape[1]
    want = want_all(c)
    got = run_all(c)
    same_all(got, want, "one batch")
    small = run_all(c, workspace_bytes=3 * nd * 12 + 5)                # three stations a batch in the widest entry
    same_all(small, want, "small batches")
    if nd > 40:
        same_bits(_qalib.obs_cnt(c["obs"], c["month"], 17, nd - 9), RH.obs_cnt(c["obs"], c["month"], 17, nd - 9), "window")
    assert (want["status"] == 0).all()
    assert ns == 1 or want["nshift"][1] == 1
    if ns in (50, 257):
        assert (np.diff(c["adj_off"]) == 0).any()                     # an empty list on a station that never needs it


def test_all_nan_rows_and_one_station_a_batch():
    c = HC.random_case(7, 5, dt.date(1979, 1, 1), dt.date(1984, 12, 31))
    c["obs"][1] = np.nan
    c["obs"][4] = np.nan
    c["mth_mean"], c["mth_miss"] = RH.monthly_means(c["obs"], c["mth_first"], c["mth_ndays"], 9)
    want = want_all(c)
    assert np.isnan(want["mean"][1]).all() and (want["cnt"][4] == 0).all()
    same_all(run_all(c), want, "all-NaN rows")
    same_all(run_all(c, workspace_bytes=1), want, "one station a batch")


def test_bad_adjustment_lists_leave_the_neighbours():
    c = HC.random_case(11, 9, dt.date(1979, 1, 1), dt.date(1984, 12, 31), bad=((2, "noadj"), (6, "overlap")))
    want = want_all(c)
    assert want["status"].tolist() == [0, 0, RH.NO_ADJ, 0, 0, 0, RH.OVERLAP, 0, 0]
    got = run_all(c)
    same_all(got, want, "bad lists")
    assert got["status"][2] == _qalib.HM_NO_ADJ and got["status"][6] == _qalib.HM_OVERLAP
    assert np.isnan(got["out"][[2, 6]]).all() and np.isnan(got["delta"][[2, 6]]).all()
    for s in (1, 3, 5, 7):
        assert not np.isnan(got["delta"][s]).all()
    same_all(run_all(c, workspace_bytes=2 * c["obs"].shape[1] * 8), want, "bad lists, small batches")


def write_all_db(gold, path, fmt):
    """The flagged all-stations database of the fixture: raw Tmin / Tmax, their quality flags, ``tobs_tmax``."""
    from topowx_amd import ncio
    from topowx_amd import stationdb as sdb
    from topowx_amd.dates import get_days_metadata
    n = gold["ids"].size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U32"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64),
                              ("station_name", "U30")])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = gold["ids"], gold["lon"], gold["lat"], gold["elev"]
    stns["station_name"] = gold["name"]
    days = get_days_metadata(HC.START, HC.END)
    ncio.create_quick_db(path, stns, days, [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                                            ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C"),
                                            ("tobs_tmax", "f4", ncio.FILL_F4, "time of observation of tmax", "hhmm"),
                                            ("qflag_tmin", "S1", "", "quality assurance flag tmin", ""),
                                            ("qflag_tmax", "S1", "", "quality assurance flag tmax", "")], format=fmt)
    with ncio.open_dataset(path, "a") as ds:
        for name, a in (("tmin", gold["raw_tmin"]), ("tmax", gold["raw_tmax"]), ("tobs_tmax", gold["tobs"])):
            ds.variables[name][:] = np.ascontiguousarray(np.where(np.isnan(a), np.float32(ncio.FILL_F4), a).T)
        for v in ("tmin", "tmax"):
            ds.variables["qflag_" + v][:] = np.where(gold["flag_" + v].T, b"X", b"").astype("S1")
    return path


@pytest.mark.parametrize("fmt", ["NETCDF4", "NETCDF3_64BIT"])
def test_end_to_end_through_files(gold, tmp_path, fmt, capsys):
    """step05 -> step09 -> step10 -> step11 --setup -> (the fixture's PHA files) -> step11 --apply, in either container."""
    import json
    import test_homog_host as TH
    from topowx_amd import homog, ncio, obs_por, step05, step09, step10, step11
    if fmt == "NETCDF4":
        from topowx_amd import h5nc
        if not h5nc.available():
            pytest.skip("libhdf5 is not available")
    db, adj, out, pha_dir = (str(tmp_path / n) for n in ("all.nc", "tobs_adj.nc", "homog.nc", "pha"))
    ids_out, hist = str(tmp_path / "ids.txt"), str(tmp_path / "hist.csv")
    write_all_db(gold, db, fmt)
    period = ["--start", "19790101", "--end", "1984-12-31"]
    assert step05.main(["--db", db, "--min-por-yrs", "5", "--ids-out", ids_out] + period) == 0
    line = json.loads(capsys.readouterr().out)
    assert line["tmin"]["obs"] == int(gold["cnt_tmin"].sum()) and line["hm_cnt_kernel_ms"] > 0
    with ncio.open_dataset(db, "r") as ds:
        for v in ("tmin", "tmax"):
            assert np.array_equal(np.asarray(ds.variables["obs_cnt_%s_19790101_19841231" % v][:]).T, gold["cnt_" + v])
            for yrs in (1, 5):
                assert np.array_equal(obs_por.build_por_mask(ds, [v], "19790101", "19841231", yrs), gold["por_%s_%d" % (v, yrs)])
    assert open(ids_out).read().split() == gold["ids"][gold["por_tmin_5"] | gold["por_tmax_5"]].tolist()
    # ---- step09 ----
    assert step09.main(["--db", db, "--out", adj, "--format", fmt] + period) == 0
    line = json.loads(capsys.readouterr().out)
    keep = np.nonzero(gold["por_tmin_1"] | gold["por_tmax_1"])[0]
    keep = keep[np.argsort(gold["ids"][keep], kind="stable")]
    assert line["stations"] == keep.size < gold["ids"].size and line["shifted"] == int((gold["tobs_nshift"][keep] > 1).sum())
    assert step09.main(["--db", db, "--out", adj] + period) == 1 and "not overwritten" in capsys.readouterr().err
    with ncio.open_dataset(adj, "r") as ds:
        assert ncio._read_ids(ds.variables["station_id"]).tolist() == gold["ids"][keep].tolist()
        got_tmin, got_tmax = obs_por.read_rows(ds, "tmin", qflags=True), obs_por.read_rows(ds, "tmax", qflags=True)
        assert float(np.ma.getdata(ds.variables["tmin"][:]).min()) == -9999.0
    want_tmin = np.where(gold["por_tmin_1"][:, None], gold["obs_tmin"], np.float32(np.nan))[keep]
    want_tmax = np.where(gold["por_tmax_1"][:, None], gold["tobs_tmax"], np.float32(np.nan))[keep]
    same_bits(got_tmin, want_tmin, "tobs_adj tmin")
    same_bits(got_tmax, want_tmax, "tobs_adj tmax")
    # ---- step10 ----
    assert step10.main(["--db", adj]) == 0
    capsys.readouterr()
    full = {"tmin": gold["por_tmin_1"][keep], "tmax": gold["por_tmax_1"][keep]}       # the others: every month wholly missing
    with ncio.open_dataset(adj, "r") as ds:
        assert ds.variables["time_mth"][:].tolist() == gold["mth_first"].astype(float).tolist()
        for v in ("tmin", "tmax"):
            mean, miss = obs_por.read_rows(ds, v + "_mth"), np.asarray(ds.variables[v + "_mthmiss"][:]).T
            same_bits(mean[full[v]], gold["mth_mean_" + v][keep][full[v]], v + "_mth")
            assert np.array_equal(miss[full[v]], gold["mth_miss_" + v][keep][full[v]]) and miss.dtype == np.int16
            assert np.isnan(mean[~full[v]]).all() and (miss[~full[v]] == gold["mth_ndays"]).all()
    # ---- step11 --setup: the input tree against the executed reference's bytes ----
    with open(hist, "w") as f:
        f.write("station_id,yyyymm\n" + "".join("%s,%s\n" % h for h in zip(gold["hist_ids"], gold["hist_yyyymm"])))
    assert step11.main(["--db", adj, "--pha-dir", pha_dir, "--setup", "--stnhist", hist]) == 0
    assert json.loads(capsys.readouterr().out)["stnhist"] == 3
    for v in ("tmin", "tmax"):
        p = homog.pha_paths(os.path.join(pha_dir, v), v)
        lines = str(gold["stnlist_" + v]).splitlines(True)
        assert open(p["stnlist"]).read() == "".join(lines[k] for k in keep)
        assert open(p["metadata"]).read() == str(gold["metadata_file"])
        for k in keep[full[v]]:
            f = gold["fmt_ids"][k]
            assert open(os.path.join(p["raw"], "%s.raw.%s" % (f, v))).read() == str(gold["raw_files_" + v][k]), (v, f)
    # ---- PHA's output dropped in, then --apply ----
    TH.drop_pha_files(gold, pha_dir)
    assert step11.main(["--db", adj, "--pha-dir", pha_dir, "--apply", "--out", out, "--format", fmt] + period) == 0
    line = json.loads(capsys.readouterr().out)
    skip = {"tmin": [7], "tmax": [8, 20]}
    with ncio.open_dataset(out, "r") as ds:
        ids = ncio._read_ids(ds.variables["station_id"])
        assert ids.tolist() == gold["ids"][keep].tolist()
        for v in ("tmin", "tmax"):
            got = obs_por.read_rows(ds, v)
            want = gold["homog_" + v].copy()
            want[~gold["por_%s_1" % v]] = np.nan
            want[skip[v]] = np.nan
            same_bits(got, want[keep], "homog " + v)
            cnt = np.asarray(ds.variables["obs_cnt_%s_19790101_19841231" % v][:]).T
            assert np.array_equal(cnt, RH.obs_cnt(want[keep], gold["month"], 0, gold["month"].size - 1))
            assert line[v]["homogenised"] == keep.size - len(skip[v]) and line[v]["obs"] == int(cnt.sum())
    # HomogDaily.homog_stn, the reference's call, is a row of the batch
    h = homog.HomogDaily(adj, os.path.join(pha_dir, "tmax"), "tmax")
    sid = gold["ids"][11]
    same_bits(h.homog_stn(sid), gold["homog_tmax"][11], "homog_stn")
    # a station whose list is missing is named
    p = homog.pha_paths(os.path.join(pha_dir, "tmin"), "tmin")
    text = [ln for ln in open(p["adj_log"]) if ln[10:21] != gold["fmt_ids"][2]]
    with open(p["adj_log"], "w") as f:
        f.writelines(text)
    with pytest.raises(ValueError, match=gold["ids"][2]):
        homog.HomogDaily(adj, os.path.join(pha_dir, "tmin"), "tmin").homog_all()
    assert step11.main(["--db", adj, "--pha-dir", pha_dir, "--apply", "--out", str(tmp_path / "h2.nc")] + period) == 1
    assert gold["ids"][2] in capsys.readouterr().err


def test_batched_tobs_shift_of_the_python_layer(gold):
    from topowx_amd.homog import tobs_shift_tmax
    same_bits(tobs_shift_tmax(gold["obs_tmax"], gold["tobs"]), gold["tobs_tmax"], "batched")
    same_bits(tobs_shift_tmax(gold["obs_tmax"][12], gold["tobs"][12]), gold["tobs_tmax"][12], "one station")
