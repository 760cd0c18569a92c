"""GPU: step19 and the front of step20 -- the kernels of ``twxrv_sample``, ``twxrv_nearest_data``, ``twxrv_dup_classes`` and
``twxrv_col_count`` against the executed-reference golden (tests/golden/make_golden_stnrast.py) and the numpy restatement
(tests/restate_stnrast.py), through the bindings, the Python layer and the two command lines.

Statuses, rows / columns, rings and winner slots are exact.  Values are the same fp64 expressions without contraction, so they
are compared bit for bit: each test prints how many are not and expects 0.  Ring distances: the device's sin / cos / asin /
sqrt are not numpy's; each is within 1-2 ulp and the formula's condition is benign at these separations, and the issue
allows 4 ulp of numpy's result.  Counts and classes are integers.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_stnrast as RR  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = {"lst": (1, True, True), "tdi": (1, True, False), "cell": (0, False, False)}


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_stnrast_v1.npz"))


def _runs(G):
    for name in G["cases"]:
        for combo in G["combos"]:
            if "%s_%s_value" % (name, combo) in G.files:
                yield str(name), str(combo)


def _times_ok(t, kernel):
    """The times an entry reported: its kernel's and the two host-clock ones, each finite and not negative."""
    return all(np.isfinite(t[k]) and t[k] >= 0 for k in (kernel + "_kernel_ms", "rv_upload_ms", "rv_download_ms"))


def test_sample_and_ring_against_the_golden(G):
    from topowx_amd import _qalib
    assert (_qalib.RV_OK, _qalib.RV_NEAREST, _qalib.RV_NODATA, _qalib.RV_NEEDS_FORCE, _qalib.RV_NO_DATA_ANYWHERE) == \
        (RR.OK, RR.NEAREST, RR.NODATA, RR.NEEDS_FORCE, RR.NO_DATA_ANYWHERE)
    nruns = nbits = nforced = nguard = 0
    worst = 0.0
    for name, combo in _runs(G):
        method, revert, force = COMBOS[combo]
        data, geo_t = G[name + "_data"], G[name + "_geo_t"]
        band, ndata = float(G[name + "_band_ndata"]), float(G[name + "_ndata"])
        if name == "mask":
            ndata = 0.0                                               # step19 reassigns it; the band keeps masking 255
        sel = G["%s_%s_sel" % (name, combo)]
        lon, lat = G[name + "_lon"][sel], G[name + "_lat"][sel]
        want = {k: G["%s_%s_%s" % (name, combo, k)] for k in ("value", "status", "row", "col", "forced", "ring_value", "ring_dist",
                                                               "ring_r", "ring_winner", "ring_runner_up")}
        tm = {}
        got = _qalib.raster_sample(data, geo_t, ndata, lon, lat, band_ndata=band, extract_method=method, revert_nn=revert,
                                   force_data_value=force, timing=tm)
        what = (name, combo)
        assert _times_ok(tm, _qalib.RV_KERNELS[0]), (what, tm)
        assert np.array_equal(got["status"], want["status"]), (what, "status", np.nonzero(got["status"] != want["status"])[0])
        assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["col"], want["col"]), (what, "row / col")
        forced = np.nonzero(got["status"] == _qalib.RV_NEEDS_FORCE)[0]
        assert np.array_equal(forced, want["forced"]), (what, "forced")
        value = got["value"].copy()
        if forced.size:
            nn = _qalib.raster_nearest_data(data, geo_t, ndata, got["row"][forced], got["col"][forced], timing=tm)
            assert (nn["status"] == _qalib.RV_OK).all() and _times_ok(tm, _qalib.RV_KERNELS[1]), (what, tm)
            assert np.array_equal(nn["ring"], want["ring_r"]), (what, "ring", nn["ring"], want["ring_r"])
            assert np.array_equal(nn["winner"], want["ring_winner"]), (what, "winner")
            assert nn["value"].tobytes() == want["ring_value"].tobytes(), (what, "ring value")
            for k in ("dist", "runner_up"):
                w = want["ring_" + k]
                fin = np.isfinite(w)
                assert np.array_equal(np.isfinite(nn[k]), fin), (what, k)
                ulps = np.abs(nn[k][fin] - w[fin]) / np.spacing(w[fin])
                worst = max(worst, float(ulps.max()) if ulps.size else 0.0)
                assert (ulps <= 4).all(), (what, k, float(ulps.max()))
            nguard += nn["redecided"]
            value[forced] = nn["value"]
            nforced += forced.size
        nbits += int((value.view(np.uint64) != want["value"].view(np.uint64)).sum())
        nruns += 1
    print("%d runs, %d forced stations, %d values not bit-equal to the golden, largest distance error %.2f ulp, "
          "%d stations inside the tie guard" % (nruns, nforced, nbits, worst, nguard))
    assert nruns == 13 and nforced > 60
    assert nbits == 0
    assert nguard == 0                                                # the golden has no station inside the tie guard


def test_constructed_near_tie_is_decided_on_the_host():
    """A one-cell hole: the cells left and right of it are equally far to within rounding.  The device and numpy may order
    them differently; the binding decides such a station again with numpy on the same ring and says so."""
    from topowx_amd import _qalib
    rs = np.random.RandomState(5)
    data = rs.uniform(270, 300, (40, 70)).astype(np.float32)
    geo_t = (-111.0, 1.0 / 120, 0.0, 46.0, 0.0, -1.0 / 120)
    starts = [(9, 13), (20, 31), (33, 60), (5, 5)]
    for r, c in starts[:3]:
        data[r, c] = -9999.0
    data[4:7, 4:7] = -9999.0
    data[5, 7] = -9999.0                                              # (5, 5): ring 2, cells (5, 3) left and ... none right
    row, col = np.array([s[0] for s in starts], np.int32), np.array([s[1] for s in starts], np.int32)
    nn = _qalib.raster_nearest_data(data, geo_t, -9999.0, row, col)
    grid = RR.Grid(data, geo_t, -9999.0)
    for p, (r, c) in enumerate(starts):
        want = RR.find_nn_data(data, grid, c, r)
        assert nn["ring"][p] == want["ring"] and nn["winner"][p] == want["winner"], (p, nn["winner"][p], want)
        assert nn["value"][p] == want["value"] and nn["dist"][p] == want["dist"], (p, "the host's decision is numpy's")
    assert nn["redecided"] == 3, nn["redecided"]
    assert nn["runner_up"][3] - nn["dist"][3] > 1e-3 * nn["runner_up"][3]


def test_ring_cap_and_no_data_anywhere():
    from topowx_amd import _qalib
    data = np.full((5, 9), -1.0)
    data[0, :] = 3.0                                                  # data only where the reference never looks
    data[:, 0] = 4.0
    nn = _qalib.raster_nearest_data(data, (0.0, 1.0, 0.0, 5.0, 0.0, -1.0), -1.0, [2, 4], [4, 8])
    assert (nn["status"] == _qalib.RV_NO_DATA_ANYWHERE).all() and (nn["winner"] == -1).all() and (nn["ring"] == 0).all()
    assert (nn["value"] == -1.0).all() and np.isinf(nn["dist"]).all()
    data[4, 8] = 7.0                                                  # ring 4 from (2, 4): beyond rows, within the cap
    nn = _qalib.raster_nearest_data(data, (0.0, 1.0, 0.0, 5.0, 0.0, -1.0), -1.0, [2], [4])
    want = RR.find_nn_data(data, RR.Grid(data, (0.0, 1.0, 0.0, 5.0, 0.0, -1.0), -1.0), 4, 2)
    assert nn["status"][0] == 0 and nn["ring"][0] == want["ring"] == 4 and nn["winner"][0] == want["winner"]
    assert nn["value"][0] == 7.0


def test_sample_refusals():
    from topowx_amd import _qalib
    a = np.ones((3, 3), np.float32)
    with pytest.raises(ValueError, match="2"):
        _qalib.raster_sample(np.ones((1, 5)), (0, 1, 0, 1, 0, -1), -1.0, [0.5], [0.5])
    with pytest.raises(ValueError, match="rotated"):
        _qalib.raster_sample(a, (0, 1, 0.1, 1, 0, -1), -1.0, [0.5], [0.5])
    with pytest.raises(ValueError, match="north-up"):
        _qalib.raster_sample(a, (0, 1, 0, 1, 0, 1), -1.0, [0.5], [0.5])
    with pytest.raises(ValueError, match="non-finite"):
        _qalib.raster_sample(a, (0, 1, 0, 3, 0, -1), -1.0, [np.nan], [0.5])
    # an integer raster is converted to the float format that holds it exactly
    big = np.array([[2 ** 24 + 1, 5], [7, 2 ** 30 + 3]], np.int32)
    got = _qalib.raster_sample(big, (0, 1, 0, 2, 0, -1), -1.0, [0.5, 1.5], [1.5, 0.5], extract_method=0)
    assert got["value"].tolist() == [2.0 ** 24 + 1, 2.0 ** 30 + 3]


@pytest.mark.parametrize("nstn", [1, 2, 63, 64, 65, 257])
def test_dup_classes(nstn, G):
    from topowx_amd import _qalib
    rs = np.random.RandomState(nstn)
    lon, lat = rs.uniform(-120, -70, nstn), rs.uniform(25, 50, nstn)
    if nstn >= 2:
        lon[-1], lat[-1] = lon[0], lat[0]                             # the first and the last station in one class
    if nstn >= 63:
        lon[40], lat[40] = lon[7], lat[7]
        lon[11], lat[11] = np.nan, lat[7]                             # NaN equals nothing, itself included
        lat[12] = np.nan
        lon[13], lat[13] = np.nan, np.nan
        lon[14], lat[14] = np.nan, np.nan
    if nstn >= 257:
        lon[255], lat[255] = lon[100], lat[100]                       # the last station of the first tile of 256; the class
        #                                                               {0, 256} of the first and last station straddles the tiles
        lon[3], lat[3] = -lon[100], lat[100]
        lat[200] = np.nextafter(lat[100], 90.0)                       # one ulp away: by the products, whichever way they fall
        lon[200] = lon[100]
    tm = {}
    cls, size = _qalib.dup_classes(lon, lat, timing=tm)
    wc, ws = RR.dup_classes(lon, lat)
    assert np.array_equal(cls, wc) and np.array_equal(size, ws), (nstn, np.nonzero(cls != wc)[0])
    assert _times_ok(tm, _qalib.RV_KERNELS[2]), tm
    if nstn >= 2:
        assert cls[-1] == 0 and size[0] >= 2
    if nstn == 257:                                                   # and against the executed reference on the golden table
        cls, size = _qalib.dup_classes(G["dup_lon"], G["dup_lat"])
        assert np.array_equal(cls[:, None] == cls[None, :], G["dup_zero"])
        assert sorted(set(size[size > 1].tolist())) == [2, 3, 5]


@pytest.mark.parametrize("nstn", [1, 64, 65, 257])
def test_col_count(nstn):
    from topowx_amd import _qalib
    rs = np.random.RandomState(1000 + nstn)
    fill = np.float32(_qalib.SC_FILL_F4)
    for ndays in (1, 255, 256, 257, 1000):
        flag = (rs.rand(ndays, nstn) < 0.3).astype(np.int8)
        flag[rs.rand(ndays, nstn) < 0.05] = -127
        flag[rs.rand(ndays, nstn) < 0.02] = 5
        x = rs.randn(ndays, nstn).astype(np.float32)
        for v in (np.nan, np.inf, -np.inf, fill):
            x[rs.rand(ndays, nstn) < 0.03] = v
        lists = [np.zeros(0, np.int32), np.array([nstn - 1]), np.arange(nstn), rs.permutation(nstn)[:max(1, nstn // 3)],
                 rs.randint(0, nstn, 2 * nstn + 3), None]
        for cols in lists:
            for data, kw in ((flag, dict(fill=-127)), (flag, dict()), (x, dict(fill=fill)), (x, dict())):
                want = RR.col_count(data, cols, kw.get("fill", fill if data.dtype == np.float32 else None))
                a = _qalib.col_count(data, cols, **kw)
                row_bytes = nstn * data.dtype.itemsize
                t = {}
                b = _qalib.col_count(data, cols, workspace_bytes=row_bytes * ((ndays + 2) // 3), timing=t, **kw)
                assert a.dtype == np.int32 and np.array_equal(a, want), (nstn, ndays, data.dtype, cols)
                assert a.tobytes() == b.tobytes(), (nstn, ndays, "the batches change nothing")
                if ndays >= 3 and (cols is None or len(cols)):
                    assert t["rv_batches"] == 3 and _times_ok(t, _qalib.RV_KERNELS[3]), t
    with pytest.raises(ValueError, match="outside"):
        _qalib.col_count(np.zeros((3, nstn), np.int8), [nstn])


# ---- end to end through files of both containers ---------------------------------------------------------------------------
def _e2e_rasters(root, rs):
    """The reference's file names under ``root``: 24 LST rasters with a no-data coast, a TDI raster that does not reach every
    station, a mask with no-data outside a region and climate divisions with a gap inside the mask."""
    from test_stnrast_host import write_tiff
    os.makedirs(os.path.join(root, "lst"))
    rows = cols = 100
    geo = dict(scale=(0.05, 0.05), tie=(0, 0, 0, -111.5, 43.5, 0))
    yy, xx = np.mgrid[0:rows, 0:cols]
    grids = {}
    for stem in ("LST_Night", "LST_Day"):
        for mth in range(1, 13):
            a = (270.0 + mth + 0.1 * yy - 0.05 * xx + rs.randn(rows, cols)).astype(np.float32)
            a[:, :9] = -9999.0                                        # the coast: forced values
            a[rs.rand(rows, cols) < 0.03] = -9999.0
            name = os.path.join("lst", "%s.%.2d" % (stem, mth))
            write_tiff(os.path.join(root, name + ".tif"), a, tiled=bool(mth % 2), deflate=mth % 3 == 0, nodata="-9999", **geo)
            grids[name] = (a, -9999.0, -9999.0)
    tdi = (50 + 10 * np.sin(yy / 9.0) + rs.randn(rows, cols)).astype(np.float32)
    mask = np.where((xx > 15) & (yy > 10), 1, 255).astype(np.uint8)
    div = (1 + yy // 25 * 4 + xx // 25).astype(np.int16)
    div[40:55, 30:50] = -32768                                        # inside the mask, no climate division
    for name, a, nd, band in (("tdi", tdi, -9999.0, -9999.0), ("mask", mask, 0.0, 255.0), ("climdiv", div, -32768.0, -32768.0)):
        write_tiff(os.path.join(root, name + ".tif"), a, deflate=True, nodata="%d" % band, **geo)
        grids[name] = (a, nd, band)
    return grids, (-111.5, 0.05, 0.0, 43.5, 0.0, -0.05)


@pytest.mark.parametrize("fmt", ["NETCDF4", "NETCDF3_64BIT"])
def test_step19_step20_end_to_end(tmp_path, capsys, fmt):
    """step18-style databases -> ``python -m topowx_amd.step19`` -> ``python -m topowx_amd.step20 --infill-* --flagged-bad``.
    The reference is not on the GPU machine, so what its lines compute on the same inputs is taken from the restatement
    that tests/test_stnrast_host.py pins to the executed reference: every station variable bit for bit, and the ``bad``
    variable = flagged ids + no TDI + no climate division inside the mask + duplicates + the outliers step20 reports."""
    import datetime as dt
    from test_stnrast_host import _write_infill_db
    from topowx_amd import ncio, step19, step20, synth
    from topowx_amd import stationdb as sdb
    from topowx_amd.dates import get_days_metadata
    if fmt == "NETCDF4" and ncio.default_format() != "NETCDF4":
        pytest.fail("libhdf5 must be loadable on the GPU machine (NetCDF-4 station databases)")
    rs = np.random.RandomState(19)
    grids, geo_t = _e2e_rasters(str(tmp_path / "rasters"), rs)
    days = get_days_metadata(dt.date(1981, 1, 1), dt.date(1981, 1, 20))
    paths, ipaths, dbs, flags = {}, {}, {}, {}
    for var in ("tmin", "tmax"):
        db = synth.make_stations((40.0, 42.0, -110.0, -108.0), 320, 5, var, days, with_obs=True, nan_frac=0.0)
        n = db.stns.size
        for a, b in ((40, 12), (41, 12), (200, 199), (n - 1, 0)):     # duplicate locations
            db.stns[sdb.LON][a], db.stns[sdb.LAT][a] = db.stns[sdb.LON][b], db.stns[sdb.LAT][b]
        flag = (rs.rand(days.size, n) < 0.3).astype(np.int8)
        flag[:, 12], flag[:, 40], flag[:, 41] = 0, 1, 0
        flag[:2, 41] = 1
        flag[:, 200] = flag[:, 199]                                   # tied: both kept
        flag[:, n - 1] = 1
        flag[:4, 0] = -127
        paths[var], ipaths[var] = str(tmp_path / ("serial_%s.nc" % var)), str(tmp_path / ("infill_%s.nc" % var))
        # the table as step18 leaves it: id, coordinates, elevation and the normals; step19 and step20 add the rest
        names = [sdb.STN_ID, sdb.LON, sdb.LAT, sdb.ELEV] + [sdb.get_norm_varname(m) for m in range(1, 13)]
        stns = np.empty(n, [(k, db.stns.dtype[k]) for k in names])
        for k in names:
            stns[k] = db.stns[k]
        db = sdb.StationSerialDataDb(stns, var, days, db.var)
        ncio.write_station_db(paths[var], db, format=fmt)
        _write_infill_db(ipaths[var], db, var, flag, fmt)
        dbs[var], flags[var] = db, flag
    argv19 = ["--serial-tmin", paths["tmin"], "--serial-tmax", paths["tmax"], "--rasters", str(tmp_path / "rasters")]
    assert step19.main(argv19) == 0
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 30 and all(r["stations"] == dbs[r["db"]].stns.size for r in lines)
    assert all(r["bilinear"] + r["nearest"] + r["forced"] + r["nodata"] == r["stations"] for r in lines)
    assert sum(r["forced"] for r in lines if r["var"].startswith("lst")) > 100
    assert all(r["forced"] == 0 for r in lines if not r["var"].startswith("lst"))
    # every station variable against the per-station restatement
    want_bad, nbits = {}, 0
    for var, stem in (("tmin", "LST_Night"), ("tmax", "LST_Day")):
        da = sdb.StationSerialDataDb(paths[var], var)
        try:
            lon, lat, ids = da.stns[sdb.LON], da.stns[sdb.LAT], da.stn_ids
            jobs = [(sdb.get_lst_varname(m), os.path.join("lst", "%s.%.2d" % (stem, m)), (1, True, True)) for m in (1, 6, 12)]
            jobs += [(sdb.TDI, "tdi", (1, True, False)), (sdb.MASK, "mask", (0, False, False)), (sdb.CLIMDIV, "climdiv", (0, False, False))]
            vals = {}
            for name, key, combo in jobs:
                a, nd, band = grids[key]
                g = RR.Grid(a, geo_t, band)
                g.ndata = nd
                w = RR.add_stn_raster_values(g, lon, lat, *combo)["value"]
                w = np.where(w == nd, np.nan, w)                      # the fill value reads back as NaN
                got = np.asarray(da.stns[name], np.float64)
                assert np.array_equal(np.isnan(got), np.isnan(w)), (var, name)
                nbits += int((got[~np.isnan(w)].view(np.uint64) != w[~np.isnan(w)].view(np.uint64)).sum())
                vals[name] = w
            assert not np.isnan(vals[sdb.get_lst_varname(6)]).any()   # force_data_value: every station has an LST value
            no_tdi = set(ids[np.isnan(vals[sdb.TDI])])
            no_div = set(ids[np.isnan(vals[sdb.CLIMDIV]) & np.isfinite(vals[sdb.MASK])])
            dup = set(RR.find_dup_stns(ids, lon, lat, np.where(flags[var] == -127, 0, flags[var])).tolist())
            assert no_tdi and no_div and dup == {ids[40], ids[41], ids[-1]}, (len(no_tdi), len(no_div), dup)
            want_bad[var] = no_tdi | no_div | dup | {ids[77]}
        finally:
            da.close()
    print("%s: station values not bit-equal to the restatement: %d" % (fmt, nbits))
    assert nbits == 0
    csv = str(tmp_path / "flagged_bad.csv")
    with open(csv, "w") as fh:
        fh.write("station_id,reason\n%s,infill issue\n" % ids[77])
    argv20 = ["--tmin", paths["tmin"], "--tmax", paths["tmax"], "--infill-tmin", ipaths["tmin"], "--infill-tmax", ipaths["tmax"],
              "--flagged-bad", csv, "--nnghs", "50"]
    assert step20.main(argv20) == 0
    out = capsys.readouterr().out
    screens = [json.loads(s) for s in out.splitlines() if s.startswith("{")]
    assert [r["var"] for r in screens] == ["tmin", "tmax"]           # XvalOutlier ran on the flagged databases
    outliers = set(screens[0]["outliers"]) | set(screens[1]["outliers"])
    for k, var in enumerate(("tmin", "tmax")):
        assert "%d total stations removed for %s:" % (len(want_bad[var]), var) in out
        assert screens[k]["stations"] == dbs[var].stns.size - len(want_bad[var])
        da = sdb.StationSerialDataDb(paths[var], var)
        try:
            assert set(da.stn_ids[~np.isnan(da.stns[sdb.BAD])].tolist()) == want_bad[var] | outliers, var
        finally:
            da.close()
    # the final check's failure path, on the file
    ds = ncio.open_dataset(paths["tmin"], "a")
    good = [i for i in range(50, 60) if dbs["tmin"].stn_ids[i] not in want_bad["tmin"] | outliers][0]
    col = np.array(ds.variables["tmin"][:, good])
    col[3] = np.nan
    ds.variables["tmin"][:, good] = col
    ds.close()
    assert step20.main(argv20) == 1
    assert "Missing values found in %s" % paths["tmin"] in capsys.readouterr().err
