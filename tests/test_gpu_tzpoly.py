"""GPU: step13's time-zone lookup (``twxtz_locate`` under ``UtcOffset``) against the exact oracle (tests/restate_tzpoly.py).
After the host settlement ``poly``, ``status`` and the zone of EVERY point must equal the oracle's: no tolerance, no point
left out.  Sizes walk the wavefront (64), the work-group and the chunk of the containment kernel; the adversarial points
sit on vertices, edges, rays through vertices and bbox corners and must send work through the filter; forced points cover
ties, both kinds of nearest feature and the reach limit to the ulp; two calls give the same bytes, also when the uncertain
list overflows; step13 end to end in both containers feeds ``step14 --estimate --nnr-dir``."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import restate_tzpoly as RT  # noqa: E402
import tzpoly_cases as TC  # noqa: E402
from topowx_amd import _qalib, h5nc, ncio  # noqa: E402
from topowx_amd.utc_offsets import UtcOffset, add_utc_offset  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
FORMATS = [pytest.param("NETCDF4", marks=pytest.mark.skipif(not h5nc.available(), reason="libhdf5 not loadable")),
           "NETCDF3_64BIT"]
WORST = {"dist": 0.0}


def dist_bound():
    """Relative bound of ``dist_deg`` against the root of the oracle's d2 rounded to float64, from the header's count of
    rounded operations: d2 carries at most TZ_D2_RELERR_ULPS x 2^-53, its root half of that plus the root's own rounding
    (2^-53); the oracle's side adds the rounding of d2 (half of 2^-53 after the root) and of its root (2^-53)."""
    h = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_tzpoly_pred.h")).read()
    return (float(re.search(r"#define TZ_D2_RELERR_ULPS ([0-9.]+)", h).group(1)) / 2.0 + 2.5) * EPS


def check(utc, lon, lat, min_settled=0):
    """Every point against the oracle; returns the result and the report."""
    tz = utc.tz
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    res = utc.get_utc_offsets(lon, lat)
    rep = utc.last_report
    poly, status, d2 = RT.Exact(tz.edges, tz.edge_off).locate_all(lon, lat, utc.max_force_deg)
    bad = np.nonzero((res.poly != poly) | (res.status != status))[0]
    assert bad.size == 0, [(int(i), float(lon[i]).hex(), float(lat[i]).hex(), int(res.poly[i]), int(poly[i]), int(res.status[i]),
                            int(status[i])) for i in bad[:5]]
    assert res.poly.dtype == np.int32 and res.status.dtype == np.int32 and res.poly.shape == lon.shape
    zone = [tz.names[tz.zone[p]] if p >= 0 else None for p in poly.tolist()]
    assert res.zone.tolist() == zone
    assert res.offset.tolist() == [utc.tz_offsets[z] if z is not None else utc.ndata for z in zone]
    bound = dist_bound()
    for i in range(lon.size):
        if status[i] == RT.INSIDE:
            assert res.dist_deg[i] == 0.0
        elif status[i] == RT.BAD_POINT:
            assert np.isnan(res.dist_deg[i])
        else:
            want = float(d2[i]) ** 0.5
            if want == 0.0 or float(d2[i]) < 2.0 ** -900:
                assert res.dist_deg[i] == want
                continue
            err = abs(res.dist_deg[i] - want) / want
            WORST["dist"] = max(WORST["dist"], err)
            assert err <= bound, (i, err / EPS)
    assert rep["settled"] >= min_settled and rep["npoints"] == lon.size
    return res, rep


def make(tmp_path, feats, form="tz_world", **kw):
    return UtcOffset(TC.write_geojson(str(tmp_path / "tz.json"), feats, form), **kw)


@pytest.mark.parametrize("nedge", TC.EDGE_COUNTS)
def test_edge_counts(tmp_path, nedge):
    """Two overlapping polygons of nedge edges each and a small third; random points, vertices and edge midpoints."""
    feats = [("America/Denver", [[TC.ngon(-110.0, 40.0, 3.0, nedge, 100 + nedge)]]),
             ("America/Chicago", [[TC.ngon(-106.5, 41.0, 3.0, nedge, 200 + nedge)]]),
             ("America/Phoenix", [[TC.ngon(-108.0, 36.5, 1.0, 5, 7)]])]
    utc = make(tmp_path, feats)
    assert np.diff(utc.tz.edge_off).tolist() == [nedge, nedge, 5]
    lon, lat = TC.box_points(97, (-114.0, 35.0, -102.5, 45.0), nedge)
    k = np.linspace(0, nedge - 1, min(nedge, 16)).astype(int)     # some vertices of the first polygon and their midpoints
    e = utc.tz.edges[k]
    lon = np.concatenate([lon, e[:, 0], (e[:, 0] + e[:, 2]) / 2.0])
    lat = np.concatenate([lat, e[:, 1], (e[:, 1] + e[:, 3]) / 2.0])
    res, rep = check(utc, lon, lat)
    assert rep["items"] >= rep["pairs"] and (rep["items"] > rep["pairs"]) == (nedge > TC.CHUNK)
    assert {RT.INSIDE, RT.FORCED}.issubset(set(res.status.tolist()))


@pytest.mark.parametrize("npt", TC.POINT_COUNTS)
@pytest.mark.parametrize("npoly", TC.POLY_COUNTS)
def test_polygon_and_point_counts(tmp_path, npoly, npt):
    feats, box = TC.grid_features(npoly, 31 + npoly)
    utc = make(tmp_path, feats, "combined")
    assert utc.tz.zone.size == npoly
    lon, lat = TC.box_points(npt, box, 1000 * npoly + npt)
    check(utc, lon, lat)


def test_geometry_cases(tmp_path):
    """A hole with another zone's enclave in it; two overlapping polygons (the lower file index wins); a MultiPolygon zone."""
    feats = [("America/Denver", [[TC.rect(0, 0, 10, 10), TC.rect(3, 3, 7, 7)], [TC.rect(20, 0, 24, 4)]]),
             ("America/Chicago", [[TC.rect(4, 4, 6, 6)]]),
             ("America/Phoenix", [[TC.rect(8, 8, 12, 12)]]),
             ("America/New_York", [[TC.rect(9, 9, 11, 11)]])]
    utc = make(tmp_path, feats, "combined")
    assert utc.tz.zone.tolist() == [0, 0, 1, 2, 3]
    lon = [5.0, 3.5, 1.0, 22.0, 9.5, 11.5, 10.5, 3.0, 7.0, 15.0]
    lat = [5.0, 5.0, 1.0, 2.0, 9.5, 11.5, 10.5, 3.0, 5.0, 2.0]
    res, _ = check(utc, lon, lat, 1)
    #        enclave  hole->nearest  body  island  overlap 0|3|4  3  3|4  hole corner  hole's edge  far from all
    assert res.poly.tolist() == [2, 0, 0, 1, 0, 3, 3, 0, 0, -1]
    assert res.status[1] == RT.FORCED and res.dist_deg[1] == 0.5 and res.status[-1] == RT.NONE and res.offset[-1] == utc.ndata
    assert res.zone[0] == "America/Chicago" and res.zone[3] == "America/Denver" and res.offset[3] == -7.0
    # without holes the enclave is never reached: the body comes first in the file
    flat = UtcOffset(str(tmp_path / "tz.json"), holes=False)
    r2, _ = check(flat, lon, lat)
    assert r2.poly[:2].tolist() == [0, 0] and r2.status[1] == RT.INSIDE
    assert flat.get_utc_offset(5.0, 5.0) == -7.0 and utc.get_utc_offset(5.0, 5.0) == -6.0


def test_adversarial_points(tmp_path):
    feats = [("America/Denver", [[TC.ngon(-110.0, 40.0, 3.0, 129, 5), TC.rect(-110.5, 39.5, -109.5, 40.5)]]),
             ("America/Chicago", [[TC.rect(-106.0, 38.0, -104.0, 40.0)]]),
             ("America/Phoenix", [[[(-104.0, 38.0), (-102.0, 38.0), (-102.0, 40.0), (-104.0, 40.0)]]]),      # shares an edge with the last
             ("America/New_York", [[TC.ngon(-107.5, 41.0, 1.5, 9, 6)]])]
    utc = make(tmp_path, feats)
    lon, lat = TC.adversarial_points(utc.tz.edges, utc.tz.bbox)
    assert lon.size > 1000
    _, rep = check(utc, lon, lat, 1)
    assert rep["settled"] > 100 and rep["uncertain"] == rep["settled"]      # the filter path did run


def test_forced_cases(tmp_path):
    feats = [("America/Denver", [[TC.rect(0, 0, 2, 2)]]), ("America/Chicago", [[TC.rect(4, 0, 6, 2)]]),
             ("America/Phoenix", [[[(0.0, 5.0), (2.0, 5.0), (1.0, 7.0)]]])]
    utc = make(tmp_path, feats, max_force_deg=1.0)
    one = 1.0
    lon = [3.0, 3.0, 2.5, 2.5, 1.0, 2.0 + one, np.nextafter(2.0 + one, 9.0), np.nextafter(3.0, 0.0), 1.0, np.nan, 1.0, -0.5, 3.0]
    lat = [1.0, 2.5, 2.5, 1.0, 2.75, -3.0, 1.0, -3.0, 3.5, 1.0, np.inf, -0.5, 1.0]
    res, rep = check(utc, lon, lat, 1)
    assert res.poly[0] == 0 and res.status[0] == RT.FORCED and res.dist_deg[0] == 1.0       # equidistant by construction: the lower index
    assert res.poly[2] == 0 and res.dist_deg[2] == 0.5 ** 0.5                                 # nearest to a vertex
    assert res.poly[3] == 0 and res.dist_deg[3] == 0.5                                        # nearest to an edge's interior
    assert res.status[9] == RT.BAD_POINT and res.status[10] == RT.BAD_POINT and res.poly[9] == -1 and res.offset[9] == utc.ndata
    assert res.status[5] == RT.NONE and res.offset[5] == utc.ndata and res.zone[5] is None
    # the reach to the ulp: max_force_deg = the distance, one ulp less, one ulp more
    for px, py in ((2.75, 1.0), (1.0, 3.1), (2.3, 2.4)):
        d2 = RT.Exact(utc.tz.edges, utc.tz.edge_off).locate_all([px], [py], None)[2][0]
        d = float(d2) ** 0.5
        for reach in (d, np.nextafter(d, 0.0), np.nextafter(d, 9.0)):
            u = UtcOffset(utc.tz, max_force_deg=float(reach))
            r, _ = check(u, [px], [py])
            assert (r.status[0] == RT.NONE) == (d2 > Fraction(float(reach)) ** 2)
        assert {int(check(UtcOffset(utc.tz, max_force_deg=float(np.nextafter(d, s))), [px], [py])[0].status[0]) for s in (0.0, 9.0)} == \
            {RT.NONE, RT.FORCED}
    r, _ = check(UtcOffset(utc.tz, max_force_deg=None), [300.0], [-80.0])
    assert r.status[0] == RT.FORCED


def test_two_calls_give_the_same_bytes(tmp_path):
    feats, box = TC.grid_features(65, 3)
    utc = make(tmp_path, feats)
    tz = utc.tz
    ax, ay = TC.adversarial_points(tz.edges, tz.bbox)
    bx, by = TC.box_points(257, box, 9)
    lon, lat = np.concatenate([ax, bx]), np.concatenate([ay, by])
    outs = []
    for cap in (1, 1, 1 << 16, 1 << 16):
        tm = {}
        poly, status, d2, unc, counts = _qalib.tz_locate(lon, lat, tz.edge_off, tz.bbox, tz.edges, 1.0, cap)
        _qalib.tz_locate(lon, lat, tz.edge_off, tz.bbox, tz.edges, 1.0, cap, timing=tm)
        assert tm["tz_calls"] == (2 if cap == 1 else 1)            # the overflow-and-retry path was taken
        assert all(np.isfinite(tm[k + "_ms"]) and tm[k + "_ms"] >= 0 for k in _qalib.TZ_PHASES), tm
        assert unc.shape[0] == counts[_qalib.TZ_C_UNCERTAIN] > 1 and np.array_equal(unc, unc[np.lexsort((unc[:, 1], unc[:, 0]))])
        outs.append(b"".join(a.tobytes() for a in (poly, status, d2, unc, counts)))
    assert outs[0] == outs[1] == outs[2] == outs[3]
    a = utc.get_utc_offsets(lon, lat, uncertain_cap=1)
    b = utc.get_utc_offsets(lon, lat)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() if x.dtype != object else x.tolist() == y.tolist()


@pytest.mark.parametrize("fmt", FORMATS)
def test_step13_end_to_end_feeds_step14(tmp_path, capsys, fmt):
    """step13 on a database without utc_offset: a dry run writes nothing; a run writes the oracle's truncated values and
    leaves the fill for the undetermined stations; with polygons for every station step14 --estimate --nnr-dir runs."""
    import chkperf_cases as CC
    import nnr_cases as NC
    from topowx_amd import stationdb as sdb, step13, step14
    pool, _, _ = CC.facade_pool()
    c, want_utc = NC.case_over(pool)
    n = pool.ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = pool.ids, pool.lon, pool.lat, 1000.0
    db = str(tmp_path / "all.nc")
    ncio.create_quick_db(db, stns, pool.days, [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                                               ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")], format=fmt)
    ds = ncio.open_dataset(db, "a")
    for name, a in (("tmin", pool.tmin), ("tmax", pool.tmax)):
        v = ds.variables[name]
        v.missing_value = np.float32(ncio.FILL_F4)
        v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
    ds.close()
    nnr_dir = c.write(str(tmp_path / "nnr"), "NETCDF3_64BIT")
    out14 = str(tmp_path / "m.npz")
    argv14 = ["--db", db, "--var", "tmin", "--out", out14, "--estimate", "--nnr-dir", nnr_dir]
    assert step14.main(argv14) == 1 and "no station variable utc_offset" in capsys.readouterr().err
    # the west cluster lies in Denver; of the east one a part lies in St Johns' polygon (-3.5 h) and the rest in no polygon: with a reach of 0 they stay undetermined
    split = float(np.sort(pool.lon[pool.lon > -108.0])[3]) + 1e-6
    part = TC.write_geojson(str(tmp_path / "part.json"), [("America/Denver", [[TC.rect(-112, 44, -108, 46)]]),
                                                          ("America/St_Johns", [[TC.rect(split - 0.001, 44, split + 3.0, 46)]])])
    before = open(db, "rb").read()
    assert step13.main(["--db", db, "--tz-polygons", part, "--dry-run", "--max-force-deg", "0", "--report",
                        str(tmp_path / "dry.npz")]) == 0
    assert open(db, "rb").read() == before and "Couldn't determine UTC offset for: " in capsys.readouterr().out
    assert step13.main(["--db", db, "--tz-polygons", part, "--max-force-deg", "0", "--report", str(tmp_path / "r.npz")]) == 0
    out = capsys.readouterr().out
    tz = UtcOffset(part).tz
    poly, status, _ = RT.Exact(tz.edges, tz.edge_off).locate_all(pool.lon, pool.lat, 0.0)
    want = np.array([{0: -7, 1: -3}.get(int(p), ncio.FILL_I2) for p in poly], np.int16)      # -3.5 truncates toward zero
    assert set(want.tolist()) == {-7, -3, int(ncio.FILL_I2)} and (status == RT.NONE).sum() == 3
    with ncio.open_dataset(db) as ds:
        v = ds.variables["utc_offset"]
        assert np.dtype(v.dtype) == np.int16 and tuple(v.dimensions) == (sdb.STN_ID,) and v.getncattr("long_name") == "utc_offset"
        assert v.getncattr("units") == "" and np.asarray(v[:]).astype(np.int16).tolist() == want.tolist()
    rep = np.load(str(tmp_path / "r.npz"))
    dry = np.load(str(tmp_path / "dry.npz"))
    assert rep["utc_offset"].tolist() == want.tolist() == dry["utc_offset"].tolist() and rep["status"].tolist() == status.tolist()
    for sid in pool.ids[status == RT.NONE]:
        assert "Error: Couldn't determine UTC offset for: %s" % sid in out
    assert step14.main(argv14) == 1 and "utc_offset must hold a value for every station" in capsys.readouterr().err
    full = TC.write_geojson(str(tmp_path / "full.json"), [("America/Denver", [[TC.rect(-112, 44, -108, 46)]]),
                                                          ("America/Chicago", [[TC.rect(-107.5, 44, -104, 46)]])], "combined")
    assert step13.main(["--db", db, "--tz-polygons", full]) == 0
    capsys.readouterr()
    with ncio.open_dataset(db) as ds:
        assert np.asarray(ds.variables["utc_offset"][:]).astype(np.int16).tolist() == want_utc.tolist()
    assert step14.main(argv14) == 0
    got = np.load(out14)
    assert (got["ncomp"][got["em_status"] == 0] > 0).any()
    # the library call: the report of add_utc_offset
    r = add_utc_offset(db, full, dry_run=True)
    assert r["utc_offset"].tolist() == want_utc.tolist() and r["written"] is False and r["inside"] == n


def test_report_the_largest_dist_error():
    """Runs last in this file: the largest relative error of dist_deg seen by the tests above."""
    print("largest relative error of dist_deg: %.2f x 2^-53 (bound %.1f)" % (WORST["dist"] / EPS, dist_bound() / EPS))
    assert WORST["dist"] <= dist_bound()
