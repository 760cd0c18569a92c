"""Step13 (the time-zone lookup) without a GPU: the GeoJSON reader on both forms; the zone -> offset table against the
reference's three lines; the two routes of the oracle against each other; the predicates of the kernels
(twx_tzpoly_pred.h) run on the CPU under the address and undefined-behaviour sanitizers as a program of its own and held
against the oracle edge by edge; header / binding / build naming and the resource table of a build; the argument checks
of ``twxtz_locate``, made before anything touches a device."""
import datetime
import json
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import restate_tzpoly as RT  # noqa: E402
import tzpoly_cases as TC  # noqa: E402
from topowx_amd import _qalib, utc_offsets  # noqa: E402
from topowx_amd.utc_offsets import UtcOffset, load_tz_polygons  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(_qalib.LIB_PATH), reason="no build in this checkout (run ./build.sh)")
NEW_KERNELS = ["k_tz_contain", "k_tz_count", "k_tz_forced", "k_tz_pick", "k_tz_scatter"]
EPS = 2.0 ** -53

SQUARE = TC.rect(0, 0, 10, 10)
HOLE = TC.rect(3, 3, 7, 7)
ISLAND = TC.rect(20, 0, 24, 4)
FEATURES = [("America/Denver", [[SQUARE, HOLE], [ISLAND]]), ("America/St_Johns", [[TC.rect(4, 4, 6, 6)]])]


def test_reader_on_both_forms(tmp_path):
    a = load_tz_polygons(TC.write_geojson(str(tmp_path / "w.json"), FEATURES, "tz_world"))
    b = load_tz_polygons(TC.write_geojson(str(tmp_path / "c.json"), FEATURES, "combined", close=False))
    doc = json.load(open(str(tmp_path / "c.json")))
    assert [f["geometry"]["type"] for f in doc["features"]] == ["MultiPolygon", "Polygon"] and "tzid" in doc["features"][0]["properties"]
    assert "TZID" in json.load(open(str(tmp_path / "w.json")))["features"][0]["properties"]
    for t in (a, b):                                              # closed and unclosed rings, one feature per part or not
        assert t.names == ["America/Denver", "America/St_Johns"] and t.zone.tolist() == [0, 0, 1] and t.zone.dtype == np.int32
        assert t.edge_off.tolist() == [0, 8, 12, 16] and t.edge_off.dtype == np.int64
        assert t.edges.shape == (16, 4) and t.edges.dtype == np.float64 and t.edges.flags.c_contiguous
        assert t.bbox.tolist() == [[0, 0, 10, 10], [20, 0, 24, 4], [4, 4, 6, 6]]
        assert t.edges[0].tolist() == [0, 0, 10, 0] and t.edges[3].tolist() == [0, 10, 0, 0] and t.edges[4].tolist() == [3, 3, 7, 3]
    assert a.edges.tobytes() == b.edges.tobytes()
    nh = load_tz_polygons(str(tmp_path / "w.json"), holes=False)
    assert nh.edge_off.tolist() == [0, 4, 8, 12] and nh.bbox.tolist() == a.bbox.tolist()
    # the even-odd rule over the one edge list makes the hole; without holes the point is inside
    assert not RT.contains(a.edges[:8].tolist(), 5.0, 3.5) and RT.contains(nh.edges[:4].tolist(), 5.0, 3.5)
    # zero-length edges are dropped, a repeated vertex in the middle of a ring does not add one
    dup = [("America/Denver", [[[(0, 0), (0, 0), (5, 0), (5, 0), (5, 5), (0, 0)]]])]
    d = load_tz_polygons(TC.write_geojson(str(tmp_path / "d.json"), dup, "tz_world", close=False))
    assert d.edges.tolist() == [[0, 0, 5, 0], [5, 0, 5, 5], [5, 5, 0, 0]]
    assert "180" in load_tz_polygons.__doc__ and "NOT been verified" in load_tz_polygons.__doc__


def _feature(geometry, props=None):
    return {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"tzid": "America/Denver"}, "geometry": {"type": "Polygon", "coordinates": [SQUARE]}},
        {"type": "Feature", "properties": {"tzid": "America/Denver"} if props is None else props, "geometry": geometry}]}


@pytest.mark.parametrize("doc, pat", [
    (_feature({"type": "Polygon", "coordinates": [[[0, 0], [1, 1], [0, 0], [1, 1]]]}), "feature 1.*fewer than 3 distinct"),
    (_feature({"type": "Polygon", "coordinates": [[[0, 0], [1, 0], [1, float("nan")]]]}), "feature 1.*not finite"),
    (_feature({"type": "MultiPolygon", "coordinates": [[SQUARE], [[[0, 0], [float("inf"), 0], [1, 1]]]]}), "feature 1.*not finite"),
    (_feature({"type": "Polygon", "coordinates": [SQUARE]}, {"name": "x"}), "feature 1 has no zone property"),
    (_feature({"type": "LineString", "coordinates": SQUARE}), "feature 1.*'LineString' is neither"),
    (_feature({"type": "Polygon", "coordinates": []}), "feature 1"),
    ({"type": "Feature"}, "not a GeoJSON FeatureCollection")])
def test_reader_refuses_by_feature(tmp_path, doc, pat):
    p = str(tmp_path / "bad.json")
    with open(p, "w") as fh:
        json.dump(doc, fh)                                         # Python writes NaN / Infinity, and reads them back
    with pytest.raises(ValueError, match=pat):
        load_tz_polygons(p)


def test_offsets_table_is_the_references(tmp_path):
    names = ["America/Denver", "America/St_Johns", "uninhabited", "Asia/Kolkata", "America/Phoenix"]
    feats = [(n, [[TC.rect(3 * k, 0, 3 * k + 2, 2)]]) for k, n in enumerate(names)]
    utc = UtcOffset(TC.write_geojson(str(tmp_path / "z.json"), feats), ndata=-32767)
    # the reference's lines (stn_utc_offsets.py:70-74), executed
    a_date = datetime.datetime(2009, 1, 1)
    want = {}
    try:
        import pytz
        zone_of = pytz.timezone
    except ImportError:
        import zoneinfo
        zone_of = zoneinfo.ZoneInfo
    for a_name in names:
        if a_name != "uninhabited":
            a_tz = zone_of(a_name)
            want[a_name] = a_tz.utcoffset(a_date).total_seconds() / 3600.0
    want["uninhabited"] = -32767
    assert utc.tz_offsets == want
    assert utc.tz_offsets["America/Denver"] == -7.0 and utc.tz_offsets["America/St_Johns"] == -3.5
    assert utc.tz_offsets["Asia/Kolkata"] == 5.5 and utc.tz_offsets["uninhabited"] == utc.ndata
    # the i2 variable truncates toward zero, as the reference's assignment does
    assert np.float64(utc.tz_offsets["America/St_Johns"]).astype("i2") == -3 and np.float64(5.5).astype("i2") == 5
    with pytest.raises(ValueError, match="unknown time zone name 'Mars/Olympus'"):
        UtcOffset(TC.write_geojson(str(tmp_path / "m.json"), [("Mars/Olympus", [[SQUARE]])]))
    with pytest.raises(ValueError, match="max_force_deg"):
        UtcOffset(str(tmp_path / "z.json"), max_force_deg=-1.0)
    for word in ("uninhabited", "KeyError", "Geonames", "restated"):
        assert word in UtcOffset.__doc__


def _case():
    """Three polygons (a 65-gon with a square hole, a triangle inside the hole, an overlapping 7-gon) and sharp points."""
    feats = [("America/Denver", [[TC.ngon(0.0, 0.0, 5.0, 65, 1), TC.rect(-1, -1, 1, 1)]]),
             ("America/Chicago", [[[(-0.5, -0.5), (0.5, -0.5), (0.0, 0.5)]]]),
             ("America/Phoenix", [[TC.ngon(5.0, 1.0, 3.0, 7, 2)]])]
    return feats


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    tz = load_tz_polygons(TC.write_geojson(str(tmp_path_factory.mktemp("tz") / "s.json"), _case()))
    ax, ay = TC.adversarial_points(tz.edges, tz.bbox)
    bx, by = TC.box_points(40, (-7, -7, 9, 7), 5)
    return tz, np.concatenate([ax, bx, [np.nan]]), np.concatenate([ay, by, [0.0]])


def test_oracle_routes_agree(small):
    tz, lon, lat = small
    pick = np.r_[0:lon.size:7, lon.size - 1]
    poly, status, d2 = RT.Exact(tz.edges, tz.edge_off).locate_all(lon[pick], lat[pick], 1.0)
    for k, i in enumerate(pick.tolist()):
        assert (poly[k], status[k], d2[k]) == RT.locate(tz.edges.tolist(), tz.edge_off.tolist(), float(lon[i]), float(lat[i]), 1.0), i
    assert set(status.tolist()) >= {RT.INSIDE, RT.FORCED, RT.BAD_POINT}
    # the enclave inside the hole, the hole, the overlap (the lower index wins)
    ex = RT.Exact(tz.edges, tz.edge_off)
    poly, status, d2 = ex.locate_all([0.0, 0.875, 4.0, 30.0], [0.0, 0.875, 1.0, 0.0], 1.0)
    assert poly.tolist() == [1, 0, 0, -1] and status.tolist() == [RT.INSIDE, RT.FORCED, RT.INSIDE, RT.NONE]
    assert d2[1] == Fraction(1, 64)                               # in the hole, an eighth from its edge: nearer than the enclave
    assert ex.locate_all([0.875], [0.875], 0.1)[1].tolist() == [RT.NONE] and ex.locate_all([30.0], [0.0], None)[1].tolist() == [RT.FORCED]


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "tzpoly_hostcheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "topowx_amd", "qa"),
                           os.path.join(HERE, "tools", "tzpoly_hostcheck.cpp"), "-o", exe])
    return exe


def test_predicates_on_the_cpu_under_sanitizers(hostcheck, small, tmp_path):
    """Every (point, edge) of the small case through tz_edge_cross and tz_seg_d2, every (point, polygon) through the bbox
    test and the parity walk.  A lane may be uncertain where the oracle is decided; it may never be decided and wrong."""
    tz, lon, lat = small
    lon, lat = lon[:-1], lat[:-1]                                  # the NaN point never reaches a predicate
    h = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_tzpoly_pred.h")).read()
    ulps = float(re.search(r"#define TZ_D2_RELERR_ULPS ([0-9.]+)", h).group(1))
    case = str(tmp_path / "case.txt")
    with open(case, "w") as fh:
        fh.write("%d %d %d\n" % (len(tz.edges), len(tz.zone), lon.size))
        for row in tz.edges.tolist():
            fh.write(" ".join(float(v).hex() for v in row) + "\n")
        fh.write(" ".join(str(int(v)) for v in tz.edge_off) + "\n")
        for row in tz.bbox.tolist():
            fh.write(" ".join(float(v).hex() for v in row) + "\n")
        for x, y in zip(lon.tolist(), lat.tolist()):
            fh.write("%s %s\n" % (float(x).hex(), float(y).hex()))
    res = subprocess.run([hostcheck, case], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    E = tz.edges.tolist()
    nunc = nill = npairs = 0
    worst = 0.0
    seen_pairs = set()
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] == "E":
            p, e, bits, ill = int(w[1]), int(w[2]), int(w[3]), int(w[4])
            d2, lo = float.fromhex(w[5]), float.fromhex(w[6])
            if bits & 2:
                nunc += 1
            else:
                assert bool(bits & 1) == RT.crosses(*E[e], float(lon[p]), float(lat[p])), (p, e)
            want = RT.seg_d2(*E[e], float(lon[p]), float(lat[p]))
            if ill:                                               # the value is a candidate only; the bound must hold
                nill += 1
                assert Fraction(lo) <= want, (p, e)
            elif want == 0:
                assert d2 == 0.0 == lo
            else:
                err = float(abs(Fraction(d2) - want) / want)
                worst = max(worst, err)
                assert err <= ulps * EPS and lo == d2, (p, e, err / EPS)
        else:
            p, q, parity, unc = int(w[1]), int(w[2]), int(w[3]), int(w[4])
            seen_pairs.add((p, q))
            npairs += 1
            if not unc:
                assert bool(parity) == RT.contains(E[tz.edge_off[q]:tz.edge_off[q + 1]], float(lon[p]), float(lat[p])), (p, q)
    # the bbox test is closed and exact: the pairs are those of the comparison on the coordinates
    want_pairs = {(p, q) for p in range(lon.size) for q, b in enumerate(tz.bbox.tolist())
                  if b[0] <= lon[p] <= b[2] and b[1] <= lat[p] <= b[3]}
    assert seen_pairs == want_pairs and npairs == len(want_pairs)
    assert nunc > 100 and nill > 0                                # the filter and the conditioning test did fire
    print("largest relative error of a well-conditioned d2: %.2f x 2^-53 (bound %.0f)" % (worst / EPS, ulps))


def test_unit_is_declared_bound_and_built():
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxtz_\w+)\s*\(", h))) == sorted(_qalib.TZ_EXPORTS)
    for name, val in (("NPHASES", len(_qalib.TZ_PHASES)), ("INSIDE", _qalib.TZ_INSIDE), ("FORCED", _qalib.TZ_FORCED),
                      ("NONE", _qalib.TZ_NONE), ("BAD_POINT", _qalib.TZ_BAD_POINT), ("UNCERTAIN", _qalib.TZ_UNCERTAIN),
                      ("PENDING", _qalib.TZ_PENDING), ("OVERFLOW", _qalib.TZ_OVERFLOW), ("CHUNK_EDGES", _qalib.TZ_CHUNK_EDGES),
                      ("C_N", 4), ("C_UNCERTAIN", _qalib.TZ_C_UNCERTAIN)):
        assert int(re.search(r"#define TWXTZ_%s (\d+)" % name, h).group(1)) == val, name
    assert (RT.INSIDE, RT.FORCED, RT.NONE, RT.BAD_POINT) == (_qalib.TZ_INSIDE, _qalib.TZ_FORCED, _qalib.TZ_NONE, _qalib.TZ_BAD_POINT)
    assert TC.CHUNK == _qalib.TZ_CHUNK_EDGES
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_tzpoly.hip" in build
    # every unit of topowx_amd/qa is named in the build script exactly once, and nothing that is not there
    named = re.findall(r"topowx_amd/qa/(twx_\w+\.hip)", build)
    on_disk = [f for f in os.listdir(os.path.join(ROOT, "topowx_amd", "qa")) if re.fullmatch(r"twx_\w+\.hip", f)]
    assert sorted(named) == sorted(on_disk) and len(set(named)) == len(named)
    assert build.count("topowx_amd/csrc/twx_hip.hip") == 1
    pred = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_tzpoly_pred.h")).read()
    assert "__host__ __device__" in pred and "hip_runtime" not in pred
    assert "Shewchuk" in open(os.path.join(ROOT, "PAPERS.md")).read()
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    import ctypes
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    assert all(hasattr(lib, n) for n in _qalib.TZ_EXPORTS)
    rows = {l.split("|")[0].strip(): [c.strip() for c in l.split("|")] for l in open(res) if l.startswith("k_tz_")}
    assert sorted(rows) == NEW_KERNELS
    head = [c.strip() for c in open(res).readline().split("|")]
    for word in ("scratch", "spills"):
        k = [i for i, c in enumerate(head) if word in c.lower()]
        assert k and all(int(r[k[0]]) == 0 for r in rows.values())


@needs_lib
def test_argument_errors_come_before_any_device_work(small):
    """None of these reaches the device: they pass on a machine without one."""
    tz = small[0]
    ok = dict(lon=[1.0], lat=[1.0], edge_off=tz.edge_off, bbox=tz.bbox, edges=tz.edges)
    zero = tz.edges.copy()
    zero[5, 2:] = zero[5, :2]
    nan = tz.edges.copy()
    nan[7, 1] = np.nan
    bb = tz.bbox.copy()
    bb[1, 0] = bb[1, 2] + 1.0
    for kw, pat in ((dict(lon=[], lat=[]), "TWXTZ_MAX_POINTS"), (dict(max_force_deg=-1.0), "max_force_deg must be >= 0"),
                    (dict(max_force_deg=float("nan")), "max_force_deg"), (dict(edges=zero), "edge 5 is not finite or has no length"),
                    (dict(edges=nan), "edge 7 is not finite"), (dict(bbox=bb), "bbox of polygon 1"),
                    (dict(edge_off=np.r_[1, tz.edge_off[1:]]), "edge_off must start at 0"),
                    (dict(edge_off=np.array([0, 9, 8, len(tz.edges)])), "edge_off descends at polygon 1"),
                    (dict(uncertain_cap=-1), "uncertain_cap")):
        with pytest.raises(_qalib.QaError, match=pat):
            _qalib.tz_locate(**dict(ok, **kw))
    with pytest.raises(ValueError, match="edge_off"):
        _qalib.tz_locate(**dict(ok, bbox=tz.bbox[:2]))
    with pytest.raises(ValueError, match="lon / lat"):
        _qalib.tz_locate(**dict(ok, lat=[1.0, 2.0]))


def test_step13_refuses_what_it_cannot_read(tmp_path, capsys):
    from topowx_amd import step13
    tzf = TC.write_geojson(str(tmp_path / "s.json"), _case())
    assert step13.main(["--db", str(tmp_path / "none.nc"), "--tz-polygons", tzf]) == 1
    assert "step13:" in capsys.readouterr().err
    (tmp_path / "bad.json").write_text("{not json")
    assert step13.main(["--db", str(tmp_path / "none.nc"), "--tz-polygons", str(tmp_path / "bad.json")]) == 1
    assert "is not JSON" in capsys.readouterr().err
    assert step13.main(["--db", str(tmp_path / "none.nc"), "--tz-polygons", str(tmp_path / "nofile.json")]) == 1
    assert "nofile.json" in capsys.readouterr().err
    import topowx_amd
    assert topowx_amd.UtcOffset is UtcOffset and topowx_amd.add_utc_offset is utc_offsets.add_utc_offset
    assert topowx_amd.load_tz_polygons is load_tz_polygons
