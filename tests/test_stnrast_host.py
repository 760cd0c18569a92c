"""CPU: step19 and the front of step20 without a GPU -- the numpy restatement (tests/restate_stnrast.py) against the
executed-reference golden (tests/golden/make_golden_stnrast.py), the zero-distance criterion of the duplicate search,
``RasterGrid`` and the GeoTIFF reader, the pins of header / binding / build script, and step20's new arguments with the
device calls stood in by the restatement."""
import ctypes
import datetime as dt
import hashlib
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_stnrast as RR  # noqa: E402
from topowx_amd import _qalib, ncio, raster, synth  # noqa: E402
from topowx_amd import stationdb as sdb  # noqa: E402
from topowx_amd.dates import get_days_metadata  # noqa: E402

COMBOS = {"lst": (1, True, True), "tdi": (1, True, False), "cell": (0, False, False)}
NEW_KERNELS = ("k_rv_sample<float>", "k_rv_sample<double>", "k_rv_ring<float>", "k_rv_ring<double>", "k_rv_dup",
               "k_rv_colcount<0>", "k_rv_colcount<1>")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_stnrast_v1.npz"))


def _grid(G, name, cls=RR.Grid):
    band, ndata = float(G[name + "_band_ndata"]), float(G[name + "_ndata"])
    if cls is RR.Grid:
        g = cls(G[name + "_data"], G[name + "_geo_t"], band)
        g.ndata = ndata
        return g
    return cls(G[name + "_data"], G[name + "_geo_t"], ndata, band_ndata=band)


def test_restatement_equals_the_golden(G):
    nruns = nforced = 0
    rings = set()
    for name in G["cases"]:
        for combo in G["combos"]:
            key = "%s_%s_" % (name, combo)
            if key + "value" not in G.files:
                continue
            sel = G[key + "sel"]
            got = RR.add_stn_raster_values(_grid(G, name), G[name + "_lon"][sel], G[name + "_lat"][sel], *COMBOS[str(combo)])
            for k in ("status", "row", "col", "forced"):
                assert np.array_equal(got[k], G[key + k]), (key, k)
            assert got["value"].tobytes() == G[key + "value"].tobytes(), (key, "values bit for bit")
            assert np.array_equal(got["value"] == float(G[name + "_ndata"]), G[key + "ndata_ids"])
            for k, gk in (("ring", "ring_r"), ("winner", "ring_winner"), ("value", "ring_value"), ("dist", "ring_dist"),
                          ("runner_up", "ring_runner_up")):
                a = np.array([nn[k] for nn in got["rings"]], G[key + gk].dtype)
                assert a.tobytes() == G[key + gk].tobytes(), (key, gk)
            rings |= set(G[key + "ring_r"].tolist())
            nforced += got["forced"].size
            nruns += 1
            if not COMBOS[str(combo)][2]:
                assert got["forced"].size == 0
    assert nruns == 13 and nforced > 60 and {1, 2, 9} <= rings
    # the mask raster: the band's 255 keeps masking, 0 is what is written
    assert float(G["mask_ndata"]) == 0.0 and float(G["mask_band_ndata"]) == 255.0
    v = G["mask_cell_value"]
    assert set(np.unique(v).tolist()) == {0.0, 1.0}


def test_quirks_are_in_the_fixture(G):
    """Row 0 and column 0 hold data next to forced stations and are never the answer; west and north of the raster the
    start cell is mirrored into it."""
    g = _grid(G, "lst")
    key = "lst_lst_"
    forced = G[key + "forced"]
    row, col = G[key + "row"][forced], G[key + "col"][forced]
    near_col0 = (col - G[key + "ring_r"] <= 0) & (g.data[row, 0] != g.ndata)
    assert near_col0.any()
    lon = G["lst_lon"][G[key + "sel"]]
    west = lon < g.min_x - 2 * g.geo_t[1]
    assert west.any() and (G[key + "col"][west] >= 3).any()       # abs(int()): not clipped to column 0


def test_zero_distance_criterion(G):
    F = RR.RADIAN
    rs = np.random.RandomState(3)
    lon, lat = rs.uniform(-180, 180, 20000), rs.uniform(-90, 90, 20000)
    lon2, lat2 = lon.copy(), lat.copy()
    k = rs.randint(0, 4, lon.size)
    lon2[k == 1] = np.nextafter(lon[k == 1], 1000.0)
    lat2[k == 2] = np.nextafter(lat[k == 2], -1000.0)
    lon2[k == 3], lat2[k == 3] = rs.uniform(-180, 180, (k == 3).sum()), lat[k == 3]
    zero = RR.grt_circle_dist(lon, lat, lon2, lat2) == 0
    key = (lon * F == lon2 * F) & (lat * F == lat2 * F)
    assert np.array_equal(zero, key)
    raw = (lon == lon2) & (lat == lat2)
    assert (zero & ~raw).sum() > 100                              # one ulp apart, distance 0: raw coordinates are the wrong test
    assert (~zero & (k != 3)).sum() > 100
    assert np.array_equal(_qalib.grt_circle_dist(G["dist_lon"][0], G["dist_lat"][0], G["dist_lon"][1], G["dist_lat"][1]), G["dist_km"])
    assert np.array_equal(RR.grt_circle_dist(G["dist_lon"][0], G["dist_lat"][0], G["dist_lon"][1], G["dist_lat"][1]), G["dist_km"])
    cls, size = RR.dup_classes(G["dup_lon"], G["dup_lat"])
    assert np.array_equal(cls[:, None] == cls[None, :], G["dup_zero"])
    flag = np.where(G["dup_flag"] == -127, 0, G["dup_flag"])
    assert RR.find_dup_stns(G["dup_ids"], G["dup_lon"], G["dup_lat"], flag).tolist() == G["dup_rm"].tolist()
    assert np.array_equal(RR.col_count(G["dup_flag"], None, fill=-127), flag.sum(axis=0))
    assert _qalib.RV_RADIAN == F and _qalib.RV_EARTH_KM == RR.EARTH_KM and _qalib.RV_TIE_REL == RR.TIE_REL


def test_raster_grid_against_the_executed_methods(G):
    for name in G["cases"]:
        name = str(name)
        g = _grid(G, name, raster.RasterGrid)
        yg, xg = g.get_coord_grid_1d()
        assert yg.tobytes() == G[name + "_ygrid"].tobytes() and xg.tobytes() == G[name + "_xgrid"].tobytes()
        y, x = g.get_coord(np.arange(g.rows)[:, None], np.arange(g.cols)[None, :])
        assert np.array_equal(y + 0 * x, G[name + "_ycell"]) and np.array_equal(x + 0 * y, G[name + "_xcell"])
        assert [g.min_x, g.max_x, g.min_y, g.max_y] == G[name + "_extent"].tolist()
        assert np.array_equal(np.ma.getmaskarray(g.read_as_array()), G[name + "_mask"])
        lon, lat = G[name + "_lon"], G[name + "_lat"]
        assert [g.is_inbounds(a, b) for a, b in zip(lon, lat)] == G[name + "_inbounds"].tolist()
        sel = G[name + "_cell_sel"]
        rc = np.array([g.get_row_col(a, b, check_bounds=False) for a, b in zip(lon[sel], lat[sel])])
        assert np.array_equal(rc[:, 0], G[name + "_cell_row"]) and np.array_equal(rc[:, 1], G[name + "_cell_col"])
        out = ~G[name + "_inbounds"]
        if out.any():
            with pytest.raises(ValueError, match="outside raster bounds"):
                g.get_row_col(lon[out][0], lat[out][0])
    with pytest.raises(ValueError, match="rotated"):
        raster.RasterGrid(np.zeros((3, 3)), (0, 1, 0.5, 3, 0, -1), -1)
    with pytest.raises(ValueError, match="north-up"):
        raster.RasterGrid(np.zeros((3, 3)), (0, 1, 0, 3, 0, 1), -1)
    g = raster.RasterGrid(np.ones((3, 3), np.uint8), (0, 1, 0, 3, 0, -1), 255)
    g.ndata = 0                                                   # step19's reassignment leaves the band's value alone
    assert g.band_ndata == 255


# ---- the GeoTIFF reader --------------------------------------------------------------------------------------------------
def write_tiff(path, a, bo="<", tiled=False, deflate=False, nodata=None, scale=(0.25, 0.5), tie=(0, 0, 0, -100.0, 45.0, 0),
               transform=None, compression=None, spp=1, block=16):
    """A tiny classic-TIFF writer: one band (``spp`` only changes the tag), strips of ``block`` rows or ``block`` x ``block``
    tiles, no compression or deflate."""
    rows, cols = a.shape
    kind = {"u": 1, "i": 2, "f": 3}[a.dtype.kind]
    a = a.astype(a.dtype.newbyteorder(bo))
    blobs = []
    if tiled:
        for r0 in range(0, rows, block):
            for c0 in range(0, cols, block):
                t = np.zeros((block, block), a.dtype)
                part = a[r0:r0 + block, c0:c0 + block]
                t[:part.shape[0], :part.shape[1]] = part
                blobs.append(t.tobytes())
    else:
        for r0 in range(0, rows, block):
            blobs.append(a[r0:r0 + block].tobytes())
    if deflate:
        blobs = [zlib.compress(b) for b in blobs]
    comp = compression if compression is not None else (8 if deflate else 1)
    entries = [(256, 4, [cols]), (257, 4, [rows]), (258, 3, [a.dtype.itemsize * 8]), (259, 3, [comp]), (262, 3, [1]),
               (277, 3, [spp]), (284, 3, [1]), (339, 3, [kind])]
    if tiled:
        entries += [(322, 4, [block]), (323, 4, [block]), (324, 4, None), (325, 4, [len(b) for b in blobs])]
    else:
        entries += [(278, 4, [block]), (273, 4, None), (279, 4, [len(b) for b in blobs])]
    if transform is not None:
        entries.append((34264, 12, list(transform)))
    else:
        entries += [(33550, 12, list(scale) + [0.0]), (33922, 12, list(tie))]
    entries.append((34735, 3, [1, 1, 0, 1, 1024, 0, 1, 2]))      # GTModelTypeGeoKey = 2: geographic
    if nodata is not None:
        entries.append((42113, 2, nodata))
    entries.sort(key=lambda e: e[0])
    code = {3: "H", 4: "I", 12: "d"}
    data_at = 8
    body = b"".join(blobs)
    ifd_at = data_at + len(body) + (len(body) & 1)
    extra_at = ifd_at + 2 + 12 * len(entries) + 4
    offs, at = [], data_at
    for b in blobs:
        offs.append(at)
        at += len(b)
    ifd, extra = struct.pack(bo + "H", len(entries)), b""
    for tag, typ, vals in entries:
        if vals is None:
            vals = offs
        if typ == 2:
            raw = vals.encode() + b"\0"
            cnt = len(raw)
        else:
            raw = struct.pack(bo + code[typ] * len(vals), *vals)
            cnt = len(vals)
        if len(raw) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            field = struct.pack(bo + "I", extra_at + len(extra))
            extra += raw + (b"\0" if len(raw) & 1 else b"")
        ifd += struct.pack(bo + "HHI", tag, typ, cnt) + field
    ifd += struct.pack(bo + "I", 0)
    with open(path, "wb") as fh:
        fh.write((b"II" if bo == "<" else b"MM") + struct.pack(bo + "HI", 42, ifd_at) + body + (b"\0" if len(body) & 1 else b""))
        fh.write(ifd + extra)
    return path


@pytest.mark.parametrize("dtype", ["u1", "i2", "u2", "i4", "f4", "f8"])
def test_geotiff_reader(tmp_path, dtype):
    rs = np.random.RandomState(8)
    a = (rs.randn(37, 53) * 50).astype(dtype)
    for bo in "<>":
        for tiled in (False, True):
            for deflate in (False, True):
                p = write_tiff(str(tmp_path / "a.tif"), a, bo, tiled, deflate, nodata="-9999")
                g = raster.from_geotiff(p)
                assert g.data.dtype == np.dtype(dtype) and np.array_equal(g.data, a), (bo, tiled, deflate)
                assert g.geo_t.tolist() == [-100.0, 0.25, 0.0, 45.0, 0.0, -0.5] and g.ndata == -9999.0 == g.band_ndata
    p = write_tiff(str(tmp_path / "t.tif"), a, transform=[0.25, 0, 0, -100.0, 0, -0.5, 0, 45.0, 0, 0, 0, 0, 0, 0, 0, 1])
    g = raster.open_raster(p)
    assert g.geo_t.tolist() == [-100.0, 0.25, 0.0, 45.0, 0.0, -0.5] and g.ndata is None
    p = write_tiff(str(tmp_path / "tie.tif"), a, tie=(2, 3, 0, -100.0, 45.0, 0))     # a tiepoint that is not the corner
    assert raster.from_geotiff(p).geo_t.tolist() == [-100.5, 0.25, 0.0, 46.5, 0.0, -0.5]


def test_geotiff_reader_refusals(tmp_path):
    a = np.arange(12, dtype=np.int16).reshape(3, 4)
    with pytest.raises(NotImplementedError, match=r"Compression \(tag 259\) = 5"):
        raster.from_geotiff(write_tiff(str(tmp_path / "lzw.tif"), a, compression=5))
    with pytest.raises(NotImplementedError, match=r"SamplesPerPixel \(tag 277\) = 2"):
        raster.from_geotiff(write_tiff(str(tmp_path / "two.tif"), a, spp=2))
    with pytest.raises(NotImplementedError, match=r"ModelTransformation \(rotated\) \(tag 34264\)"):
        raster.from_geotiff(write_tiff(str(tmp_path / "rot.tif"), a,
                                       transform=[0.25, 0.1, 0, -100.0, 0.1, -0.5, 0, 45.0, 0, 0, 0, 0, 0, 0, 0, 1]))
    with open(str(tmp_path / "no.tif"), "wb") as fh:
        fh.write(b"not a tiff")
    with pytest.raises(ValueError, match="not a TIFF"):
        raster.from_geotiff(str(tmp_path / "no.tif"))


def test_geotiff_reader_on_a_pillow_file(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from PIL import TiffImagePlugin
    rs = np.random.RandomState(9)
    a = rs.randn(45, 31).astype(np.float32)
    info = TiffImagePlugin.ImageFileDirectory_v2()
    info[33550] = (0.5, 0.25, 0.0)
    info.tagtype[33550] = 12
    info[33922] = (0.0, 0.0, 0.0, -110.0, 40.0, 0.0)
    info.tagtype[33922] = 12
    info[42113] = "-3.4e+38"
    info.tagtype[42113] = 2
    for comp in ("raw", "tiff_adobe_deflate"):
        p = str(tmp_path / ("pil_%s.tif" % comp))
        Image.fromarray(a).save(p, tiffinfo=info, compression=comp)
        g = raster.from_geotiff(p)
        assert np.array_equal(g.data, a) and g.geo_t.tolist() == [-110.0, 0.5, 0.0, 40.0, 0.0, -0.25]
        assert g.ndata == -3.4e+38


# ---- header, binding, build script ---------------------------------------------------------------------------------------
def test_header_binding_and_build():
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxrv_\w+)\s*\(", h))) == sorted(_qalib.RV_EXPORTS) == \
        ["twxrv_col_count", "twxrv_dup_classes", "twxrv_nearest_data", "twxrv_sample"]
    assert h.index("int twxhm_homog_daily(") < h.index("#define TWXRV_F32")        # the new section is the last
    for macro, val in (("TWXRV_F32", _qalib.RV_F32), ("TWXRV_F64", _qalib.RV_F64), ("TWXRV_MAX_EXTENT", _qalib.RV_MAX_EXTENT),
                       ("TWXRV_MAX_DUP_STNS", _qalib.RV_MAX_DUP_STNS), ("TWXRV_COUNT_I8_SUM", _qalib.RV_COUNT_I8_SUM),
                       ("TWXRV_COUNT_F32_MISSING", _qalib.RV_COUNT_F32_MISSING), ("TWXRV_NTIMES", _qalib.RV_NTIMES),
                       ("TWXRV_NEAREST", _qalib.RV_NEAREST), ("TWXRV_NODATA", _qalib.RV_NODATA),
                       ("TWXRV_NEEDS_FORCE", _qalib.RV_NEEDS_FORCE), ("TWXRV_NO_DATA_ANYWHERE", _qalib.RV_NO_DATA_ANYWHERE)):
        assert re.search(r"#define %s %d\b" % (macro, val), h), macro
    assert re.search(r"#define TWXRV_TIE_REL 1e-9\b", h) and _qalib.RV_TIE_REL == 1e-9
    # new status numbers from 35 up: the unit before ends at 34 and nothing else uses 35 .. 38
    assert re.search(r"#define TWXHM_OVERLAP 34\b", h)
    assert (_qalib.RV_NEAREST, _qalib.RV_NODATA, _qalib.RV_NEEDS_FORCE, _qalib.RV_NO_DATA_ANYWHERE) == (35, 36, 37, 38)
    assert not re.findall(r"#define TWX(?!RV_)\w+_\w+ (?:35|36|37|38) +/\*", h)
    assert 8 * (_qalib.RV_MAX_EXTENT + 1) + 2 <= 2 ** 31 - 1 + 8
    assert (RR.OK, RR.NEAREST, RR.NODATA, RR.NEEDS_FORCE, RR.NO_DATA_ANYWHERE) == (0, 35, 36, 37, 38)
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_stnrast.hip" in build and os.path.exists(os.path.join(ROOT, "topowx_amd", "qa", "twx_stnrast.hip"))
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_stnrast.hip")).read()
    for k in ("k_rv_sample", "k_rv_ring", "k_rv_dup", "k_rv_colcount"):
        assert re.search(r"void %s\(" % k, src), k
    assert "0.017453292519943295" in src and "6371.009" in src
    import topowx_amd.infill as infill
    for name in ("add_stn_raster_values", "find_dup_stns"):
        assert name in infill.__all__ and callable(getattr(infill, name)), name
    from topowx_amd import step19
    jobs = step19.raster_jobs()
    assert len(jobs) == 30 and len({j[4] for j in jobs}) == 27   # 24 LST rasters and three that serve both databases
    assert [j[6] for j in jobs if j[1] == sdb.MASK] == [dict(extract_method=0)] * 2 and [j[5] for j in jobs if j[1] == sdb.MASK] == [0, 0]


def test_resource_table_lists_the_new_kernels():
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.RV_EXPORTS:
        assert hasattr(lib, name), name
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, (k, [t for t in table if t.startswith("k_rv")])
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    assert table["k_rv_dup"]["lds"] == 2 * 8 * 256 and table["k_rv_colcount<0>"]["lds"] == 4 * 256


def test_call_level_refusals_need_no_device():
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    with pytest.raises(ValueError, match="2"):
        _qalib.raster_sample(np.ones((1, 1)), (0, 1, 0, 1, 0, -1), -1.0, [0.5], [0.5])
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    geo = (ctypes.c_double * 6)(0, 1, 0, 1, 0, -1)
    lib.twxrv_sample.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int64] + [ctypes.c_void_p] * 2 + \
        [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 5 + [ctypes.c_char_p, ctypes.c_int]
    rc = lib.twxrv_sample(0, 1, 5, 0, None, geo, 0, 0.0, -1.0, 1, None, None, 1, 0, 0, None, None, None, None, None, buf, 256)
    assert rc != 0 and b"at least 2 x 2" in buf.value            # refused before any device work
    assert _qalib.col_count(np.zeros((4, 3), np.int8), []).size == 0


# ---- step20 with and without the new arguments ---------------------------------------------------------------------------
def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _serial_db(var, n=40):
    days = get_days_metadata(dt.date(1981, 1, 1), dt.date(1981, 1, 20))
    return synth.make_stations((40.0, 42.0, -110.0, -108.0), n, 5, var, days, with_obs=True, nan_frac=0.0)


def _write_infill_db(path, db, var, flag, fmt):
    ncio.create_quick_db(path, db.stns, db.days, [(var, "f4", float(ncio.FILL_F4), "", "C"),
                                                  ("flag_infilled", "i1", -127, "infilled flag", "")], format=fmt)
    ds = ncio.open_dataset(path, "a")
    ds.variables[var][:] = db.var
    ds.variables["flag_infilled"][:] = flag
    ds.close()


def _stub_device(monkeypatch):
    """The three device calls behind step20's new arguments, stood in by the restatement."""
    from topowx_amd import step20
    monkeypatch.setattr(_qalib, "dup_classes", lambda lon, lat, **kw: RR.dup_classes(lon, lat))
    monkeypatch.setattr(_qalib, "col_count", lambda data, cols=None, fill=None, **kw: RR.col_count(
        data, cols, float(ncio.FILL_F4) if fill is None and np.asarray(data).dtype == np.float32 else fill))
    monkeypatch.setattr(step20, "screen", lambda da, *a, **kw: (int(np.isnan(da.stns[sdb.BAD]).sum()),
                                                                np.array([da.stn_ids[1]]), 0.0))


@pytest.mark.parametrize("fmt", ncio.FORMATS)
def test_step20_front_and_final_check(tmp_path, monkeypatch, capsys, fmt):
    from topowx_amd import step20
    if fmt == "NETCDF4" and ncio.default_format() != "NETCDF4":
        pytest.skip("libhdf5 not loadable here")
    _stub_device(monkeypatch)
    paths, ipaths, want = {}, {}, {}
    rs = np.random.RandomState(4)
    for var in ("tmin", "tmax"):
        db = _serial_db(var)
        n = db.stns.size
        db.stns[sdb.LON][[7, 30]] = db.stns[sdb.LON][3]               # a class of three: 3, 7, 30
        db.stns[sdb.LAT][[7, 30]] = db.stns[sdb.LAT][3]
        db.stns[sdb.LON][21], db.stns[sdb.LAT][21] = db.stns[sdb.LON][20], db.stns[sdb.LAT][20]     # tied counts: both kept
        db.stns[sdb.TDI][[4, 9]] = np.nan
        db.stns[sdb.CLIMDIV][[9, 12, 15]] = np.nan
        db.stns[sdb.MASK][15] = np.nan                                 # outside the mask: no climate division is no fault
        db.stns[sdb.BAD][[0, 2]] = 1.0                                 # reset=True: forgotten
        flag = (rs.rand(db.days.size, n) < 0.3).astype(np.int8)
        flag[:, 3], flag[:, 7], flag[:, 30] = 0, 1, 0
        flag[:3, 30] = 1
        flag[:, 21] = flag[:, 20]
        paths[var], ipaths[var] = str(tmp_path / ("serial_%s.nc" % var)), str(tmp_path / ("infill_%s.nc" % var))
        ncio.write_station_db(paths[var], db, format=fmt)
        _write_infill_db(ipaths[var], db, var, flag, fmt)
        ids = db.stn_ids
        want[var] = dict(no_tdi={ids[4], ids[9]}, no_climdiv={ids[9], ids[12]}, dup={ids[7], ids[30]})
    csv = str(tmp_path / "flagged_bad.csv")
    with open(csv, "w") as fh:
        fh.write("station_id,reason\n%s,infill issue\n%s,infill issue\nNOT_THERE,infill issue\n" % (ids[25], ids[25]))
    argv = ["--tmin", paths["tmin"], "--tmax", paths["tmax"], "--infill-tmin", ipaths["tmin"], "--infill-tmax", ipaths["tmax"],
            "--flagged-bad", csv]
    before = {v: _sha(p) for v, p in paths.items()}
    assert step20.main(argv + ["--dry-run"]) == 0
    assert {v: _sha(p) for v, p in paths.items()} == before          # --dry-run writes nothing
    capsys.readouterr()
    assert step20.main(argv) == 0
    out = capsys.readouterr().out
    for var in ("tmin", "tmax"):
        assert "7 total stations removed for %s:" % var in out       # with the id that is in no database, as the reference counts
    for line in ("2 stations removed due to infilling issues", "2 stations removed due to no TDI values",
                 "2 stations removed due no climate division value, but within domain mask",
                 "2 stations removed due to being duplicates", "Performing final checks"):
        assert line in out, line
    for var in ("tmin", "tmax"):
        da = sdb.StationSerialDataDb(paths[var], var)
        ida = sdb.StationSerialDataDb(ipaths[var], var)
        try:
            flagged = set(da.stn_ids[~np.isnan(da.stns[sdb.BAD])].tolist())
            parts = step20.front(da, ida, step20.read_flagged_bad(csv), out=open(os.devnull, "w"))
        finally:
            da.close()
            ida.close()
        w = want[var]
        assert (set(parts["no_tdi"]), set(parts["no_climdiv"]), set(parts["dup"])) == (w["no_tdi"], w["no_climdiv"], w["dup"])
        assert set(parts["bad"]) == {ids[25], "NOT_THERE"}
        assert flagged == w["no_tdi"] | w["no_climdiv"] | w["dup"] | {ids[25], ids[1]}     # and the stubbed outlier
    # the final check: a good station with a missing day
    ds = ncio.open_dataset(paths["tmax"], "a")
    col = np.array(ds.variables["tmax"][:, 17])
    col[5] = ncio.FILL_F4
    ds.variables["tmax"][:, 17] = col
    ds.close()
    assert step20.main(argv) == 1
    assert "Missing values found in %s" % paths["tmax"] in capsys.readouterr().err
    with pytest.raises(SystemExit):
        step20.main(argv[:6])                                         # the three arguments come together


def test_step20_without_the_new_arguments_is_unchanged(tmp_path, monkeypatch, capsys):
    """The old flow, restated here from the parent's ``main``: screen both, then ``set_bad_stations(union, reset=False)``."""
    from topowx_amd import step20
    _stub_device(monkeypatch)
    monkeypatch.setattr(step20, "front", lambda *a, **kw: pytest.fail("the front must not run"))
    monkeypatch.setattr(step20, "final_check", lambda *a, **kw: pytest.fail("the final check must not run"))
    new, old = {}, {}
    for var in ("tmin", "tmax"):
        db = _serial_db(var)
        db.stns[sdb.BAD][[0, 2]] = 1.0
        for d, tag in ((new, "new"), (old, "old")):
            d[var] = str(tmp_path / ("%s_%s.nc" % (tag, var)))
            ncio.write_station_db(d[var], db, format="NETCDF3_64BIT")
    assert _sha(new["tmin"]) == _sha(old["tmin"])
    assert step20.main(["--tmin", new["tmin"], "--tmax", new["tmax"]]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and all(line.startswith('{"var": ') for line in lines)      # nothing but the two JSON lines
    dbs = [sdb.StationSerialDataDb(old[v], v, mode="r+") for v in ("tmin", "tmax")]
    union = np.unique(np.array([str(s) for da in dbs for s in step20.screen(da)[1]], dtype=str))
    for da in dbs:
        step20.set_bad_stations(da, union, reset=False)
        da.close()
    for var in ("tmin", "tmax"):
        assert _sha(new[var]) == _sha(old[var]), var


@pytest.mark.parametrize("fmt", ncio.FORMATS)
def test_from_netcdf(tmp_path, fmt):
    if fmt == "NETCDF4" and ncio.default_format() != "NETCDF4":
        pytest.skip("libhdf5 not loadable here")
    p = str(tmp_path / "tdi.nc")
    ds = ncio.open_dataset(p, "w", fmt)
    ds.createDimension("lat", 4)
    ds.createDimension("lon", 5)
    la, lo = ds.createVariable("lat", "f8", ("lat",)), ds.createVariable("lon", "f8", ("lon",))
    la[:] = np.array([43.75, 43.25, 42.75, 42.25])
    lo[:] = -110 + 0.25 * np.arange(5)
    v = ds.createVariable("tdi", "f4", ("lat", "lon"), fill_value=-9999.0)
    a = np.arange(20, dtype=np.float32).reshape(4, 5)
    a[1, 2] = -9999.0
    v[:] = a
    ds.close()
    g = raster.open_raster(p)
    assert g.geo_t.tolist() == [-110.125, 0.25, 0.0, 44.0, 0.0, -0.5] and g.ndata == -9999.0
    assert np.array_equal(g.data, a) and np.ma.getmaskarray(g.read_as_array()).sum() == 1
    from topowx_amd import step19
    os.makedirs(str(tmp_path / "r"))
    os.rename(p, str(tmp_path / "r" / "tdi.nc"))
    assert step19.find_raster(str(tmp_path / "r"), "tdi").endswith("tdi.nc")     # a .nc in a GeoTIFF's place
    with pytest.raises(IOError):
        step19.find_raster(str(tmp_path / "r"), "mask")
