"""Step12 (the reanalysis subsets) without a GPU: the restatement against the executed reference (the golden fixture) in
every hash, count and sample; the calendar; the argument checks of ``twxns_subset`` through the built library, all made
before anything touches a device; the writer's files in both containers under ``NNRNghData``; and the kernels' index
mapping (twx_nnrsub_map.h) run on the CPU under the address and undefined-behaviour sanitizers as a program of its own."""
import datetime as dt
import hashlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import nnrsub_cases as NC  # noqa: E402
import restate_nnrsub as RN  # noqa: E402
from topowx_amd import _qalib, h5nc, ncio, reanalysis, step12  # noqa: E402
from topowx_amd.dates import YMD, get_days_metadata  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "golden_nnrsub_v1.npz"))
FORMATS = [pytest.param("NETCDF4", marks=pytest.mark.skipif(not h5nc.available(), reason="libhdf5 not loadable")),
           "NETCDF3_64BIT"]
needs_lib = pytest.mark.skipif(not os.path.exists(_qalib.LIB_PATH), reason="no build in this checkout (run ./build.sh)")


@pytest.fixture(scope="module")
def restated():
    """{file stem: (array [ndays, nlev, 6, 7], counts [3], levels or None)} of the 21 products, computed once."""
    days, out = NC.days(), {}
    for raw_var, products in NC.PRODUCTS:
        _, pack, mv, fv, _, _ = NC.VARS[raw_var]
        scale, offset = pack if pack is not None else (1, 0)
        outs, counts, levs = RN.route([NC.year_raw(raw_var, y) for y in NC.YEARS], [NC.year_times(y) for y in NC.YEARS], NC.EPOCH,
                                      NC.START, days.size, scale, offset, (mv, fv), NC.LEVELS, NC.LONS, NC.LATS, products)
        for p, a, c, lv in zip(products, outs, counts, levs):
            a.setflags(write=False)
            out[p["fname"][:-3]] = (a, c, lv)
    return out


def test_fixture_is_of_these_inputs():
    assert str(GOLD["input_sha"]) == NC.checksum()
    assert len(GOLD["names"]) == 21 and step12.PRODUCTS == NC.PRODUCTS
    assert os.path.getsize(os.path.join(HERE, "golden", "golden_nnrsub_v1.npz")) < 1 << 17


def test_restatement_equals_the_executed_reference(restated):
    assert sorted(restated) == sorted(str(n) for n in GOLD["names"])
    nmarked = 0
    for name, (a, counts, _) in restated.items():
        shape = tuple(GOLD[name + "/shape"])
        assert a.size == np.prod(shape) and a.shape[0] == shape[0] and a.shape[-2:] == shape[-2:] == (6, 7), name
        assert hashlib.sha256(a.tobytes()).hexdigest() == str(GOLD[name + "/sha"]), name
        assert list(counts) == list(GOLD[name + "/counts"]), name
        assert a.ravel()[GOLD[name + "/idx"]].tobytes() == GOLD[name + "/val"].tobytes(), name
        nmarked += int(counts[1])
    assert nmarked > 1000
    # what the cases pin: the 24z of the last day stays fill, a mark on one level of the pair fills the thickness
    a, c, _ = restated["nnr_thick_18z"]
    assert (a[1, 0, 1, 2] == NC.FILL_F4) and list(restated["nnr_thick_24z"][1]) == [730, restated["nnr_thick_24z"][1][1], 1]
    assert (restated["nnr_slp_24z"][0][-1] == NC.FILL_F4).all() and not (restated["nnr_slp_24z"][0][:-1] == NC.FILL_F4).any()
    assert np.signbit(restated["nnr_rhum_18z"][0][1, 0, 1, 1]) and restated["nnr_rhum_18z"][0][1, 0, 1, 1] == 0       # -0 survives


def test_calendar():
    days = NC.days()
    for y in NC.YEARS:
        slot, day = reanalysis.record_slots_days(NC.year_times(y), NC.UNITS, days)
        s2, d2 = RN.slots_days(NC.year_times(y), NC.EPOCH, NC.START, days.size)
        assert np.array_equal(slot, s2) and np.array_equal(day, d2)
    # 24z across the year boundary: the first record of 2001 is the 24z of 31 December 2000
    slot, day = reanalysis.record_slots_days(NC.year_times(2001), NC.UNITS, days)
    assert slot[0] == 2 and days[YMD][day[0]] == 20001231 and slot[1] == -1 and slot[2] == 0 and days[YMD][day[2]] == 20010101
    # the first record of 2000 falls before the period; nothing gives the last day its 24z
    slot0, day0 = reanalysis.record_slots_days(NC.year_times(2000), NC.UNITS, days)
    assert slot0[0] == 2 and day0[0] == -1
    assert days.size - 1 not in set(day[slot == 2]) | set(day0[slot0 == 2]) and days.size - 1 in set(day[slot == 1])
    # a period that starts and ends mid-year
    mid = get_days_metadata(dt.date(2000, 6, 15), dt.date(2001, 3, 10))
    slot, day = reanalysis.record_slots_days(NC.year_times(2000), NC.UNITS, mid)
    s2, d2 = RN.slots_days(NC.year_times(2000), NC.EPOCH, dt.date(2000, 6, 15), mid.size)
    assert np.array_equal(slot, s2) and np.array_equal(day, d2)
    # 200 days of 2000: the 0z of 15 June belongs to the 14th, the 0z of 1 January 2001 is in the next file
    assert (day >= 0).sum() == 4 * 200 - 1 and mid[YMD][day[day >= 0][0]] == 20000615 and day[slot == 2].max() == 199 - 1
    slot, day = reanalysis.record_slots_days(NC.year_times(2001), NC.UNITS, mid)
    assert mid[YMD][day.max()] == 20010310 and (day >= 0).sum() == 4 * 69 + 1 and day[0] == 199 and slot[0] == 2
    # a gap in time, an epoch of year 1
    t = NC.year_times(2000)
    with pytest.raises(ValueError, match=r"hgt\.2000\.nc: time holds 1463 records, but 1464"):
        reanalysis.record_slots_days(np.delete(t, 100), NC.UNITS, days, "hgt.2000.nc")
    with pytest.raises(ValueError, match="gap"):
        RN.slots_days(np.delete(t, 100), NC.EPOCH, NC.START, days.size)
    with pytest.raises(ValueError, match=r"air\.1948\.nc.*before 1583"):
        reanalysis.record_slots_days(t, "hours since 1-1-1 00:00:0.0", days, "air.1948.nc")
    with pytest.raises(ValueError, match="not 'hours since"):
        reanalysis.record_slots_days(t, "days since 1800-01-01", days)
    assert step12.period(2000, 2000)[YMD][[0, -1]].tolist() == [20000101, 20011231]


@pytest.mark.parametrize("fmt", FORMATS)
def test_yearly_files_with_a_gap_or_an_old_epoch_are_refused_by_name(tmp_path, fmt):
    """Through the files: the check is made on what the reader returns, before any library call."""
    days = NC.days()
    raw, t = NC.year_raw("slp", 2000)[:40], NC.year_times(2000, 40)
    NC.write_raw_file(str(tmp_path / "slp.2000.nc"), "slp", 2000, fmt, raw=raw[:39], times=np.delete(t, 7))
    NC.write_raw_file(str(tmp_path / "slp.2001.nc"), "slp", 2001, fmt, raw=raw, times=t, units="hours since 1-1-1 00:00:0.0")
    prods = [dict(fname="x.nc", varname_out="slp", utc_time=12)]
    with pytest.raises(ValueError, match=r"slp\.2000\.nc: time holds 39 records"):
        reanalysis.create_nnr_subsets(str(tmp_path), str(tmp_path), [2000], days, "slp", prods, format=fmt)
    with pytest.raises(ValueError, match=r"slp\.2001\.nc.*before 1583"):
        reanalysis.create_nnr_subsets(str(tmp_path), str(tmp_path), [2001], days, "slp", prods, format=fmt)
    with pytest.raises(IOError, match=r"no reanalysis file .*slp\.2002\.nc"):
        reanalysis.create_nnr_subsets(str(tmp_path), str(tmp_path), [2002], days, "slp", prods, format=fmt)
    assert step12.main(["--nnr-raw", str(tmp_path), "--out", str(tmp_path / "o"), "--start-year", "2000", "--end-year", "2000",
                        "--format", fmt]) == 1
    assert not (tmp_path / "x.nc").exists()


@needs_lib
def test_argument_errors_come_before_any_device_work():
    """None of these reaches the device: they pass on a machine without one."""
    raw = np.zeros((4, 2, 3, 5), np.int16)
    ok = dict(raw=raw, scale=0.01, offset=477.65, marks=(32766, None), rec_slot=[0, 1, 2, -1], rec_day=[0, 0, 0, -1], ndays=2,
              lat_idx=[0, 2], lon_idx=[4, 1, 0], products=[dict(slot=0, levels=[0, 1]), dict(slot=2, thick=(1, 0), conv="k_to_c")])
    many = [dict(slot=0, levels=[0])] * (_qalib.NS_MAX_PROD + 1)
    for kw, pat in ((dict(rec_slot=[0, 1, 0, -1]), "records 0 and 2 both map to slot 0, day 0"),
                    (dict(lat_idx=[0, 3]), "lat_idx entry is out of range"), (dict(lon_idx=[5]), "lon_idx entry is out of range"),
                    (dict(lon_idx=[-1]), "lon_idx entry is out of range"),
                    (dict(products=[dict(slot=0, levels=[2])]), "product 0: level index 2 is out of range"),
                    (dict(products=[dict(slot=0, levels=[0]), dict(slot=1, thick=(0, 2))]), "product 1: level index 2"),
                    (dict(products=[dict(slot=0, levels=[])]), "need 1 <= nlev_out <= TWXNS_MAX_LEV = 32, got 0"),
                    (dict(products=[dict(slot=0, levels=[0] * 33)]), "TWXNS_MAX_LEV = 32, got 33"),
                    (dict(products=[dict(slot=1, thick=(1, 1))]), "two different levels, got index 1 twice"),
                    (dict(products=[dict(slot=3, levels=[0])]), "slot must be 0, 1 or 2"),
                    (dict(dtype=2), "dtype must be"), (dict(layout=2), "layout must be"),
                    (dict(rec_day=[0, 0, 2, -1]), "record 2: slot 2, day 2"), (dict(rec_slot=[0, 1, 3, -1]), "record 2: slot 3"),
                    (dict(products=many), "TWXNS_MAX_PROD = 64"), (dict(products=[]), "TWXNS_MAX_PROD"),
                    (dict(ndays=_qalib.NS_MAX_DAYS + 1), r"TWXNS_MAX_DAYS = 1048576"),
                    (dict(lon_idx=[0] * (_qalib.NS_MAX_SIDE + 1)), "TWXNS_MAX_SIDE = 4096"), (dict(ndays=0), "TWXNS_MAX_DAYS")):
        with pytest.raises(_qalib.QaError, match=pat):
            _qalib.ns_subset(**dict(ok, **kw))
    with pytest.raises(ValueError, match="int16 or float32"):
        _qalib.ns_subset(**dict(ok, raw=raw.astype(np.float64)))
    with pytest.raises(ValueError, match="conv"):
        _qalib.ns_subset(**dict(ok, products=[dict(slot=0, levels=[0], conv="c_to_k")]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_written_files_open_in_the_reader(tmp_path, fmt, restated):
    """The 21 files written from the restatement's arrays (the PLAIN route; in NetCDF-4 also the chunk route from tiled
    bytes): the reader's axes, the arrays, and the matrix of a point."""
    days = NC.days()
    lons, mlon, mlat = RN.masks(NC.LONS, NC.LATS)
    for raw_var, products in NC.PRODUCTS:
        for p in products:
            a, _, lv = restated[p["fname"][:-3]]
            reanalysis.write_nnr_subset(str(tmp_path / p["fname"]), reanalysis._title(p), p["varname_out"], days, lons[mlon],
                                        NC.LATS[mlat], lv, a, False, format=fmt)
    assert ncio.file_format(str(tmp_path / "nnr_hgt_12z.nc")) == fmt
    nn = reanalysis.NNRNghData(str(tmp_path), (20000301, 20010630))
    try:
        assert nn.days[YMD][[0, -1]].tolist() == [20000301, 20010630] and nn.day_mask[0] == 60
        assert nn.nnr_lons.tolist() == [-132 + 12 * k for k in range(7)] and nn.nnr_lats.tolist() == [60, 50, 40, 30, 20, 10]
        ds = nn.ds_nnr["hgt12z"]
        v = ds.variables["hgt"]
        assert tuple(v.dimensions) == ("time", "level", "lat", "lon") and ds.variables["level"][:].tolist() == [700.0, 500.0]
        assert v[:].tobytes() == restated["nnr_hgt_12z"][0].tobytes() and np.float32(v.getncattr("_FillValue")) == NC.FILL_F4
        assert ds.getncattr("title") == "NCEP/NCAR Daily hgt 12Z Subset"
        assert nn.ds_nnr["thick24z"].getncattr("title") == "NCEP/NCAR Daily 500-1000 thickness 24Z Subset"
        tv = ds.variables["time"]
        assert tv.getncattr("units") == "days since 2000-1-1 0:0:0" and tv[:].tolist() == list(range(731)) and tv.calendar == "standard"
        assert tuple(nn.ds_nnr["slp18z"].variables["slp"].dimensions) == ("time", "lat", "lon")
        if fmt == "NETCDF4":
            assert v.chunking() == [731, 2, 4, 4] and nn.ds_nnr["slp18z"].variables["slp"].chunking() == [731, 4, 4]
    finally:
        nn.close()
    # the matrix of a point whose four nearest cells hold no mark on ten days, found from the arrays
    nn = reanalysis.NNRNghData(str(tmp_path), (20000305, 20000314))
    try:
        d0 = int(nn.day_mask[0])
        free = np.ones((6, 7), bool)
        for name in nn.NNR_VARS:
            free &= ~(restated["nnr_%s_18z" % name][0][d0:d0 + 10] == NC.FILL_F4).any(axis=(0, 1))
        pts = [(nn.nnr_lons[j] + 5.0, nn.nnr_lats[i] - 4.0) for i in range(5) for j in range(6)]
        pts = [pt for pt in pts if free.ravel()[nn.nearest_cells(*pt)].all()]
        assert pts and nn.days.size == 10
        order = nn.nearest_cells(*pts[0])
        m = nn.get_nngh_matrix(pts[0][0], pts[0][1], "tmax", -5)
        want = np.hstack([restated["nnr_%s_18z" % name][0][d0:d0 + 10, :, c // 7, c % 7] for c in order for name in nn.NNR_VARS])
        assert m.tobytes() == want.tobytes() and m.shape == (10, 32)
    finally:
        nn.close()
    if fmt == "NETCDF4":
        for name in ("nnr_hgt_12z", "nnr_slp_24z"):
            a, _, lv = restated[name]
            reanalysis.write_nnr_subset(str(tmp_path / "tiled.nc"), "t", "x", days, lons[mlon], NC.LATS[mlat], lv, RN.tile(a), True,
                                        format=fmt)
            with ncio.open_dataset(str(tmp_path / "tiled.nc")) as ds:
                assert ds.variables["x"][:].tobytes() == a.tobytes()
            assert reanalysis.untile(RN.tile(a), 6, 7).tobytes() == a.tobytes()


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "nnrsub_hostcheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "topowx_amd", "qa"), os.path.join(HERE, "tools", "nnrsub_hostcheck.cpp"),
                           "-o", exe])
    return exe


def test_index_mapping_on_the_cpu_under_sanitizers(hostcheck):
    """Every thread of a launch, and the threads past its end, over the edge shapes of the GPU tests: each output element
    owned exactly once, every offset inside its buffer, the padding where the layout says; a clean exit."""
    for ndays in (1, 63, 64, 65, 257):
        for nlat, nlon in ((1, 1), (4, 4), (5, 3), (6, 7), (21, 33)):
            for nlev in (1, 2):
                res = subprocess.run([hostcheck, str(ndays), str(nlev), str(nlat), str(nlon)], capture_output=True, text=True)
                assert res.returncode == 0 and res.stderr == "", (ndays, nlat, nlon, nlev, res.stdout[-500:], res.stderr[-2000:])


def test_unit_is_declared_bound_and_built():
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxns_\w+)\s*\(", h))) == sorted(_qalib.NS_EXPORTS)
    for name, val in (("NKERNELS", len(_qalib.NS_KERNELS)), ("MAX_LEV", _qalib.NS_MAX_LEV), ("MAX_PROD", _qalib.NS_MAX_PROD),
                      ("MAX_SIDE", _qalib.NS_MAX_SIDE), ("C_N", 3), ("TILED", _qalib.NS_TILED), ("PLAIN", _qalib.NS_PLAIN),
                      ("I16", _qalib.NS_I16), ("F32", _qalib.NS_F32), ("CONV_K_TO_C", _qalib.NS_CONV["k_to_c"])):
        assert int(re.search(r"#define TWXNS_%s (\d+)" % name, h).group(1)) == val, name
    assert np.float32(float(re.search(r"#define TWXNS_FILL ([0-9.e]+)f", h).group(1))) == ncio.FILL_F4 == _qalib.NS_FILL
    assert "topowx_amd/qa/twx_nnrsub.hip" in open(os.path.join(ROOT, "build.sh")).read()
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    import ctypes
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    assert all(hasattr(lib, n) for n in _qalib.NS_EXPORTS)
    rows = {l.split("|")[0].strip(): [c.strip() for c in l.split("|")] for l in open(res) if l.startswith("k_nsub_")}
    assert sorted(rows) == ["k_nsub_plain<float>", "k_nsub_plain<short>", "k_nsub_tiled<float>", "k_nsub_tiled<short>"]
    head = [c.strip() for c in open(res).readline().split("|")]
    for word in ("scratch", "spills"):
        k = [i for i, c in enumerate(head) if word in c.lower()]
        assert k and all(int(r[k[0]]) == 0 for r in rows.values())
