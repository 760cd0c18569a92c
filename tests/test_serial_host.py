"""CPU: step17 / step18 without a GPU -- the numpy restatement (tests/restate_serial.py) against the executed-reference
golden (tests/golden/make_golden_serial.py): runs, decisions, flags, missing positions and the serial bytes exactly, the
normals bit for bit; the log parser and ``suspect_infill_stnids`` against the fixture; the group ranges of the binding;
header / binding / build naming; the resource table of a build; the writer of the infilled database; the call-level
failures of the two ``twxsc_`` entries (they come before any device work) and the error paths of the two command lines."""
import ctypes
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_serial as RS  # noqa: E402
import serial_cases as SC  # noqa: E402

from topowx_amd import _qalib, ncio  # noqa: E402
from topowx_amd.dates import DAY, MONTH, YEAR, get_days_metadata  # noqa: E402
from topowx_amd.infill import (SERIAL_DB_VARIABLES, USE_ALL_INFILL_THRESHOLD, get_bad_infill_stnids, suspect_infill_stnids,  # noqa: E402
                               write_bad_stns_csv, write_infill_db)

NEW_KERNELS = ("k_sc_select", "k_sc_norms", "k_sc_series")


@pytest.fixture(scope="module")
def gold():
    return SC.load_gold()


def test_golden_content(gold):
    path = os.path.join(ROOT, "tests", "golden", "golden_serial_v1.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_spatial_v1.npz"))
    assert gold["db_fnl"].shape == (16, 2922) and gold["db_norm_yrs"].tolist() == [1981, 1984]
    assert (gold["db_year"][0], gold["db_year"][-1]) == (1979, 1986) and int(gold["norm_bits_differ"]) == 0
    assert gold["db_max_run"][[1, 2, 4, 5, 6]].tolist() == [2190, 1826, 1825, 1826, 1827]
    assert gold["db_all_infill"].tolist() == [s in (1, 2, 5, 6, 9) for s in range(16)]
    assert (gold["db_flag"][9] == -127).all() and gold["db_max_run"][9] == 2922      # the int8 fill counts as infilled
    assert gold["runs_thresholds"].tolist() == [1, 5, 30, 31, 420]
    assert gold["runs_all_infill"].sum(axis=1).tolist() == [14, 12, 9, 5, 2]


def test_restatement_equals_the_golden_runs(gold):
    for k, t in enumerate(gold["runs_thresholds"]):
        r = RS.serial_complete(gold["runs_tair"], gold["runs_tinf"], gold["runs_flag"], run_threshold=int(t))
        assert np.array_equal(r["max_run"], gold["runs_max_run"]) and np.array_equal(r["all_infill"], gold["runs_all_infill"][k])
        assert np.array_equal(r["flag_infilled"], gold["runs_flag_out"][k])
        assert r["serial"].tobytes() == gold["runs_serial"][k].tobytes()
        assert np.array_equal(r["miss"], gold["runs_serial"][k] == RS.FILL_F4)
        assert np.array_equal(r["nmissing"], (gold["runs_serial"][k] == RS.FILL_F4).sum(axis=1))
    assert (r["nmissing"] > 0).all()                                 # NaN, +-Inf and the fill sit in both sources


def test_restatement_equals_the_golden_database(gold):
    """Integers, masks and the serial bytes exactly; the normals BIT FOR BIT (numpy's axis-0 reduction adds row after row, as
    the day-order sum does: the maker counted 0 differing entries)."""
    gf, gn = RS.norm_groups(gold["db_year"], gold["db_month"], 1981, 1984)
    assert np.array_equal(gf, gold["db_group_first"]) and np.array_equal(gn, gold["db_group_ndays"])
    for key, max_miss in (("9", 9), ("none", None)):
        r = RS.serial_complete(gold["db_fnl"], gold["db_model"], gold["db_flag"], group_first=gf, group_ndays=gn, max_miss=max_miss)
        assert np.array_equal(r["max_run"], gold["db_max_run"]) and np.array_equal(r["all_infill"], gold["db_all_infill"])
        assert np.array_equal(r["flag_infilled"], gold["db_flag_out"]) and r["serial"].tobytes() == gold["db_serial"].tobytes()
        assert np.array_equal(r["norm_nmths"], gold["db_nmths_" + key])
        assert r["norm"].tobytes() == gold["db_norm_" + key].tobytes(), key
    # what the planted stations are for
    nm9, nmn = gold["db_nmths_9"], gold["db_nmths_none"]
    assert nm9[3].tolist() == [4] * 10 + [3, 3] and nmn[3].tolist() == [4] * 12        # 1981: 10 and 11 missing days
    assert nm9[7, 5] == 3 and nmn[7, 5] == 3                                           # June 1982 wholly missing
    assert nm9[8, 1] == 0 and np.isnan(gold["db_norm_9"][8, 1]) and nmn[8, 1] == 4     # February masked in every year
    assert (nm9[9] == 0).all() and np.isnan(gold["db_norm_none"][9]).all()             # all fill
    assert nm9[10, 2] == 3 and nmn[10, 2] == 4                                         # 9 missing days stay, 10 do not
    assert (nm9[0] == 4).all()


def test_binding_groups_equal_the_loop(gold):
    gf, gn = _qalib.norm_groups(gold["db_year"], gold["db_month"], 1981, 1984)
    assert np.array_equal(gf, gold["db_group_first"]) and np.array_equal(gn, gold["db_group_ndays"]) and gf.dtype == np.int32
    days = get_days_metadata(dt.date(1983, 3, 5), dt.date(1985, 2, 3))              # an axis that begins and ends inside a month
    a, b = _qalib.norm_groups(days[YEAR], days[MONTH], 1981, 1986), RS.norm_groups(days[YEAR], days[MONTH], 1981, 1986)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0][a[1] > 0], b[0][b[1] > 0]) and a[1].sum() == days.size
    assert a[1][:26].sum() == 0 and a[1][26] == 27 and a[1][49] == 3
    keep = np.ones(days.size, bool)
    keep[80:160] = False                                                             # two skipped months
    with pytest.raises(ValueError, match="gap-free"):
        _qalib.norm_groups(days[YEAR][keep], days[MONTH][keep], 1981, 1986)
    keep[:] = True
    keep[100] = False                                                                # one skipped day: seen only day by day
    assert _qalib.norm_groups(days[YEAR][keep], days[MONTH][keep], 1981, 1986)[1].sum() == days.size - 1
    with pytest.raises(ValueError, match="consecutive days"):
        _qalib.norm_groups(days[YEAR][keep], days[MONTH][keep], 1981, 1986, day=days[DAY][keep])
    assert np.array_equal(_qalib.norm_groups(days[YEAR], days[MONTH], 1981, 1986, day=days[DAY])[1], a[1])
    with pytest.raises(ValueError, match="gap-free"):
        _qalib.norm_groups(days[YEAR][::-1], days[MONTH][::-1], 1981, 1986)
    with pytest.raises(ValueError):
        _qalib.norm_groups(days[YEAR], days[MONTH], 1900, 1900 + _qalib.SC_MAX_GROUPS // 12)
    assert _qalib.run_threshold() == 1826 == USE_ALL_INFILL_THRESHOLD == _qalib.SC_RUN_THRESHOLD


def test_log_parser_and_suspects(gold, tmp_path):
    log = tmp_path / "infill.log"
    log.write_text(str(gold["log"]))
    got = get_bad_infill_stnids(str(log))
    assert got.tolist() == gold["log_ids"].tolist() == ["SNOTEL_13C01S", "USC00241044", "USC00245761", "USW00024033"]
    log.write_text("Status: 1 of 2\n")
    assert get_bad_infill_stnids(str(log)).size == 0
    days, ids, lon, lat, obs, reports = SC.e2e_pool()
    assert suspect_infill_stnids(reports["tmin"]).tolist() == ["S004", "S007"]
    assert suspect_infill_stnids(reports["tmax"]).tolist() == ["S002", "S004"]
    plain = {k: v for k, v in reports["tmax"].items() if k not in ("nonoptimal", "attempt", "reasons")}
    assert suspect_infill_stnids(plain).size == 0                    # without --chk-perf only the status speaks
    assert suspect_infill_stnids({k: v for k, v in reports["tmin"].items() if k != "reasons"}).tolist() == ["S007"]


def test_header_binding_and_build():
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxsc_\w+)\s*\(", h))) == sorted(_qalib.SC_EXPORTS) == \
        ["twxsc_serial_complete", "twxsc_series_check"]
    assert h.index("int twxxv_score(") < h.index("#define TWXSC_MAX_DAYS")
    for macro, val in (("TWXSC_MAX_DAYS", _qalib.SC_MAX_DAYS), ("TWXSC_MAX_GROUPS", _qalib.SC_MAX_GROUPS),
                       ("TWXSC_DEFAULT_RUN_THRESHOLD", _qalib.SC_RUN_THRESHOLD), ("TWXSC_DEFAULT_MAX_MISS", _qalib.SC_MAX_MISS),
                       ("TWXSC_NTIMES", len(_qalib.SC_KERNELS) + len(_qalib.SC_HOST_TIMES))):
        assert re.search(r"#define %s %d\b" % (macro, val), h), macro
    assert len(_qalib.SC_CHECK_TIMES) == len(_qalib.SC_KERNELS) + len(_qalib.SC_HOST_TIMES)
    assert _qalib.SC_MAX_DAYS >= 1 << 20 and _qalib.SC_MAX_GROUPS >= 12 * 64 and _qalib.SC_MAX_GROUPS % 12 == 0
    assert (RS.MAX_DAYS, RS.MAX_GROUPS, RS.RUN_THRESHOLD, RS.MAX_MISS) == (_qalib.SC_MAX_DAYS, _qalib.SC_MAX_GROUPS,
                                                                          _qalib.SC_RUN_THRESHOLD, _qalib.SC_MAX_MISS)
    assert np.float32(_qalib.SC_FILL_F4) == RS.FILL_F4 == ncio.FILL_F4
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_serial.hip" in build and os.path.exists(os.path.join(ROOT, "topowx_amd", "qa", "twx_serial.hip"))
    assert SERIAL_DB_VARIABLES["tmax"][0][:3] == ("tmax", "f4", float(ncio.FILL_F4)) and SERIAL_DB_VARIABLES["tmin"][1][:3] == ("flag_infilled", "i1", -127)
    import topowx_amd.infill as infill
    for name in ("write_infill_db", "get_bad_infill_stnids", "suspect_infill_stnids", "find_bad_infill_stns", "write_bad_stns_csv",
                 "create_serially_complete_db", "add_monthly_normals"):
        assert name in infill.__all__ and callable(getattr(infill, name)), name


def test_resource_table_lists_the_new_kernels():
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.SC_EXPORTS:
        assert hasattr(lib, name), name
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    assert table["k_sc_norms"]["lds"] == 8 * _qalib.SC_MAX_GROUPS and table["k_sc_select"]["lds"] == 4 * 4 * 4
    assert table["k_sc_series"]["lds"] == 4 * 4 * 8


def _stns(ids):
    from topowx_amd import stationdb as sdb
    stns = np.empty(len(ids), dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = ids, -110.0, 45.0, 100.0
    return stns


@pytest.mark.parametrize("fmt", ["NETCDF3_64BIT", None])
def test_write_infill_db(tmp_path, fmt):
    days, ids, lon, lat, obs, reports = SC.e2e_pool()
    rep = reports["tmin"]
    sub = dict(rep, **{k: rep[k][[6, 1, 7]] for k in ("ids", "fnl_tair", "mask_infill", "infill_tair", "mae", "bias")})
    path = str(tmp_path / "infill_tmin.nc")
    assert write_infill_db(path, _stns(ids), days, "tmin", sub, format=fmt) == path
    ds = ncio.open_dataset(path, "r")
    try:
        assert ncio._read_ids(ds.variables["station_id"]).tolist() == ["S001", "S006", "S007"]      # the table's order
        for name, dims in (("tmin", 2), ("tmin_infilled", 2), ("flag_infilled", 2), ("mae", 1), ("bias", 1)):
            assert len(ds.variables[name].dimensions) == dims, name
        t, m, f = (np.asarray(ds.variables[k][:]) for k in ("tmin", "tmin_infilled", "flag_infilled"))
        assert t.shape == (days.size, 3) and t.dtype == np.float32 and f.dtype == np.int8
        for col, row in enumerate((1, 6, 7)):
            want = rep["fnl_tair"][row].astype(np.float32)
            assert np.array_equal(t[:, col], np.where(np.isnan(want), ncio.FILL_F4, want))
            assert np.array_equal(f[:, col], rep["mask_infill"][row].astype(np.int8))
            assert np.asarray(ds.variables["mae"][:])[col] == rep["mae"][row]
        assert (t[:, 2] == ncio.FILL_F4).sum() == np.isnan(rep["fnl_tair"][7]).sum() > 0 and (m[:, 2] == ncio.FILL_F4).sum() == 240
        assert not np.isnan(t).any() and not np.isnan(m).any()
    finally:
        ds.close()
    with pytest.raises(FileExistsError):
        write_infill_db(path, _stns(ids), days, "tmin", sub)
    with pytest.raises(KeyError, match="not in the station table"):
        write_infill_db(str(tmp_path / "x.nc"), _stns(ids[:5]), days, "tmin", rep)
    with pytest.raises(ValueError):
        write_infill_db(str(tmp_path / "x.nc"), _stns(ids), days[:100], "tmin", rep)
    with pytest.raises(ValueError):
        write_infill_db(str(tmp_path / "x.nc"), _stns(ids), days, "prcp", rep)
    assert not os.path.exists(str(tmp_path / "x.nc"))
    csv = write_bad_stns_csv(str(tmp_path / "bad.csv"), ["S002", "S004"])
    assert open(csv).read() == "station_id,reason\nS002,infill issue\nS004,infill issue\n"


def test_entries_reject_bad_arguments_before_any_device_work():
    """Call-level failures (the library is needed, a GPU is not)."""
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    x = np.zeros((2, 40), np.float32)
    f = np.zeros((2, 40), np.int8)
    ok = (np.array([0] * 12, np.int32), np.array([0] * 12, np.int32))
    for kw, text in ((dict(fill=np.nan), "fill must be finite"), (dict(fill=np.inf), "fill must be finite"),
                     (dict(group_first=np.zeros(11, np.int32), group_ndays=np.zeros(11, np.int32)), "multiple of 12"),
                     (dict(group_first=np.zeros(1548, np.int32), group_ndays=np.zeros(1548, np.int32)), "multiple of 12"),
                     (dict(group_first=np.array([30] + [0] * 11, np.int32), group_ndays=np.array([11] + [0] * 11, np.int32)), "outside the day axis"),
                     (dict(group_first=np.array([-1] + [0] * 11, np.int32), group_ndays=np.array([3] + [0] * 11, np.int32)), "outside the day axis"),
                     (dict(group_first=np.array([0, 4] + [0] * 10, np.int32), group_ndays=np.array([5, 5] + [0] * 10, np.int32)), "ascending, disjoint"),
                     (dict(group_first=np.array([10, 0] + [0] * 10, np.int32), group_ndays=np.array([5, 5] + [0] * 10, np.int32)), "ascending, disjoint")):
        with pytest.raises(_qalib.QaError) as e:
            _qalib.serial_complete(x, x, f, **kw)
        assert text in str(e.value), str(e.value)
    with pytest.raises(_qalib.QaError, match="ndays <= 1048576"):
        _qalib.serial_complete(np.zeros((1, (1 << 20) + 1), np.float32))
    with pytest.raises(_qalib.QaError, match="nseries"):
        _qalib.serial_complete(np.zeros((0, 4), np.float32))
    for bad in (dict(tair_infilled=x), dict(flag=f), dict(group_first=ok[0]), dict(tair_infilled=x[:, :3], flag=f),
                dict(tair_infilled=x, flag=f[:1])):
        with pytest.raises(ValueError):
            _qalib.serial_complete(x, **bad)
    with pytest.raises(ValueError):
        _qalib.serial_complete(x[0])
    # the library itself refuses exactly one of tair_infilled / flag
    L = _qalib.load()
    buf = ctypes.create_string_buffer(512)
    out = np.zeros(64, np.int32)
    rc = L.twxsc_serial_complete(0, 2, 40, x.ctypes.data, x.ctypes.data, None, 5, 1e30, 0, None, None, 9, 0, None, None,
                                 out.ctypes.data, out.ctypes.data, out.ctypes.data, None, None, None, None, buf, 512)
    assert rc != 0 and b"together" in buf.value
    for kw in (dict(fill=np.nan), dict(impossible_high=np.inf), dict(impossible_low=np.nan)):
        with pytest.raises(_qalib.QaError, match="finite"):
            _qalib.series_check(x, pen=10.0, **kw)
    with pytest.raises(_qalib.QaError, match="ndays <= 1048576"):
        _qalib.series_check(np.zeros((1, (1 << 20) + 1), np.float32))
    with pytest.raises(_qalib.QaError, match="nseries"):
        _qalib.series_check(np.zeros((0, 10), np.float32))
    with pytest.raises(ValueError):
        _qalib.series_check(x[0])


def test_command_lines_fail_with_1(tmp_path, capsys):
    from topowx_amd import step17, step18
    days, ids, lon, lat, obs, reports = SC.e2e_pool()
    a, b = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    write_infill_db(a, _stns(ids), days, "tmin", reports["tmin"], format="NETCDF3_64BIT")
    write_infill_db(b, _stns(ids), days, "tmax", reports["tmax"], format="NETCDF3_64BIT")
    out = str(tmp_path / "bad.csv")
    base = ["--infill-tmin", a, "--infill-tmax", b, "--out", out]
    (tmp_path / "ids.txt").write_text("S002\nnobody\n")
    assert step17.main(base + ["--stnids", str(tmp_path / "ids.txt")]) == 1
    assert "neither infilled database" in capsys.readouterr().err and not os.path.exists(out)
    assert step17.main(base + ["--stnids", str(tmp_path / "nothing.txt")]) == 1
    assert "cannot open" in capsys.readouterr().err
    assert step17.main(["--infill-tmin", str(tmp_path / "none.nc"), "--infill-tmax", b, "--out", out, "--stnids", str(tmp_path / "ids.txt")]) == 1
    assert "cannot open" in capsys.readouterr().err
    (tmp_path / "junk.npz").write_bytes(b"not a zip")
    np.savez(str(tmp_path / "r.npz"), **reports["tmin"])
    assert step17.main(base + ["--db", a, "--report-tmin", str(tmp_path / "junk.npz"), "--report-tmax", str(tmp_path / "r.npz")]) == 1
    assert "cannot open" in capsys.readouterr().err
    # the databases exist already: --report-* does not overwrite them
    assert step17.main(base + ["--db", a, "--report-tmin", str(tmp_path / "r.npz"), "--report-tmax", str(tmp_path / "r.npz")]) == 1
    assert "not overwritten" in capsys.readouterr().err
    for bad in (base, base + ["--stnids", "x", "--log", "y"], base + ["--report-tmin", str(tmp_path / "r.npz")]):
        with pytest.raises(SystemExit) as e:
            step17.main(bad)
        assert e.value.code == 2
    capsys.readouterr()
    s18 = ["--infill-tmin", a, "--infill-tmax", b, "--serial-tmin", str(tmp_path / "c.nc"), "--serial-tmax", str(tmp_path / "d.nc")]
    assert step18.main(["--infill-tmin", str(tmp_path / "none.nc")] + s18[2:]) == 1
    assert "cannot open" in capsys.readouterr().err
    (tmp_path / "junk.nc").write_bytes(b"junk junk junk")
    assert step18.main(["--infill-tmin", str(tmp_path / "junk.nc")] + s18[2:]) == 1
    assert "cannot open" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "c.nc"))
