"""CPU: the rest of step08's spatial stage without a GPU -- the numpy restatement (tests/restate_corrob.py) against the
executed-reference golden (tests/golden/make_golden_corrob.py), the constants, the header against the binding, the
window table, ``StationObsPool.from_netcdf(qflags=True)``, the ``--write`` merge on both containers and the unchanged
default path of the step08 driver.

Flags are compared exactly and normals to 1e-7 degC: the tolerance / margin pair of the regression check's tests (the
golden maker asserted that every dif the reference looked at lies more than 1e-5 from the 10.0 cutoff)."""
import datetime as dt
import json
import os
import re
import sys

import numpy as np
import pytest

from topowx_amd.dates import YMD, get_days_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from spatial_cases import FORMATS, TOL  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_corrob_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_corrob as mk
    c = mk.case_inputs()
    assert mk.input_hash(*c[:6]) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return c


@pytest.fixture(scope="module")
def restated(case):
    import restate_corrob as RC
    ids, lon, lat, tmin, tmax, days, _ = case
    return RC.run(lon, lat, tmin, tmax, days[YMD])


def test_golden_content(gold, case):
    import make_golden_corrob as mk
    ids, lon, lat, tmin, tmax, days, spikes = case
    nd, n = days.size, ids.size
    assert (nd, n) == (3653, 30) and set(np.unique(days.YEAR[days.MONTH * 100 + days.DAY == 229])) == {1996, 2000, 2004}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_corrob_v1.npz")) < 1024 * 1024
    # the margins the maker asserted
    assert float(gold["cutoff_margin"]) > 1e-5 and (gold["margins"][:3] > 1e-5).all() and gold["margins"][3] > 1e-9
    assert float(gold["dist_gap"]) > 1e-9 and float(gold["radius_margin"]) > 1e-6
    f = (gold["flags_tmin"], gold["flags_tmax"])
    for k in (16, 17, 18):
        assert (f[0] == k).sum() + (f[1] == k).sum() > 0, k
    assert set(np.unique(f[0])) | set(np.unique(f[1])) == {1, 2, 16, 17, 18}
    # a stage only writes where the flag was 1
    for v, name in enumerate(("tmin", "tmax")):
        reg, cor = gold["reg_" + name], gold["cor_" + name]
        assert set(np.unique(reg)) <= {1, 2, 16} and set(np.unique(cor)) <= {1, 2, 16, 17}
        assert np.array_equal(reg[reg != 1], cor[reg != 1]) and np.array_equal(cor[cor != 1], f[v][cor != 1])
        assert np.array_equal(f[v] == 2, np.isnan((tmin, tmax)[v]))
    # the MAD == 0 branch and the empty list of anomalies occurred; the long-record target of the short-record cluster
    assert int(gold["mad0_rows"]) > 0 and int(gold["nempty"]) > 0
    rec = gold["rec_targets"].tolist()
    i = rec.index(mk.LONG_TARGET)
    empty = gold["rec_ndifs"][i] == 0
    assert empty.sum() > 100
    for v in range(2):
        assert (f[v][gold["rec_days"][empty[v]], mk.LONG_TARGET] == 17).all()
    # flag 18 on the station without neighbours; the sparse station's spike is the corroboration check's
    assert (f[0][:, mk.ALONE] == 18).sum() == 1 and (f[1][:, mk.ALONE] == 18).sum() == 1
    s, d, _ = spikes[-1]
    assert gold["reg_tmin"][d, s] == 1 and f[0][d, s] == 17
    # spikes on the second and second-to-last day of the series
    assert [tuple(x[:2]) for x in spikes[-3:-1]] == [(3, 1), (11, nd - 2)]


def test_restatement_flags_match_golden_at_every_stage(gold, restated):
    res = restated
    for v, name in enumerate(("tmin", "tmax")):
        assert np.array_equal(res["reg"][v], gold["reg_" + name] == 16), name
        assert np.array_equal(res["cor"][v], gold["cor_" + name] == 17), name
        assert np.array_equal(res["mega"][v], gold["flags_" + name] == 18), name
        assert np.array_equal(res["flags_" + name], gold["flags_" + name]), name
    tested = np.unpackbits(gold["tested"])[:res["tested"].size].reshape(res["tested"].shape).astype(bool)
    assert np.array_equal(res["tested"], tested)
    assert abs(res["cutoff_margin"] - float(gold["cutoff_margin"])) < TOL
    assert int(res["empty"].sum()) == int(gold["nempty"])
    assert not res["near"].any()


def test_restatement_normals_match_golden(gold, case, restated):
    import restate_corrob as RC
    ids, lon, lat, tmin, tmax, days, _ = case
    want, got = gold["tnorm"], restated["norms"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want).any() and np.isfinite(want).sum() > 30000
    print("max |normal - golden| %.3g degC" % np.nanmax(np.abs(got - want)))
    assert np.nanmax(np.abs(got - want)) < TOL
    mad0_seen = False
    for k, s in enumerate(gold["nnorm_stns"]):
        for v, obs in enumerate((tmin, tmax)):
            n, mad0 = RC.doy_norms(obs[:, s], days[YMD], with_mad0=True)
            mad0_seen |= bool(mad0.any())
            assert np.array_equal(np.isnan(n), np.isnan(gold["nnorm"][k, v]))
            if np.isfinite(n).any():
                assert np.nanmax(np.abs(n - gold["nnorm"][k, v])) < TOL
    assert mad0_seen                                              # station 7, constant for seven years
    assert np.isnan(gold["nnorm"][list(gold["nnorm_stns"]).index(26)]).all()      # five years of record: no normals


def test_recorded_anomalies(gold, case, restated):
    """anom_stn of the recorded days from the restated normals; the recorded difs decide the recorded flags."""
    import restate_corrob as RC
    ids, lon, lat, tmin, tmax, days, _ = case
    rows = RC.norm_rows(days[YMD])
    x = gold["rec_days"]
    for i, s in enumerate(gold["rec_targets"]):
        for v, obs in enumerate((tmin, tmax)):
            vals = obs[:, s].astype(np.float64)
            vals[restated["reg"][v][:, s]] = np.nan
            anom = np.abs(vals[x] - restated["norms"][s, v][rows[x]])
            was = gold["rec_ndifs"][i, v] >= 0
            assert np.array_equal(was, restated["tested"][v][x, s])
            assert np.abs(anom[was] - gold["rec_anom"][i, v][was]).max() < TOL
            d = gold["rec_difs"][i, v]
            flag = was & ~(d < 10.0).any(1)
            assert np.array_equal(flag, gold[("cor_tmin", "cor_tmax")[v]][x, s] == 17)


def test_window_table(gold):
    import restate_corrob as RC
    w365, w366 = RC.window_table(2003), RC.window_table(2004)
    assert w365.shape == (365, 15) and w366.shape == (366, 15)
    for w, name in ((w365, "win365"), (w366, "win366")):
        g = gold[name]
        for x in range(w.shape[0]):
            assert np.unique(w[x]).size == 15
            have = set(g[x][g[x] > 0].tolist())                   # the (month, day) values the reference's mask let through
            assert have == set(w[x].tolist())
    assert w365[0].tolist() == [1225, 1226, 1227, 1228, 1229, 1230, 1231, 101, 102, 103, 104, 105, 106, 107, 108]
    assert w365[364].tolist()[-8:] == [1231, 101, 102, 103, 104, 105, 106, 107]
    assert 229 not in w365
    assert [x for x in range(366) if 229 in w366[x]] == list(range(52, 67))          # Feb 22 .. Mar 7
    # rows of the two tables with the same centre date are the same window wherever Feb 29 is not in it
    for x in range(365):
        y = x if x < 59 else x + 1
        assert (set(w365[x]) == set(w366[y])) == (229 not in w366[y])


def test_constants_equal_the_reference(gold):
    from topowx_amd.qa import qa_temp
    import restate_corrob as RC
    for k in ("QA_OK", "QA_MISSING", "QA_SPATIAL_REGRESS", "QA_SPATIAL_CORROB", "QA_MEGA_INCONSIST", "ANOMALY_CUTOFF",
              "MIN_NORM_VALUES", "MIN_NGHS", "MAX_NGHS", "NGH_RADIUS"):
        assert float(getattr(qa_temp, k)) == float(gold["const_" + k]), k
    assert qa_temp.GHCN_TO_TWX_FLAGS_MAP == dict(zip(gold["ghcn_map_keys"].tolist(), gold["ghcn_map_vals"].tolist()))
    assert (RC.ANOMALY_CUTOFF, RC.MIN_NORM_VALUES, RC.MIN_NGHS, RC.MAX_NGHS) == tuple(
        float(gold["const_" + k]) for k in ("ANOMALY_CUTOFF", "MIN_NORM_VALUES", "MIN_NGHS", "MAX_NGHS"))
    # every character the write can produce maps back to a number with the same character
    for num, ch in qa_temp.TWX_TO_GHCN_FLAGS_MAP.items():
        assert qa_temp.TWX_TO_GHCN_FLAGS_MAP[qa_temp.GHCN_TO_TWX_FLAGS_MAP[ch]] == ch


def test_header_binding_and_constants():
    from topowx_amd import _qalib
    from topowx_amd.qa import qa_temp
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxqa_\w+)\s*\(", h))) == sorted(_qalib.EXPORTS)
    assert {"twxqa_spatial_only", "twxqa_doy_norms"} <= set(_qalib.EXPORTS)

    def define(name):
        m = re.search(r"#define %s (\S+)" % name, h)
        assert m, name
        return float(m.group(1))

    for name, val in (("TWXQA_ANOMALY_CUTOFF", qa_temp.ANOMALY_CUTOFF), ("TWXQA_MIN_NORM_VALUES", qa_temp.MIN_NORM_VALUES),
                      ("TWXQA_ANOMALY_CUTOFF", _qalib.ANOMALY_CUTOFF), ("TWXQA_MIN_NORM_VALUES", _qalib.MIN_NORM_VALUES),
                      ("TWXQA_NORM_ROWS", _qalib.NORM_ROWS), ("TWXQA_MAX_NORM_VALUES", _qalib.MAX_NORM_VALUES)):
        assert define(name) == float(val), name
    assert _qalib.NORM_ROWS == 365 + 366
    assert _qalib.MAX_NORM_VALUES >= 15 * 128                     # sized for at least 128 years
    assert _qalib.MAX_NORM_VALUES & (_qalib.MAX_NORM_VALUES - 1) == 0          # the sort pads to a power of two within it
    assert len(_qalib.SPATIAL_ONLY_KERNELS) == 6


def test_qa_library_lists_the_corroboration_kernels():
    """The new kernels are in libtwxqa.so's resource table, spill nothing, and the normals kernel's LDS is what the
    value cap was sized for (no build in this checkout: skipped, as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.EXPORTS:
        assert hasattr(lib, name), name
    table = isa_resources.parse(res)
    for k in ("k_doy_norms", "k_radius_dist", "k_corrob", "k_mega_final"):
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    lds = table["k_doy_norms"]["lds"]
    assert 4 * _qalib.MAX_NORM_VALUES + 2048 <= lds <= 4 * _qalib.MAX_NORM_VALUES + 2048 + 64
    assert 8 * lds <= 160 * 1024                                  # the 8 workgroups of 4 waves a CU can hold fit its LDS
    assert table["k_doy_norms"]["vgprs"] <= 64                    # registers do not cut the 8 waves per SIMD
    assert table["k_radius_dist"]["lds"] == 12 * _qalib.MAX_RADIUS_NGH


def test_series_longer_than_the_value_cap_fails_the_call():
    """A series that touches more years than TWXQA_MAX_NORM_VALUES / 15 is a call-level failure with a message, before
    any device work (the library is needed, a GPU is not)."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    years = _qalib.MAX_NORM_VALUES // 15 + 1
    days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    series = np.zeros((1, days.size), np.float32)
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_NORM_VALUES"):
        _qalib.doy_norms(series, days[YMD])
    with pytest.raises(_qalib.QaError, match="%d years" % years):
        _qalib.spatial_only(np.zeros(1), np.zeros(1), series, series, days[YMD], np.zeros(1, np.int32))
    ymd = np.array(days[YMD][:40])
    ymd[7] = ymd[6]
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        _qalib.doy_norms(series[:, :40], ymd)
    with pytest.raises(ValueError):
        _qalib.doy_norms(series[0], days[YMD])


# ---- the database side ------------------------------------------------------------------------------------------
def _small_pool(n=5, nd=40, seed=4):
    rs = np.random.RandomState(seed)
    days = get_days_metadata(dt.date(1990, 1, 1), dt.date(1990, 1, 1) + dt.timedelta(days=nd - 1))
    tmin = np.round(rs.randn(nd, n) * 5, 1).astype(np.float32)
    tmax = (tmin + 10).astype(np.float32)
    tmin[rs.rand(nd, n) < 0.1] = np.nan
    ids = np.array(["GHCN_%03d" % i for i in range(n)])
    return ids, -110 + rs.rand(n), 45 + rs.rand(n), tmin, tmax, days


PREV = (("qflag_tmin", 3, 1, b"D"), ("qflag_tmin", 4, 1, b"X"), ("qflag_tmax", 3, 1, b"K"), ("qflag_tmax", 9, 2, b"G"),
        ("qflag_tmin", 12, 4, b"I"))


@pytest.mark.parametrize("fmt", FORMATS)
def test_from_netcdf_masks_flagged_observations(tmp_path, fmt):
    import corrob_cases
    from topowx_amd.qa import StationObsPool
    ids, lon, lat, tmin, tmax, days = _small_pool()
    tmin[[3, 4, 12], [1, 1, 4]] = [1.5, 2.5, 3.5]                 # the flagged entries hold values
    path = corrob_cases.write_db(str(tmp_path / ("all_%s.nc" % fmt)), ids, lon, lat, tmin, tmax, days, fmt, prev=PREV)
    plain = StationObsPool.from_netcdf(path)                      # the default: flags not read, nothing masked
    assert plain.qflag_tmin is None and plain.qflag_tmax is None
    np.testing.assert_array_equal(plain.tmin, tmin)
    np.testing.assert_array_equal(plain.tmax, tmax)
    pool = StationObsPool.from_netcdf(path, qflags=True)
    assert pool.qflag_tmin.dtype == np.dtype("S1") and pool.qflag_tmin.shape == tmin.shape
    want0, want1 = tmin.copy(), tmax.copy()
    for name, d, s, ch in PREV:
        q = pool.qflag_tmin if name == "qflag_tmin" else pool.qflag_tmax
        assert q[d, s] == ch
        (want0 if name == "qflag_tmin" else want1)[d, s] = np.nan
    assert (pool.qflag_tmin != b"").sum() == 3 and (pool.qflag_tmax != b"").sum() == 2
    np.testing.assert_array_equal(pool.tmin, want0)
    np.testing.assert_array_equal(pool.tmax, want1)
    bare = corrob_cases.write_db(str(tmp_path / ("bare_%s.nc" % fmt)), ids, lon, lat, tmin, tmax, days, fmt, qflags=False)
    with pytest.raises(KeyError, match="qflag_tmin"):
        StationObsPool.from_netcdf(bare, qflags=True)


def test_merge_qflags_semantics():
    from topowx_amd import step08
    f0 = np.array([1, 2, 16, 17, 18, 1, 2, 1], np.uint8)
    f1 = np.array([1, 1, 1, 2, 2, 17, 16, 1], np.uint8)
    p0 = np.array([b"D", b"", b"X", b"", b"", b"K", b"G", b"T"], "S1")
    p1 = np.array([b"", b"", b"I", b"R", b"", b"", b"D", b""], "S1")
    rows, c0, c1 = step08.merge_qflags(f0, f1, p0, p1)
    assert rows.tolist() == [False, False, True, True, True, True, True, False]
    # new flag's character; a previous character kept where the new flag is 1 / 2; both variables on every row
    assert c0[rows].tolist() == [b"S", b"S", b"M", b"K", b"G"]
    assert c1[rows].tolist() == [b"I", b"R", b"", b"S", b"S"]
    with pytest.raises(ValueError):
        step08.merge_qflags(np.array([99]), np.array([1]), np.array([b""]), np.array([b""]))
    with pytest.raises(ValueError):
        step08.merge_qflags(f0, f1[:-1], p0, p1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_write_qflags_on_a_database(tmp_path, fmt):
    import corrob_cases
    from topowx_amd import step08
    from topowx_amd.qa import StationObsPool
    ids, lon, lat, tmin, tmax, days = _small_pool()
    path = corrob_cases.write_db(str(tmp_path / ("all_%s.nc" % fmt)), ids, lon, lat, tmin, tmax, days, fmt, prev=PREV)
    nd = days.size
    cols = [4, 1, 2]                                              # targets in non-table order
    f0, f1 = np.ones((nd, 3), np.uint8), np.ones((nd, 3), np.uint8)
    f0[12, 0] = 2                   # station 4, day 12: previous 'I' in tmin, new corroboration flag in tmax
    f1[12, 0] = 17
    f0[3, 1], f1[3, 1] = 16, 2      # station 1, day 3: previous 'D' / 'K'; tmin re-flagged, tmax keeps 'K'
    f0[20, 1] = 18                  # station 1, day 20: nothing before
    f1[9, 2] = 2                    # station 2, day 9: previous 'G' in tmax, no new flag: not a row
    assert step08.write_qflags(path, cols, f0, f1) == 3
    back = StationObsPool.from_netcdf(path, qflags=True)
    want0, want1 = np.zeros((nd, ids.size), "S1"), np.zeros((nd, ids.size), "S1")
    for name, d, s, ch in PREV:
        (want0 if name == "qflag_tmin" else want1)[d, s] = ch
    want1[12, 4] = b"S"
    want0[3, 1] = b"S"
    want0[20, 1] = b"M"
    np.testing.assert_array_equal(back.qflag_tmin, want0)
    np.testing.assert_array_equal(back.qflag_tmax, want1)
    # the numeric variables are untouched
    np.testing.assert_array_equal(StationObsPool.from_netcdf(path).tmin, tmin)
    bare = corrob_cases.write_db(str(tmp_path / ("bare_%s.nc" % fmt)), ids, lon, lat, tmin, tmax, days, fmt, qflags=False)
    with pytest.raises(KeyError):
        step08.write_qflags(bare, cols, f0, f1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_step08_write_without_qflag_variables_exits_1(tmp_path, capsys, fmt):
    import corrob_cases
    from topowx_amd import step08
    ids, lon, lat, tmin, tmax, days = _small_pool()
    bare = corrob_cases.write_db(str(tmp_path / ("bare_%s.nc" % fmt)), ids, lon, lat, tmin, tmax, days, fmt, qflags=False)
    out = str(tmp_path / "r.npz")
    assert step08.main(["--db", bare, "--out", out, "--spatial", "--write"]) == 1
    assert "qflag" in capsys.readouterr().err and not os.path.exists(out)
    with pytest.raises(SystemExit):                               # --write is only valid with --spatial
        step08.main(["--db", bare, "--out", out, "--write"])


def test_step08_default_path_is_unchanged(tmp_path, capsys, monkeypatch):
    """Without --spatial the driver calls the regression check alone on the unmasked pool -- flags in the database are
    not read -- and prints / writes what it did before (the device call is replaced by a stand-in here; the GPU suite
    runs the real one)."""
    import corrob_cases
    from topowx_amd import step08
    ids, lon, lat, tmin, tmax, days = _small_pool()
    path = corrob_cases.write_db(str(tmp_path / "all.nc"), ids, lon, lat, tmin, tmax, days, "NETCDF3_64BIT", prev=PREV)
    seen = {}

    def fake(pool, targets, device=0, details=False, timing=None):
        seen["tmin"], seen["targets"], seen["qflag"] = pool.tmin.copy(), targets, pool.qflag_tmin
        timing.update(radius_kernel_ms=1.0, regress_kernel_ms=2.0)
        f = np.where(np.isnan(pool.tmin), 2, 1).astype(np.uint8)
        f[5, 0] = 16
        return f, np.ones_like(f), {"status": np.zeros((pool.ids.size, 2, 1), np.int32)}

    def never(*a, **k):
        raise AssertionError("the default path must not run the whole stage")

    monkeypatch.setattr(step08, "qa_spatial_regress", fake)
    monkeypatch.setattr(step08, "run_qa_spatial_only", never)
    out = str(tmp_path / "report.npz")
    assert step08.main(["--db", path, "--out", out]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(line) == ["stations", "pool", "items", "flags_tmin", "flags_tmax", "seconds", "radius_kernel_ms",
                          "regress_kernel_ms"]
    assert (line["stations"], line["pool"], line["items"], line["flags_tmin"], line["flags_tmax"]) == (5, 5, 10, 1, 0)
    np.testing.assert_array_equal(seen["tmin"], tmin)             # flagged observations are NOT masked here
    assert seen["targets"] is None and seen["qflag"] is None
    rep = np.load(out)
    assert sorted(rep.files) == ["flags_tmax", "flags_tmin", "ids", "status", "ymd"]
    assert rep["flags_tmin"][5, 0] == 16
