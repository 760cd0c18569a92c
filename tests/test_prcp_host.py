"""CPU: the non-spatial precipitation QA without a GPU -- the numpy restatement (tests/restate_prcp.py) against the
executed-reference golden (tests/golden/make_golden_prcp.py) at every stage of both chains, the header against the binding
and the build script, the resource table of the new kernels, the argument checks, the import surface, and the command line
end to end on both containers with a stand-in for the library call.

Flags are compared exactly and tables to 1e-12 relative: the golden maker asserted that every comparison of checks 15 and
19 the reference made lies more than 1e-5 relative from equality or is a tie that no precision can decide otherwise."""
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

import prcp_cases as PC  # noqa: E402
import restate_prcp as RP  # noqa: E402
from spatial_cases import FORMATS  # noqa: E402

NEW_KERNELS = ("k_pq_init", "k_pq_dups", "k_pq_streak", "k_pq_compact", "k_pq_frequent", "k_pq_apply", "k_pq_gap",
               "k_pq_pctiles", "k_pq_clim")
TABLE_TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_prcp_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    prcp, tavg, days, plants = PC.case_inputs()
    assert PC.input_hash(prcp, tavg, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return prcp, tavg, days, plants


def _rel(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] / want[fin] - 1.0))) if fin.any() else 0.0


def test_golden_content(gold, case):
    prcp, tavg, days, plants = case
    assert prcp.shape == (5844, 16) and prcp.dtype == np.float32 and tavg.dtype == np.float32
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_prcp_v1.npz")) < 1024 * 1024
    wet = np.isfinite(prcp) & (prcp > 0)
    plain = [PC.S_PLAIN7, PC.S_PLAIN12, PC.S_PLAIN14, PC.S_PLAIN15]
    assert 0.25 < wet[:, plain].mean() < 0.33 and 0.02 < np.isnan(prcp[:, plain]).mean() < 0.04
    assert gold["stages"].tolist() == list(RP.STAGE_ORDER)
    assert float(gold["margin"]) > 1e-5 and float(gold["ref_station_years_per_second"]) > 0
    f, fa = gold["flags_default"], gold["flags_all"]
    assert np.array_equal(f == 2, np.isnan(prcp)) and not np.isin(f, (9, 19)).any()
    for k in (1, 2, 4, 5, 6, 8, 10, 15):
        assert (f == k).any(), k
    for k in (1, 2, 4, 5, 6, 8, 9, 10, 15, 19):
        assert (fa == k).any(), k
    for k, want in plants.items():
        assert np.array_equal(gold["plant_" + k], np.asarray(want)), k
    # the stored stages are nested: a check writes only where the flag is still 1
    for key, final in (("stage_flags_default", f), ("stage_flags_all", fa)):
        st = gold[key]
        assert np.array_equal(st[-1], final)
        for i, num in enumerate(RP.STAGE_ORDER):
            assert np.array_equal(st[i], RP.stage_flags(final, num)), (key, num)
    # the kept quirks
    assert not np.isin(f[plants["dupmonths_quirk"], PC.S_DUPMONTHS], (4, 5, 6)).any()
    assert not (fa[plants["streak_end"], PC.S_STREAK] == 9).any()
    assert f[plants["shift_day"], PC.S_SPARSE] == 15
    assert f[plants["imposs_edge"], PC.S_IMPOSS] != 8 and f[plants["imposs_next"], PC.S_IMPOSS] == 8
    assert f[plants["gap30"], PC.S_GAP] == 10 and f[plants["gap_below"], PC.S_GAP] != 10


@pytest.mark.parametrize("both", [False, True], ids=["default", "streak_frequent"])
def test_restatement_equals_the_golden_at_every_stage(gold, case, both):
    res = PC.restated("main", both, both)
    st = gold["stage_flags_all" if both else "stage_flags_default"]
    for i, num in enumerate(RP.STAGE_ORDER):
        bad = np.argwhere(res["stages"][num] != st[i])
        assert bad.size == 0, (num, bad[:10].tolist())
    assert np.array_equal(res["flags"], gold["flags_all" if both else "flags_default"])
    assert not res["knife"].any()
    stns = gold["pct_stns"]
    d = _rel(res["pctiles"][stns], gold["pctiles_all" if both else "pctiles_default"])
    print("tables of check 15: max relative difference %.3g" % d)
    assert d <= TABLE_TOL
    if both:
        assert _rel(res["pctiles_frequent"][stns], gold["pctiles_all_frequent"]) <= TABLE_TOL
    else:
        n = res["pctiles"].shape[0]
        nan = np.unpackbits(gold["pctiles_nan"])[:n * 366].reshape(n, 366).astype(bool)
        assert np.array_equal(np.isnan(res["pctiles"][..., 0]), nan)
        assert np.isnan(res["pctiles"][PC.S_DRY]).all() and np.isfinite(res["pctiles"][PC.S_PLAIN12]).all()


def test_restatement_equals_the_short_record(gold):
    p, tv, days = PC.short_inputs()
    assert PC.input_hash(p, tv, days) == str(gold["short_hash"]) and np.unique(days.MONTH).size == 7
    for both, key in ((False, "short_stage_flags_default"), (True, "short_stage_flags_all")):
        res = PC.restated("short", both, both)
        for i, num in enumerate(RP.STAGE_ORDER):
            assert np.array_equal(res["stages"][num], gold[key][i]), (key, num)
    f = gold["short_stage_flags_default"][-1]
    assert not (f[:, 0] == 6).any() and (f[:, 1] == 6).sum() == 62 and (f[:, 2] == 6).sum() == 61


def test_random_pool_has_at_most_one_knife_edge_station():
    """The GPU test leaves a station out when the restatement sees a comparison within 1e-6 relative of equality."""
    for both in (False, True):
        want = PC.restated("random", both, both)
        assert want["knife"].shape == (PC.RANDOM_NSTN,) and want["knife"].sum() <= PC.RANDOM_MAX_KNIFE
    f = want["flags"]
    assert set(np.unique(f).tolist()) == {1, 2, 4, 5, 6, 8, 9, 10, 15, 19}
    assert np.isfinite(want["pctiles"][..., 4]).mean() > 0.5


def test_header_binding_and_build_script_agree():
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxpq_\w+)\s*\(", h))) == sorted(_qalib.PQ_EXPORTS)
    assert not any(name in _qalib.EXPORTS for name in _qalib.PQ_EXPORTS)
    for macro, val in (("TWXPQ_MAX_WINDOW_VALUES", _qalib.PQ_MAX_WINDOW_VALUES), ("TWXPQ_PCTILE_ROWS", _qalib.PQ_PCTILE_ROWS),
                       ("TWXPQ_PCTILE_COLS", _qalib.PQ_PCTILE_COLS), ("TWXPQ_NKERNELS", len(_qalib.PQ_KERNELS)),
                       ("TWXPQ_MIN_PERCENTILE_VALUES", _qalib.PQ_MIN_PERCENTILE_VALUES)):
        m = re.search(r"#define %s (\d+)" % macro, h)
        assert m and int(m.group(1)) == val, macro
    assert _qalib.PQ_MAX_WINDOW_VALUES // 29 == 141 and _qalib.PQ_MAX_WINDOW_VALUES & (_qalib.PQ_MAX_WINDOW_VALUES - 1) == 0
    b = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_prcpqa.hip" in b and os.path.exists(os.path.join(ROOT, "topowx_amd", "qa", "twx_prcpqa.hip"))
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_prcpqa.hip")).read()
    assert sorted(set(re.findall(r'extern "C" int (twxpq_\w+)\(', src))) == sorted(_qalib.PQ_EXPORTS)
    assert sorted(set(re.findall(r"\b(k_pq_\w+)\(", src))) == sorted(NEW_KERNELS)
    assert "atomicAdd(float" not in src and "atomicAdd(double" not in src


def test_import_surface_and_constants(gold):
    from topowx_amd import qa
    from topowx_amd.qa import qa_prcp, qa_temp
    for name in ("qa_prcp", "run_qa_non_spatial_prcp", "build_percentiles", "load_prcp_pool", "QA_FREQUENT", "QA_YR_CLIM_OUTLIER",
                 "PRCP_MAX_VALUE", "GAP_THRES", "MIN_PERCENTILE_VALUES", "PRCP_TWX_TO_GHCN_FLAGS_MAP"):
        assert name in qa.__all__ and hasattr(qa, name), name
    assert qa.run_qa_non_spatial is qa_temp.run_qa_non_spatial and qa.run_qa_non_spatial_prcp is qa_prcp.run_qa_non_spatial
    for name in qa_prcp.__all__:
        assert hasattr(qa_prcp, name), name
    for k in ("QA_OK", "QA_MISSING", "QA_DUP_YEAR", "QA_DUP_MONTH", "QA_DUP_YEAR_MONTH", "QA_IMPOSS_VALUE", "QA_STREAK", "QA_GAP",
              "QA_CLIM_OUTLIER", "QA_FREQUENT", "QA_YR_CLIM_OUTLIER", "PRCP_MIN_VALUE", "PRCP_MAX_VALUE", "STREAK_LEN",
              "GAP_THRES", "MIN_PERCENTILE_VALUES", "MAX_SPATIAL_COLLAB_THRES"):
        assert float(getattr(qa_prcp, k)) == float(gold["const_" + k]), k
    assert qa_prcp.PRCP_NON_SPATIAL_FLAGS == tuple(RP.STAGE_ORDER) == tuple(gold["stages"].tolist())
    t = qa_prcp.PRCP_TWX_TO_GHCN_FLAGS_MAP
    assert all(t[k] == v for k, v in qa_temp.TWX_TO_GHCN_FLAGS_MAP.items()) and t[19] == "K" and 20 in t
    assert qa_prcp.PRCP_GHCN_TO_TWX_FLAGS_MAP == qa_temp.GHCN_TO_TWX_FLAGS_MAP


def test_resource_table_lists_the_new_kernels():
    """No scratch, no spills, and the LDS the cap was sized for (no build in this checkout: skipped, as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    assert all(hasattr(lib, name) for name in _qalib.PQ_EXPORTS)
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    lds = table["k_pq_pctiles"]["lds"]
    assert 4 * _qalib.PQ_MAX_WINDOW_VALUES <= lds <= 4 * _qalib.PQ_MAX_WINDOW_VALUES + 64
    assert 8 * lds <= 160 * 1024 and table["k_pq_pctiles"]["vgprs"] <= 64       # 8 workgroups of 4 waves per compute unit
    lds = table["k_pq_gap"]["lds"]
    assert 4 * _qalib.MAX_GAP_VALUES <= lds <= 4 * _qalib.MAX_GAP_VALUES + 64 and table["k_pq_gap"]["vgprs"] <= 64
    assert 8 * table["k_pq_dups"]["lds"] <= 160 * 1024


def test_argument_checks_come_before_any_device_work():
    from topowx_amd import _qalib
    from topowx_amd.qa import qa_prcp
    days = get_days_metadata(dt.date(2000, 1, 1), dt.date(2000, 3, 1))
    x = np.zeros((days.size, 3), np.float32)
    for bad in ((x[:-1], x), (x, x[:, :2]), (x[None], x[None])):
        with pytest.raises(ValueError):
            qa_prcp.run_qa_non_spatial(bad[0], bad[1], days)
    with pytest.raises(ValueError):
        qa_prcp.build_percentiles(x[:-1], days)
    with pytest.raises(ValueError):
        _qalib.prcp_non_spatial(x.T[0], x.T[0], days[YMD])
    with pytest.raises(ValueError):
        _qalib.prcp_non_spatial(x.T, x.T[:2], days[YMD])
    with pytest.raises(ValueError):
        _qalib.prcp_percentiles(x, days[YMD])                       # [ndays, n] where [n, ndays] is wanted
    if not os.path.exists(_qalib.LIB_PATH):
        return
    # call-level failures of the library: the message names the macro; nothing touches a device (none is needed here)
    years = _qalib.PQ_MAX_WINDOW_VALUES // 29 + 1
    long_days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    series = np.zeros((1, long_days.size), np.float32)
    with pytest.raises(_qalib.QaError, match="TWXPQ_MAX_WINDOW_VALUES"):
        _qalib.prcp_non_spatial(series, series, long_days[YMD])
    with pytest.raises(_qalib.QaError, match="%d years" % years):
        _qalib.prcp_percentiles(series, long_days[YMD])
    gap_years = _qalib.MAX_GAP_VALUES // 31 + 1                     # inside the window cap, over the gap check's
    keep = long_days.YEAR < 1800 + gap_years
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_GAP_VALUES"):
        _qalib.prcp_non_spatial(series[:, keep], series[:, keep], long_days[YMD][keep])
    ymd = np.array(days[YMD])
    ymd[7] = ymd[6]
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        _qalib.prcp_non_spatial(x.T, x.T, ymd)


def test_merge_keeps_previous_flags_and_maps_every_number():
    from topowx_amd.qa import qa_prcp
    flags = np.array([1, 2, 4, 5, 6, 8, 9, 10, 15, 19, 1, 2], np.uint8)
    prev = np.array([b"", b"", b"", b"X", b"", b"", b"", b"", b"", b"", b"S", b"G"], "S1")
    rows, chars = qa_prcp.merge_qflags(flags, prev)
    assert rows.tolist() == [False, False] + [True] * 8 + [False, False]
    assert chars.tolist() == [b"", b"", b"D", b"D", b"D", b"X", b"K", b"G", b"O", b"K", b"S", b"G"]
    with pytest.raises(ValueError):
        qa_prcp.merge_qflags(np.array([21]), np.array([b""], "S1"))


@pytest.mark.parametrize("fmt", FORMATS)
def test_command_line_with_a_stand_in_for_the_library(tmp_path, capsys, monkeypatch, fmt):
    from topowx_amd.qa import qa_prcp
    rs = np.random.RandomState(4)
    days = get_days_metadata(dt.date(1990, 1, 1), dt.date(1990, 2, 9))
    n, nd = 5, days.size
    prcp = np.round(rs.rand(nd, n), 2).astype(np.float32)
    prcp[2, 1] = np.nan
    tmin = np.round(rs.randn(nd, n) * 5, 1).astype(np.float32)
    tmax = (tmin + 10).astype(np.float32)
    tmax[4, 1] = np.nan
    ids = np.array(["GHCN_%03d" % i for i in range(n)])
    lon, lat = -110 + rs.rand(n), 45 + rs.rand(n)
    db = PC.write_db(str(tmp_path / "all.nc"), ids, lon, lat, prcp, tmin, tmax, days, fmt,
                     qflags=("qflag_tmin", "qflag_tmax", "qflag_prcp"),
                     prev=(("qflag_tmin", 3, 1, b"D"), ("qflag_prcp", 7, 1, b"S"), ("qflag_prcp", 5, 4, b"O")))
    bare = PC.write_db(str(tmp_path / "bare.nc"), ids, lon, lat, prcp, tmin, tmax, days, fmt, qflags=())
    pool = qa_prcp.load_prcp_pool(db, qflags=True)
    assert np.array_equal(pool.prcp, prcp, equal_nan=True) and pool.qflag_prcp[7, 1] == b"S"
    assert np.isnan(pool.tavg[3, 1]) and np.isnan(pool.tavg[4, 1]) and pool.tavg[5, 1] == (tmin[5, 1] + tmax[5, 1]) / np.float32(2)
    assert np.isfinite(qa_prcp.load_prcp_pool(db).tavg[3, 1]) and qa_prcp.load_prcp_pool(bare).qflag_prcp is None
    with pytest.raises(KeyError):
        qa_prcp.load_prcp_pool(bare, qflags=True)
    seen = {}

    def fake(p, tv, days_, device=0, streak=False, frequent=False, details=False, timing=None):
        seen.update(shape=p.shape, streak=streak, frequent=frequent, tavg=tv.copy())
        timing.update(pq_gap_kernel_ms=1.0)
        f = np.where(np.isnan(p), 2, 1).astype(np.uint8)
        f[5, 0], f[6, 0] = 10, 19
        return f

    monkeypatch.setattr(qa_prcp, "run_qa_non_spatial", fake)
    out = str(tmp_path / "r.npz")
    with pytest.raises(SystemExit):
        qa_prcp.main(["--out", out])
    capsys.readouterr()
    assert qa_prcp.main(["--db", str(tmp_path / "nothing.nc"), "--out", out]) == 1
    assert "cannot open" in capsys.readouterr().err
    before = open(db, "rb").read()
    assert qa_prcp.main(["--db", db, "--out", out, "--streak"]) == 0                      # a report: the database is left alone
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert open(db, "rb").read() == before and "rows_written" not in line
    assert seen["shape"] == (nd, n) and seen["streak"] and not seen["frequent"] and np.isnan(seen["tavg"][3, 1])
    assert line["stations"] == n and line["flags_prcp"]["10"] == 1 and line["flags_prcp"]["19"] == 1 and line["flags_prcp"]["2"] == 1
    assert sorted(line["flags_prcp"]) == sorted(str(k) for k in (1, 2, 4, 5, 6, 8, 9, 10, 15, 19))
    assert sorted(np.load(out).files) == ["flags_prcp", "ids", "ymd"]
    tfile = tmp_path / "t.txt"
    tfile.write_text("GHCN_001\nGHCN_004\n")
    assert qa_prcp.main(["--db", db, "--out", out, "--frequent", "--write", "--targets", str(tfile)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["shape"] == (nd, 2) and seen["frequent"] and line["rows_written"] == 2
    back = qa_prcp.load_prcp_pool(db)
    assert back.qflag_prcp[5, 1] == b"G" and back.qflag_prcp[6, 1] == b"K"            # written on the target's column
    assert back.qflag_prcp[7, 1] == b"S" and back.qflag_prcp[5, 4] == b"O"            # flags already there are kept
    assert (back.qflag_prcp != b"").sum() == 4 and np.array_equal(back.prcp, prcp, equal_nan=True)
    bad = tmp_path / "bad.txt"
    bad.write_text("NOPE\n")
    assert qa_prcp.main(["--db", db, "--out", out, "--targets", str(bad)]) == 1
    capsys.readouterr()
    # a database without qflag_prcp: --write creates it
    assert qa_prcp.main(["--db", bare, "--out", out, "--write"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["rows_written"] == 2
    made = qa_prcp.load_prcp_pool(bare)
    assert made.qflag_prcp.shape == (nd, n) and made.qflag_prcp[5, 0] == b"G" and (made.qflag_prcp != b"").sum() == 2
    assert np.array_equal(made.prcp, prcp, equal_nan=True) and np.array_equal(made.tmin, tmin, equal_nan=True)
