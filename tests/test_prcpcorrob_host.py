"""CPU: the precipitation QA's spatial corroboration check (flag 17) without a GPU -- the numpy restatement
(tests/restate_prcpcorrob.py) against the executed-reference golden (tests/golden/make_golden_prcpcorrob.py) in every flag
of both chains, the row counts and the per-day figures; the header against the binding and the build script; the resource
table of the new kernels; the argument checks; the random pool's margins; and the command line with a stand-in for the
library calls (the default invocation's report keys are unchanged).

Flags and counts are compared exactly, ``abs_dif`` / ``pctile`` / ``thres`` to 1e-12 relative: the golden maker asserted
that every ``abs_dif`` lies more than 1e-5 relative from its ``thres`` and that no two neighbours of a target are
equidistant."""
import ctypes
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
import prcpcorrob_cases as CC  # noqa: E402
import restate_prcp as RP  # noqa: E402
import restate_prcpcorrob as RC  # noqa: E402
from spatial_cases import FORMATS  # noqa: E402

NEW_KERNELS = ("k_pc_radius", "k_pc_rowcounts", "k_pc_walk", "k_pc_rank", "k_pc_apply")
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_prcpcorrob_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    ids, lon, lat, prcp, tavg, days, plants = CC.case_inputs()
    assert CC.input_hash(lon, lat, prcp, tavg, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return ids, lon, lat, prcp, tavg, days, plants


def dense(gold, chain, shape):
    """The golden's per-day figures as [ndays, n] arrays, NaN where the day did not get past the range test."""
    out = {k: np.full(shape, np.nan) for k in ("abs_dif", "pctile", "thres")}
    key = gold["reached_" + chain]
    for k in out:
        out[k][key[:, 1], key[:, 0]] = gold[k + "_" + chain]
    return out


def rel(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want) & (want != 0)
    assert np.array_equal(got[np.isfinite(want) & (want == 0)], want[np.isfinite(want) & (want == 0)])
    return float(np.max(np.abs(got[fin] / want[fin] - 1.0))) if fin.any() else 0.0


def test_golden_content(gold, case):
    ids, lon, lat, prcp, tavg, days, P = case
    assert prcp.shape == (2192, 28) and prcp.dtype == np.float32
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_prcpcorrob_v1.npz")) < 1024 * 1024
    assert float(gold["margin"]) > 1e-5 and float(gold["f32_abs_dif_rel"]) <= 6e-8 and float(gold["dist_gap"]) > 1e-9
    assert float(gold["ref_station_years_per_second"]) > 0
    fs, fa, fc = gold["flags_spatial"], gold["flags_all"], gold["flags_chain"]
    assert set(np.unique(fs).tolist()) == {1, 2, 17} and np.array_equal(fs == 2, np.isnan(prcp))
    assert (fa == 17).sum() > 0 and np.array_equal(fa[fa != 17], fc[fa != 17]) and (fc[fa == 17] == 1).all()
    assert gold["nngh"].tolist() == [8] * 9 + [7] * 8 + [3] * 8 + [2] * 3
    s, d = P["chain15"]
    assert fa[d, s] == 15 and fs[d, s] == 17
    s, d = P["dry_wet"]
    th = dense(gold, "spatial", fs.shape)
    assert fs[d, s] == 1 and th["thres"][d, s] > th["abs_dif"][d, s] > 26.924 and th["pctile"][d, s] == 0.0
    assert float(gold["const_MAX_SPATIAL_COLLAB_THRES"]) == RC.THRES and float(gold["const_MAX_SPATIAL_COLLAB_THRES_MM"]) == RC.THRES_MM
    assert (gold["const_MIN_NGHS"], gold["const_MAX_NGHS"], gold["const_MIN_PERCENTILE_VALUES"], gold["const_NGH_RADIUS"]) == (3, 7, 20, 75)


@pytest.mark.parametrize("chain", ["spatial", "all"])
def test_restatement_equals_the_executed_reference(gold, case, chain):
    ids, lon, lat, prcp, tavg, days, P = case
    res = CC.restated("main", chain)
    if chain == "all":                                              # the restated non-spatial chain is the reference's
        assert np.array_equal(res["flags_in"], gold["flags_chain"])
    want = gold["flags_" + chain]
    bad = np.argwhere(res["flags"] != want)
    assert bad.size == 0, bad[:10].tolist()
    assert np.array_equal(res["nngh"], gold["nngh"])
    assert np.array_equal(res["status"], np.where(gold["nngh"] < 3, RC.SP_FEW_NGHS, RC.SP_OK))
    d = dense(gold, chain, want.shape)
    for k in ("abs_dif", "pctile", "thres"):
        assert rel(res[k], d[k]) <= TOL, k
    assert np.isfinite(d["abs_dif"]).sum() == gold["reached_" + chain].shape[0] > 3000


def test_restated_row_counts_equal_the_executed_reference(gold, case):
    ids, lon, lat, prcp, tavg, days, P = case
    assert np.array_equal(RC.pors_counts(prcp, days[YMD]), gold["counts_pool"])
    left = np.where(gold["flags_chain"] == 1, prcp, np.float32(np.nan))
    assert np.array_equal(RC.pors_counts(left, days[YMD]), gold["counts_all"])
    assert RC.pors_counts(prcp[:, 3], days[YMD]).shape == (366,)
    c = gold["counts_pool"][:, CC.S_SPARSE]
    assert {20, 21} <= set(c.tolist())
    row, _ = RC.calendar(days[YMD])
    assert np.array_equal(row, np.asarray(days.YDAY, np.int64) - 1)


def test_random_pool_is_nowhere_within_the_margin():
    """The GPU test may leave out days whose restatement margin is under 1e-5; the seed is chosen so that there are none."""
    ids, lon, lat, p, tv, days = CC.random_inputs()
    assert p.shape == (1461, 40) and days[YMD][0] == 20010307
    for chain in ("spatial", "all"):
        res = CC.restated("random", chain)
        assert res["margin"].min() > CC.RANDOM_MARGIN, (chain, res["margin"].min())
        assert (res["flags"] == 17).sum() >= 20 and np.isfinite(res["pctile"]).sum() > 500
        assert ((res["thres"] < RC.THRES) & (res["flags"] == 17)).sum() > 0 and (res["thres"] == RC.THRES).sum() > 0
        assert res["status"][-1] == RC.SP_FEW_NGHS and 8 < res["nngh"][:-1].min() and res["nngh"].max() < 40
    assert (CC.restated("random", "all")["flags_in"] == 15).sum() > 0


def test_header_binding_and_build_script_agree():
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxpc_\w+)\s*\(", h))) == sorted(_qalib.PC_EXPORTS)
    m = re.search(r"#define TWXPC_NKERNELS (\d+)", h)
    assert m and int(m.group(1)) == len(_qalib.PC_KERNELS)
    assert (_qalib.SP_OK, _qalib.SP_FEW_NGHS, _qalib.SP_NGH_CAP) == (RC.SP_OK, RC.SP_FEW_NGHS, RC.SP_NGH_CAP)
    assert _qalib.MAX_RADIUS_NGH == RC.MAX_RADIUS_NGH
    b = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_prcpcorrob.hip" in b
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_prcpcorrob.hip")).read()
    assert sorted(set(re.findall(r'extern "C" int (twxpc_\w+)\(', src))) == sorted(_qalib.PC_EXPORTS)
    assert sorted(set(re.findall(r"__global__[^\n]*\bvoid (k_\w+)\(", src))) == sorted(NEW_KERNELS)
    assert "atomicAdd(float" not in src and "atomicAdd(double" not in src
    assert len(re.findall(r"atomic\w+\(", src)) == 2                 # the histogram count and the window slot, both integers


def test_resource_table_lists_the_new_kernels():
    """No scratch, no spills, and the LDS of the rank kernel (no build in this checkout: skipped, as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    assert all(hasattr(lib, name) for name in _qalib.PC_EXPORTS)
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    lds = table["k_pc_rank"]["lds"]
    assert 4 * _qalib.PQ_MAX_WINDOW_VALUES <= lds <= 4 * _qalib.PQ_MAX_WINDOW_VALUES + 512
    assert 8 * lds <= 160 * 1024 and table["k_pc_rank"]["vgprs"] <= 128
    assert table["k_pc_walk"]["lds"] == 0 and table["k_pc_walk"]["vgprs"] <= 64


def test_import_surface():
    from topowx_amd.qa import qa_prcp
    for name in ("qa_spatial_corrob", "run_qa_spatial_only", "run_qa_all", "pors_counts", "PRCP_SPATIAL_FLAGS"):
        assert name in qa_prcp.__all__ and hasattr(qa_prcp, name), name
    assert qa_prcp.PRCP_SPATIAL_FLAGS == (2, 17) and qa_prcp.PRCP_TWX_TO_GHCN_FLAGS_MAP[17] == "S"
    assert qa_prcp.MAX_SPATIAL_COLLAB_THRES == RC.THRES and qa_prcp.MIN_NGHS == RC.MIN_NGHS and qa_prcp.MAX_NGHS == RC.MAX_NGHS


def _small_pool(qa_prcp, n=5, nd=40):
    rs = np.random.RandomState(4)
    days = get_days_metadata(dt.date(1990, 1, 1), dt.date(1990, 1, 1) + dt.timedelta(days=nd - 1))
    prcp = np.round(rs.rand(nd, n), 2).astype(np.float32)
    prcp[2, 1] = np.nan
    tmin = np.round(rs.randn(nd, n) * 5, 1).astype(np.float32)
    ids = np.array(["GHCN_%03d" % i for i in range(n)])
    lon, lat = -110 + 0.1 * rs.rand(n), 45 + 0.1 * rs.rand(n)
    return qa_prcp.PrcpObsPool(ids, lon, lat, prcp, tmin, tmin + 10, days), days


def test_argument_checks_come_before_any_device_work():
    from topowx_amd import _qalib
    from topowx_amd.qa import qa_prcp
    pool, days = _small_pool(qa_prcp)
    nd, n = pool.prcp.shape
    with pytest.raises(ValueError):
        qa_prcp.qa_spatial_corrob(pool, flags=np.ones((nd, n - 1), np.uint8))
    with pytest.raises(ValueError):
        qa_prcp.qa_spatial_corrob(pool, targets=[0, n])
    with pytest.raises(ValueError):
        qa_prcp.qa_spatial_corrob(pool, targets=["NOPE"])
    with pytest.raises(ValueError):
        qa_prcp.run_qa_spatial_only(pool, targets=[])
    with pytest.raises(ValueError):
        qa_prcp.pors_counts(pool.prcp[:-1], days)
    ymd = np.ascontiguousarray(days[YMD], np.int32)              # (a field of a record array is strided)
    sm =np.ascontiguousarray(pool.prcp.T)
    ones = np.ones((n, nd), np.uint8)
    with pytest.raises(ValueError):
        _qalib.prcp_spatial_corrob(pool.lon[:-1], pool.lat, sm, ymd, np.arange(n), ones)
    with pytest.raises(ValueError):
        _qalib.prcp_spatial_corrob(pool.lon, pool.lat, sm, ymd, np.arange(n), ones[:, :-1])
    with pytest.raises(ValueError):
        _qalib.prcp_spatial_corrob(pool.lon, pool.lat, sm, ymd, np.array([0.5]), ones[:1])
    with pytest.raises(ValueError):
        _qalib.prcp_spatial_corrob(pool.lon, pool.lat, sm, ymd, np.array([-1]), ones[:1])
    if not os.path.exists(_qalib.LIB_PATH):
        return
    # call-level failures of the library, each with a message and before any device work (none is needed here)
    bad = ymd.copy()
    bad[7] = bad[6]
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        _qalib.prcp_spatial_corrob(pool.lon, pool.lat, sm, bad, np.arange(n), ones)
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        _qalib.prcp_pors_counts(sm, bad)
    years = _qalib.PQ_MAX_WINDOW_VALUES // 29 + 1
    long_days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    series = np.zeros((3, long_days.size), np.float32)
    with pytest.raises(_qalib.QaError, match="TWXPQ_MAX_WINDOW_VALUES.*%d years" % (years - 1)):
        _qalib.prcp_spatial_corrob(pool.lon[:3], pool.lat[:3], series, long_days[YMD], np.arange(3),
                                   np.ones(series.shape, np.uint8))
    with pytest.raises(_qalib.QaError, match="%d years" % years):
        _qalib.prcp_pors_counts(series, long_days[YMD])
    # a target index out of range, past the binding's own check
    fn = _qalib.load().twxpc_spatial_corrob
    buf = ctypes.create_string_buffer(512)
    tgt = np.array([0, n], np.int32)
    fl = np.ones((2, nd), np.uint8)
    lon, lat = np.ascontiguousarray(pool.lon), np.ascontiguousarray(pool.lat)
    rc = fn(0, n, nd, lon.ctypes.data, lat.ctypes.data, sm.ctypes.data, ymd.ctypes.data, 2, tgt.ctypes.data, fl.ctypes.data,
            None, None, None, None, None, buf, 512)
    assert rc != 0 and b"target_idx[1] = 5 is not a row of the pool" in buf.value and (fl == 1).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_command_line_with_a_stand_in_for_the_library(tmp_path, capsys, monkeypatch, fmt):
    from topowx_amd.qa import qa_prcp
    pool0, days = _small_pool(qa_prcp)
    nd, n = pool0.prcp.shape
    db = PC.write_db(str(tmp_path / "all.nc"), pool0.ids, pool0.lon, pool0.lat, pool0.prcp, pool0.tmin, pool0.tmax, days, fmt,
                     qflags=("qflag_tmin", "qflag_tmax", "qflag_prcp"), prev=(("qflag_prcp", 7, 1, b"O"),))
    seen = {}

    def fake_chain(p, tv, days_, device=0, streak=False, frequent=False, details=False, timing=None):
        seen.update(chain=p.shape, streak=streak)
        timing.update(pq_gap_kernel_ms=1.0)
        f = np.where(np.isnan(p), 2, 1).astype(np.uint8)
        f[5, 0] = 10
        return f

    def fake_corrob(pool, targets=None, flags=None, device=0, details=False, timing=None):
        cols = qa_prcp._target_cols(pool, targets)
        f = np.where(np.isnan(pool.prcp[:, cols]), 2, 1).astype(np.uint8) if flags is None else np.array(flags)
        seen.update(corrob=f.shape, given=flags is not None, cols=cols.tolist())
        timing.update(pc_walk_kernel_ms=2.0)
        f[9, 0] = 17
        st = np.zeros(cols.size, np.int32)
        st[-1] = 1
        return {"flags": f, "status": st, "abs_dif": None, "pctile": None, "thres": None} if details else f

    monkeypatch.setattr(qa_prcp, "run_qa_non_spatial", fake_chain)
    monkeypatch.setattr(qa_prcp, "qa_spatial_corrob", fake_corrob)
    out = str(tmp_path / "r.npz")
    # the default invocation: today's report keys and files, no spatial call
    assert qa_prcp.main(["--db", db, "--out", out]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(line) == ["days", "flags_prcp", "pool", "pq_gap_kernel_ms", "seconds", "stations"] and "corrob" not in seen
    assert sorted(line["flags_prcp"]) == sorted(str(k) for k in (1, 2, 4, 5, 6, 8, 9, 10, 15, 19))
    assert sorted(np.load(out).files) == ["flags_prcp", "ids", "ymd"]
    with pytest.raises(SystemExit):
        qa_prcp.main(["--db", db, "--out", out, "--spatial", "--all"])
    capsys.readouterr()
    # --spatial: no chain call, the flags of the missing check go in
    seen.clear()
    assert qa_prcp.main(["--db", db, "--out", out, "--spatial"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "chain" not in seen and seen["corrob"] == (nd, n) and not seen["given"]
    assert line["chain"] == "spatial_only" and line["flags_prcp"] == {"1": nd * n - 2, "2": 1, "17": 1}
    assert line["status"] == {"0": n - 1, "1": 1} and line["pc_walk_kernel_ms"] == 2.0 and "rows_written" not in line
    rep = np.load(out)
    assert sorted(rep.files) == ["flags_prcp", "ids", "status", "ymd"] and rep["status"].tolist() == [0] * (n - 1) + [1]
    # --all --write on two targets: the chain's flags go into the check; 17 is written as "S", an earlier flag is kept
    tfile = tmp_path / "t.txt"
    tfile.write_text("GHCN_001\nGHCN_004\n")
    seen.clear()
    assert qa_prcp.main(["--db", db, "--out", out, "--all", "--streak", "--write", "--targets", str(tfile)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["chain"] == (nd, 2) and seen["streak"] and seen["given"] and seen["cols"] == [1, 4]
    assert line["chain"] == "all" and line["rows_written"] == 2 and line["flags_prcp"]["17"] == 1 and line["flags_prcp"]["10"] == 1
    assert sorted(line["flags_prcp"]) == sorted(str(k) for k in (1, 2, 4, 5, 6, 8, 9, 10, 15, 19, 17))
    back = qa_prcp.load_prcp_pool(db)
    assert back.qflag_prcp[9, 1] == b"S" and back.qflag_prcp[5, 1] == b"G" and back.qflag_prcp[7, 1] == b"O"
    assert (back.qflag_prcp != b"").sum() == 3
