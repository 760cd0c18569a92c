"""CPU: step05 / step09-11 without a GPU -- the numpy restatement (tests/restate_homog.py) against the executed-reference
golden (tests/golden/make_golden_homog.py) bit for bit; the writers of PHA's input tree against the bytes the executed
reference wrote and the parsers of PHA's output against the arrays the executed parsers returned; header / binding /
build naming; the resource table of a build; the argument errors of the bindings and of the four ``twxhm_`` entries (they
come before any launch) and the error paths of the command lines."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import homog_cases as HC  # noqa: E402
import restate_homog as RH  # noqa: E402

from topowx_amd import _qalib, homog, obs_por  # noqa: E402
from topowx_amd import stationdb as sdb  # noqa: E402

NEW_KERNELS = ("k_hm_cnt", "k_hm_means", "k_hm_tobs", "k_hm_delta", "k_hm_apply")


@pytest.fixture(scope="module")
def gold():
    return HC.load_fixture()


def stns_of(gold):
    n = gold["ids"].size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U32"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64),
                              ("station_name", "U30")])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = gold["ids"], gold["lon"], gold["lat"], gold["elev"]
    stns["station_name"] = gold["name"]
    return stns


def test_golden_content(gold):
    assert os.path.getsize(HC.FIXTURE) <= 1 << 20
    assert gold["raw_tmin"].shape == (51, 2192) and (gold["year"][0], gold["year"][-1]) == (1979, 1984)
    assert gold["mth_first"].size == 72 and gold["mth_ndays"][13] == 29               # February 1980
    miss, mean = gold["mth_miss_tmin"], gold["mth_mean_tmin"]
    g = dict(((y, m), 12 * (y - 1979) + m - 1) for y in range(1979, 1985) for m in range(1, 13))
    assert miss[0, g[1980, 3]] == 9 and not np.isnan(mean[0, g[1980, 3]])             # exactly max_miss: kept
    assert miss[0, g[1980, 4]] == 10 and np.isnan(mean[0, g[1980, 4]])                # one more: masked
    assert miss[0, g[1980, 2]] == 10 and np.isnan(mean[0, g[1980, 2]]) and miss[0, g[1981, 2]] == 9
    assert miss[1, g[1982, 6]] == 30 == gold["mth_ndays"][g[1982, 6]] and gold["pha_tmin"][1, g[1982, 6]] == 1500
    assert np.isnan(gold["delta_tmin"][1, g[1982, 6]])                                 # miss == ndays: untouched
    assert mean[5, g[1983, 4]] == np.float32(1.125) and RH.round2(1.125) == 1.12       # a tie held by float32: to even
    assert np.isnan(mean[50, 12:]).all() and (miss[50, 12:] == gold["mth_ndays"][12:]).all()
    d = gold["delta_tmin"][2]                                                          # before, start, end, inside, after
    st, ad = gold["adj_start_tmin"], gold["adj_tmin"]
    mine = gold["adj_ids_tmin"] == gold["fmt_ids"][2]
    a1, a2 = ad[mine][np.argsort(st[mine])]
    assert d[g[1979, 3]] == RH.round2(-a1) and d[g[1980, 1]] == RH.round2(-a1) and d[g[1981, 6]] == RH.round2(-a1)
    assert d[g[1982, 3]] == RH.round2(-a2) and d[g[1984, 5]] == 0.0 and not np.signbit(d[g[1984, 5]])
    mine = gold["adj_ids_tmin"] == gold["fmt_ids"][3]
    assert 0.0 in ad[mine].tolist()                                                    # a station with an adj of 0
    assert set(gold["tobs_nshift"].tolist()) >= {0, 1, 2} and gold["tobs_nshift"][10] == 1 and gold["tobs_nshift"][11] == 2
    assert gold["tobs_tmax"][10].tobytes() == gold["obs_tmax"][10].tobytes()           # |S| = 1: nothing moves
    assert gold["tobs_tmax"][11, 99] == np.float32(20.5) and gold["tobs_tmax"][11, 100] == np.float32(22.5)
    assert gold["tobs_tmax"][12, 0] == np.float32(2.5) and gold["tobs_tmax"][12, 1] == np.float32(3.5)   # day 0 is not shifted
    assert np.isnan(gold["tobs_tmax"][12, 2])
    assert not gold["por_tmin_1"][50] and not gold["por_tmin_1"][49] and gold["por_tmax_1"][49] and not gold["por_tmax_1"][48]
    assert gold["por_tmin_5"].sum() < gold["por_tmin_1"].sum()


def test_restatement_equals_the_golden(gold):
    nd = gold["year"].size
    shifted, nshift = RH.tobs_shift(gold["obs_tmax"], gold["tobs"])
    assert shifted.tobytes() == gold["tobs_tmax"].tobytes() and np.array_equal(nshift, gold["tobs_nshift"])
    mf, mn, mymd = RH.month_groups(gold["year"], gold["month"])
    assert np.array_equal(mf, gold["mth_first"]) and np.array_equal(mn, gold["mth_ndays"]) and np.array_equal(mymd, gold["mth_ymd"])
    for v, rows in (("tmin", gold["obs_tmin"]), ("tmax", gold["tobs_tmax"])):
        assert np.array_equal(RH.obs_cnt(gold["raw_" + v], gold["month"], 0, nd - 1), gold["cnt_" + v])
        for yrs in (1, 5):
            assert np.array_equal(obs_por._build_a_por_mask(gold["cnt_" + v].T, yrs), gold["por_%s_%d" % (v, yrs)])
        mean, miss = RH.monthly_means(rows, mf, mn, 9)
        assert mean.tobytes() == gold["mth_mean_" + v].tobytes() and np.array_equal(miss, gold["mth_miss_" + v])
        off, st, en, ad = HC.adj_csr(gold["fmt_ids"], gold["adj_ids_" + v], gold["adj_start_" + v], gold["adj_end_" + v],
                                     gold["adj_" + v])
        r = RH.homog_daily(rows, mean, miss, gold["pha_" + v], mymd, mf, mn, off, st, en, ad)
        assert r["out"].tobytes() == gold["homog_" + v].tobytes() and r["delta"].tobytes() == gold["delta_" + v].tobytes()
        assert not r["status"].any() and np.array_equal(r["nchanged"], gold["nchanged_" + v])


def test_writers_equal_the_reference_bytes(gold, tmp_path):
    stns = stns_of(gold)
    assert [homog.format_stnid(s) for s in gold["ids"]] == gold["fmt_ids"].tolist()
    assert homog.format_stnid("NRCS_806:MT:SNTL") == "SNT806MTSNT" and homog.format_stnid("RAWS_T003") == "WRC0000T003"
    with pytest.raises(ValueError):
        homog.format_stnid("XX_1")
    with pytest.raises(ValueError, match="11 characters"):
        homog.format_stnid("GHCND_USC0024")
    hist = list(zip(gold["hist_ids"].tolist(), gold["hist_yyyymm"].tolist()))
    for v in ("tmin", "tmax"):
        run = str(tmp_path / v)
        p = homog.pha_paths(run, v)
        os.makedirs(p["raw"])
        open(os.path.join(p["raw"], "example.raw.tavg"), "w").close()
        mean = np.ma.masked_invalid(gold["mth_mean_" + v].T)
        homog.write_input_station_data(run, v, stns, mean, np.arange(1979, 1985), hist)
        assert open(p["stnlist"]).read() == str(gold["stnlist_" + v])
        assert open(p["metadata"]).read() == str(gold["metadata_file"])
        assert sorted(os.listdir(p["raw"])) == sorted("%s.raw.%s" % (f, v) for f in gold["fmt_ids"])
        for f, text in zip(gold["fmt_ids"], gold["raw_files_" + v]):
            assert open(os.path.join(p["raw"], "%s.raw.%s" % (f, v))).read() == str(text), f
    bad = stns[:1].copy()
    bad[sdb.LON] = 10.0
    with pytest.raises(ValueError, match="negative Lons"):
        homog.write_stn_list(bad, str(tmp_path / "x"))


def drop_pha_files(gold, pha_dir):
    """PHA's output of the fixture under ``pha_dir``/<var>, where ``step11 --apply`` reads it."""
    for v in ("tmin", "tmax"):
        p = homog.pha_paths(os.path.join(pha_dir, v), v)
        for d in (p["fls"], os.path.dirname(p["adj_log"]), p["corr"]):
            os.makedirs(d, exist_ok=True)
        for f, text in zip(gold["fmt_ids"], gold["fls_files_" + v]):
            with open(os.path.join(p["fls"], "%s.FLs.r00.%s" % (f, v)), "w") as fh:
                fh.write(str(text))
        with open(p["adj_log"], "w") as fh:
            fh.write(str(gold["adj_log_" + v]))
        with open(os.path.join(p["corr"], "corr.%s.input_not_stnlist" % v), "w") as fh:
            fh.write(str(gold["not_stnlist_" + v]))


def test_parsers_equal_the_reference_arrays(gold, tmp_path):
    drop_pha_files(gold, str(tmp_path))
    for v, skip in (("tmin", [7]), ("tmax", [8, 20])):
        run = str(tmp_path / v)
        p = homog.pha_paths(run, v)
        adjs = homog.parse_pha_adj(p["adj_log"])
        assert adjs[sdb.STN_ID].tolist() == gold["adj_ids_" + v].tolist()
        assert np.array_equal(adjs["ymd_start"], gold["adj_start_" + v]) and np.array_equal(adjs["ymd_end"], gold["adj_end_" + v])
        assert adjs["adj"].tobytes() == gold["adj_" + v].tobytes()
        pha = homog.read_pha_monthly(p["fls"], gold["fmt_ids"], v, np.arange(1979, 1985))
        assert pha.dtype == np.int32 and np.array_equal(pha, gold["pha_" + v]) and (pha == -9999).any()
        assert homog.load_input_not_stnlist(run).tolist() == sorted(gold["fmt_ids"][skip].tolist())
        with pytest.raises(ValueError, match="not on the database's axis"):
            homog.read_pha_monthly(p["fls"], gold["fmt_ids"][:1], v, np.arange(1980, 1985))
    # the CSV of step28: non-zero adjustments of known stations, sign flipped, months moved on by one
    stns = stns_of(gold)[:4]
    rows = homog.get_pha_adj_csv(homog.pha_paths(str(tmp_path / "tmin"), "tmin")["adj_log"], stns, "tmin", str(tmp_path / "adj.csv"))
    text = open(str(tmp_path / "adj.csv")).read().splitlines()
    assert text[0] == "STN_ID,YEAR_MONTH_START,YEAR_MONTH_END,ADJ(C),VARIABLE,NAME,LON,LAT,ELEV(m)" and len(text) == 1 + len(rows)
    assert 1 <= len(rows) <= 8 and set(r[0] for r in rows) <= set(gold["ids"][:4].tolist())
    assert set(r[1] for r in rows) <= {"198002", "198108"} and set(r[2] for r in rows) <= {"198107", "198401"}
    mine = gold["adj_ids_tmin"] == gold["fmt_ids"][0]
    assert sorted(float(r[3]) for r in rows if r[0] == gold["ids"][0]) == sorted((-gold["adj_tmin"][mine]).tolist())


def test_names_in_header_binding_and_build():
    hdr = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    for name in _qalib.HM_EXPORTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
    for name, val in (("TWXHM_NO_ADJ", _qalib.HM_NO_ADJ), ("TWXHM_OVERLAP", _qalib.HM_OVERLAP),
                      ("TWXHM_MAX_MONTHS", _qalib.HM_MAX_MONTHS), ("TWXHM_DEFAULT_MAX_MISS", _qalib.HM_MAX_MISS)):
        assert re.search(r"#define %s \(?%d\b" % (name, val), hdr), name
    assert re.search(r"#define TWXHM_PHA_MISSING \(-9999\)", hdr) and _qalib.HM_PHA_MISSING == -9999 == RH.PHA_MISSING
    assert (RH.NO_ADJ, RH.OVERLAP) == (_qalib.HM_NO_ADJ, _qalib.HM_OVERLAP)
    assert "topowx_amd/qa/twx_homog.hip" in open(os.path.join(ROOT, "build.sh")).read()
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_homog.hip")).read()
    assert "atomic" not in src.replace("no float atomics", "").replace("No atomics", "")
    for k in NEW_KERNELS:
        assert re.search(r"void %s\(" % k, src), k


def test_exports_are_in_the_built_library():
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("libtwxqa.so has not been built")
    L = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.HM_EXPORTS:
        assert hasattr(L, name), name


def test_new_kernels_use_no_scratch():
    path = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(path):
        pytest.skip("libtwxqa.so has not been built")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    table = isa_resources.parse(path)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    assert table["k_hm_means"]["lds"] == 4 * (128 * 31 + 8) and table["k_hm_cnt"]["lds"] == 4 * 4 * 12


def small_case():
    return HC.random_case(3, 4, HC.START, HC.END)


def test_binding_argument_errors_come_before_the_library():
    """Every one of these raises in the binding, before libtwxqa.so is loaded: they pass without a build."""
    c = small_case()
    nd = c["obs"].shape[1]
    args = [c[k] for k in ("obs", "mth_mean", "mth_miss", "pha", "mth_ymd", "mth_first", "mth_ndays", "adj_off", "adj_start",
                           "adj_end", "adj")]
    far = c["mth_first"].copy()
    far[-1] = nd - 5                                                                  # the last month runs past the axis
    with pytest.raises(ValueError, match="outside the day axis"):
        _qalib.monthly_means(c["obs"], far, c["mth_ndays"])
    with pytest.raises(ValueError, match="outside the day axis"):
        _qalib.homog_daily(*(args[:5] + [far] + args[6:]))
    gap = c["mth_first"].copy()
    gap[3] += 1
    with pytest.raises(ValueError, match="consecutive"):
        _qalib.monthly_means(c["obs"], gap, c["mth_ndays"])
    with pytest.raises(ValueError, match="nstn"):
        _qalib.monthly_means(c["obs"][0], c["mth_first"], c["mth_ndays"])
    with pytest.raises(ValueError, match="like the record"):
        _qalib.tobs_shift(c["obs"], c["tobs"][:, :-1])
    with pytest.raises(ValueError, match=r"\[nstn, nmth\]"):
        _qalib.homog_daily(*(args[:3] + [c["pha"][:, :-1]] + args[4:]))
    assert c["adj_off"][1] >= 2
    st = c["adj_start"].copy()
    st[0], st[1] = st[1] + 100, st[0]
    with pytest.raises(ValueError, match="sorted"):
        _qalib.homog_daily(*(args[:8] + [st] + args[9:]))
    with pytest.raises(ValueError, match="ascending from 0"):
        _qalib.homog_daily(*(args[:7] + [c["adj_off"][::-1].copy()] + args[8:]))
    with pytest.raises(ValueError, match="day_month"):
        _qalib.obs_cnt(c["obs"], c["month"][:-1], 0, nd - 1)
    with pytest.raises(ValueError, match="first_day"):
        _qalib.obs_cnt(c["obs"], c["month"], 5, nd)
    a, b, y = _qalib.month_groups(c["year"], c["month"])
    assert np.array_equal(a, c["mth_first"]) and np.array_equal(b, c["mth_ndays"]) and np.array_equal(y, c["mth_ymd"])
    with pytest.raises(ValueError, match="gap-free"):
        _qalib.month_groups(c["year"][::-1], c["month"][::-1])


def test_entry_argument_errors_come_before_any_launch():
    """The same mistakes handed to the C entries: -1 and a message, with device -1 never reached (no GPU needed)."""
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("libtwxqa.so has not been built")
    L = ctypes.CDLL(_qalib.LIB_PATH)
    c = small_case()
    ns, nd = c["obs"].shape
    nm = c["mth_first"].size
    buf = ctypes.create_string_buffer(512)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                                       # noqa: E731
    i64, i32 = ctypes.c_int64, ctypes.c_int32
    mean, miss = np.empty((ns, nm), np.float32), np.empty((ns, nm), np.int16)
    far = c["mth_first"].copy()
    far[-1] = nd - 5
    rc = L.twxhm_monthly_means(-1, i64(ns), i64(nd), p(c["obs"]), i32(nm), p(far), p(c["mth_ndays"]), i32(9), i64(0), p(mean),
                               p(miss), None, None, buf, 512)
    assert rc == -1 and b"outside the day axis" in buf.value
    rc = L.twxhm_monthly_means(-1, i64(0), i64(nd), p(c["obs"]), i32(nm), p(c["mth_first"]), p(c["mth_ndays"]), i32(9), i64(0),
                               p(mean), p(miss), None, None, buf, 512)
    assert rc == -1 and b"nstn" in buf.value
    st = c["adj_start"].copy()
    st[0], st[1] = st[1] + 100, st[0]
    delta, out = np.empty((ns, nm)), np.empty((ns, nd), np.float32)
    status, nch = np.empty(ns, np.int32), np.empty(ns, np.int32)
    rc = L.twxhm_homog_daily(-1, i64(ns), i64(nd), p(c["obs"]), i32(nm), p(c["mth_mean"]), p(c["mth_miss"]), p(c["pha"]),
                             p(c["mth_ymd"]), p(c["mth_first"]), p(c["mth_ndays"]), p(c["adj_off"]), p(st), p(c["adj_end"]),
                             p(c["adj"]), i64(0), p(delta), p(out), p(status), p(nch), None, None, buf, 512)
    assert rc == -1 and b"not sorted" in buf.value
    cnt = np.empty((ns, 12), np.int32)
    mon = c["month"].astype(np.int8)
    rc = L.twxhm_obs_cnt(-1, i64(ns), i64(nd), p(c["obs"]), p(mon), i64(3), i64(nd), i64(0), p(cnt), None, None, buf, 512)
    assert rc == -1 and b"first_day" in buf.value
    rc = L.twxhm_tobs_shift(-1, i64(ns), i64(nd), p(c["obs"]), None, i64(0), p(out), p(status), None, None, buf, 512)
    assert rc == -1 and b"null buffer" in buf.value


def test_command_lines_fail_cleanly(tmp_path, capsys):
    from topowx_amd import step05, step09, step10, step11
    missing = str(tmp_path / "none.nc")
    assert step05.main(["--db", missing, "--start", "19790101", "--end", "19841231"]) == 1
    assert step09.main(["--db", missing, "--out", str(tmp_path / "o.nc"), "--start", "19790101", "--end", "19841231"]) == 1
    assert step10.main(["--db", missing]) == 1
    assert step11.main(["--db", missing, "--pha-dir", str(tmp_path), "--setup"]) == 1
    err = capsys.readouterr().err
    assert all(("step%s:" % s) in err for s in ("05", "09", "10", "11"))
    for mod in (step05, step09, step10, step11):
        with pytest.raises(SystemExit) as e:
            mod.main(["--help"])
        assert e.value.code == 0
    with pytest.raises(SystemExit):
        step11.main(["--db", missing, "--pha-dir", str(tmp_path), "--apply"])            # --apply needs --out
    assert "usage: python -m topowx_amd.step11" in capsys.readouterr().out
