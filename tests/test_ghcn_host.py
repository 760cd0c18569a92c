"""The GHCN-Daily ingest (step04) without a GPU: the restatement against the executed reference (the golden fixture) on
every scripted case and the seeded pool, the station list, the writer's files in both containers, argument errors before
any device work, and the kernels' field logic (twx_ghcn_field.h) run on the CPU under the address and undefined-behaviour
sanitizers as a program of its own."""
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
import ghcn_cases as GC  # noqa: E402
import restate_ghcn as RG  # noqa: E402
from topowx_amd import _qalib, ghcn, h5nc, ncio, step04  # noqa: E402
from topowx_amd.dates import YMD, get_days_metadata  # noqa: E402
from topowx_amd.qa import qa_prcp, qa_temp  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "golden_ghcn_v1.npz"))
FORMATS = [pytest.param("NETCDF4", marks=pytest.mark.skipif(not h5nc.available(), reason="libhdf5 not loadable")),
           "NETCDF3_64BIT"]
HAVE = {"USC00010008", "CA001011501", "USS0010B04S"}


def column_sha(val, flag):
    return hashlib.sha256(np.ascontiguousarray(val).tobytes() + np.ascontiguousarray(flag).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def scripted():
    return GC.scripted_cases()


@pytest.fixture(scope="module")
def pool():
    return GC.pool_case()


def test_fixture_is_of_these_inputs():
    assert str(GOLD["input_hash"]) == GC.input_hash()
    size = os.path.getsize(os.path.join(HERE, "golden", "golden_ghcn_v1.npz"))
    assert size <= max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden"))
                       if f.endswith(".npz") and "ghcn" not in f)


def test_restatement_equals_the_executed_reference(scripted, pool):
    nraised = nfallback = 0
    for case in scripted:
        val, flag, raised = (GOLD[case["name"] + k] for k in ("/val", "/flag", "/raised"))
        assert val.shape[0] == len(case["files"])
        for k, (stn, data) in enumerate(case["files"]):
            r = RG.parse_dly(data, case["min_ymd"], case["max_ymd"])
            assert (r["raised"] is not None) == bool(raised[k]), (case["name"], stn)
            nraised += int(raised[k])
            if not raised[k]:
                assert r["val"].tobytes() == val[k].tobytes() and np.array_equal(r["flag"], flag[k]), (case["name"], stn)
                nfallback += len(r["fallback"])
    assert nraised == 20 and nfallback > 20
    # what the cut case pins: a cut inside a value field is the shorter number, a cut header raises, an empty file does not
    cut = {n: k for k, n in enumerate(range(271))}
    v, raised = GOLD["cut/val"], GOLD["cut/raised"]
    assert not raised[cut[0]] and raised[1:16].all() and not raised[16:].any()     # ('0' is a month)
    assert v[cut[23], 1, 0] == -9999.0 and v[cut[24], 1, 0] == np.float32(0.2) and v[cut[25], 1, 0] == np.float32(2.0)
    assert v[cut[26], 1, 0] == np.float32(20.0)
    for k, (stn, data) in enumerate(pool["files"]):
        r = RG.parse_dly(data, pool["min_ymd"], pool["max_ymd"])
        assert r["raised"] is None and r["fallback"] == []                # canonical text only: a condition of the pool
        assert column_sha(r["val"], r["flag"]) == str(GOLD["pool/sha"][k]), stn
        assert (r["val"] != -9999).sum() == GOLD["pool/nvalues"][k]


def test_python_route_equals_the_executed_reference(scripted):
    """``ghcn._parse_dly_python``, the route of a file whose header the kernel does not take: the golden arrays, and the
    reference's ValueError naming file and line."""
    for case in scripted:
        val, flag, raised = (GOLD[case["name"] + k] for k in ("/val", "/flag", "/raised"))
        a, b, d0, n = ghcn._period(case["min_ymd"], case["max_ymd"])
        for k, (stn, data) in enumerate(case["files"]):
            if raised[k]:
                with pytest.raises(ValueError, match=r"%s\.dly, line \d+" % stn):
                    ghcn._parse_dly_python(data, stn + ".dly", a, b, d0, n)
            else:
                v, q, _ = ghcn._parse_dly_python(data, stn + ".dly", a, b, d0, n)
                assert v.tobytes() == val[k].tobytes() and np.array_equal(q, flag[k]), (case["name"], stn)


def test_read_ghcn_stations_equals_get_stns(tmp_path):
    p = tmp_path / "ghcnd-stations.txt"
    p.write_bytes(GC.stations_text())
    obs = tmp_path / "obs"
    obs.mkdir()
    for s in HAVE:
        (obs / (s + ".dly")).write_bytes(b"")
    for tag, kw in (("stns", {}), ("stns_checked", dict(path_obs_files=str(obs), check_obs_exist=True))):
        stns = ghcn.read_ghcn_stations(str(p), **kw)
        assert list(stns["station_id"]) == list(GOLD[tag + "/id"]) and stns.size == GOLD[tag + "/id"].size
        assert np.array_equal(np.c_[stns["latitude"], stns["longitude"], stns["elevation"]], GOLD[tag + "/num"])
        assert list(stns["state"]) == list(GOLD[tag + "/state"]) and list(stns["station_name"]) == list(GOLD[tag + "/name"])
        rows = RG.get_stns(GC.stations_text(), HAVE if kw else None)
        assert [r[0] for r in rows] == list(stns["station_id"])
    assert "GHCN_USS0010B04S" not in GOLD["stns_checked/id"] and GOLD["stns/id"].size == 6
    assert "TIJUANA  AEROPUERTO" in list(GOLD["stns/name"])                # the non-ASCII byte dropped
    with pytest.raises(ValueError, match="path_obs_files"):
        ghcn.read_ghcn_stations(str(p), check_obs_exist=True)


def test_tobs_restatement_equals_the_executed_reference():
    seen = set()
    for case in GC.tobs_cases():
        want, exc = GOLD[case["name"] + "/tobs"], str(GOLD[case["name"] + "/raised"])
        r = RG.parse_tobs(case["files"], case["ids"], case["element"], case["min_ymd"], case["max_ymd"])
        seen.add(exc)
        if exc == "":
            assert r["raised"] is None and r["outside"] == 0 and np.array_equal(r["tobs"], want), case["name"]
        elif exc == "IndexError":                                          # the one deviation: skipped and counted
            assert r["raised"] is None and r["outside"] == 2
            assert np.array_equal(r["tobs"], GOLD["tobs/tobs"])
        else:
            assert r["raised"] == (0, case["files"][0].index(b"USC00010008,19480103"))
    assert seen == {"", "IndexError", "ValueError"}
    t = GOLD["tobs/tobs"]
    assert t[0, 0] == 1600 and t[3, 2] == 1700 and t[2, 6] == -100 and t[2, 7] == 630 and (t != -1).sum() == 9
    assert GOLD["tobs_last_line/tobs"][0, 9] == 900                        # grep ends the last line with a newline


def _write_case(tmp_path, case):
    d = tmp_path / case["name"]
    d.mkdir()
    paths = []
    for stn, data in case["files"]:
        (d / (stn + ".dly")).write_bytes(data)
        paths.append(str(d / (stn + ".dly")))
    return paths


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "ghcn_hostcheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "topowx_amd", "qa"), os.path.join(HERE, "tools", "ghcn_hostcheck.cpp"),
                           "-o", exe])
    return exe


def test_field_logic_on_the_cpu_under_sanitizers(hostcheck, scripted, tmp_path):
    """Every scripted case through the kernels' own field code, as a stand-alone program: the golden's arrays, a bad-header
    position exactly where the reference raised, the restatement's fallback list, a clean exit."""
    for case in scripted:
        paths = _write_case(tmp_path, case)
        man, out = tmp_path / (case["name"] + ".manifest"), tmp_path / (case["name"] + ".bin")
        man.write_text("dly %d %d %d\n%s\n" % (case["min_ymd"], case["max_ymd"], len(paths), "\n".join(paths)))
        res = subprocess.run([hostcheck, str(man), str(out)], capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
        val, flag, raised = (GOLD[case["name"] + k] for k in ("/val", "/flag", "/raised"))
        nf, _, nd = val.shape
        raw = out.read_bytes()
        got_v = np.frombuffer(raw, np.float32, nf * 3 * nd).reshape(nf, 3, nd)
        got_q = np.frombuffer(raw, np.uint8, nf * 3 * nd, offset=nf * 3 * nd * 4).reshape(nf, 3, nd)
        p = nf * 3 * nd * 5
        bad = np.frombuffer(raw, np.uint32, nf, offset=p)
        nvalues, nfb = np.frombuffer(raw, np.int64, 2, offset=p + 4 * nf)
        fb = np.frombuffer(raw, np.int64, 3 * nfb, offset=p + 4 * nf + 16).reshape(nfb, 3)
        want_fb, want_n = [], 0
        for k, (stn, data) in enumerate(case["files"]):
            r = RG.parse_dly(data, case["min_ymd"], case["max_ymd"])
            assert (bad[k] != 0xffffffff) == bool(raised[k]) and (not raised[k] or bad[k] == r["raised"]), (case["name"], stn)
            if raised[k]:
                continue
            want_fb += [(k, pos, d) for pos, d in r["fallback"]]
            if not r["fallback"]:                                         # (fields left to float() are settled in Python)
                assert got_v[k].tobytes() == val[k].tobytes() and np.array_equal(got_q[k], flag[k]), (case["name"], stn)
                want_n += r["nvalues"]
        assert sorted(map(tuple, fb.tolist())) == sorted(t for t in want_fb)
        if not want_fb and not raised.any():
            assert nvalues == want_n


def test_tobs_field_logic_on_the_cpu_under_sanitizers(hostcheck, tmp_path):
    for case in GC.tobs_cases():
        paths = []
        for k, data in enumerate(case["files"]):
            paths.append(str(tmp_path / ("%s_%d.csv" % (case["name"], k))))
            with open(paths[-1], "wb") as fh:
                fh.write(data)
        man, out = tmp_path / (case["name"] + ".manifest"), tmp_path / (case["name"] + ".bin")
        man.write_text("tobs %d %d %d %d %s\n%s\n%s\n" % (case["min_ymd"], case["max_ymd"], len(paths), len(case["ids"]),
                                                       case["element"], "\n".join(sorted(case["ids"])), "\n".join(paths)))
        res = subprocess.run([hostcheck, str(man), str(out)], capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
        r = RG.parse_tobs(case["files"], sorted(case["ids"]), case["element"], case["min_ymd"], case["max_ymd"])
        raw = out.read_bytes()
        n = r["tobs"].size
        got = np.frombuffer(raw, np.int16, n).reshape(r["tobs"].shape)
        values, outside, nbad = np.frombuffer(raw, np.int64, 3, offset=2 * n)
        assert (nbad > 0) == (r["raised"] is not None) and outside == r["outside"]
        if r["raised"] is None:
            assert np.array_equal(got, r["tobs"]) and values == r["nvalues"]
            if str(GOLD[case["name"] + "/raised"]) == "":
                assert np.array_equal(got, GOLD[case["name"] + "/tobs"])


@pytest.mark.parametrize("fmt", FORMATS)
def test_writer_files_open_with_the_readers_and_hold_the_golden(tmp_path, fmt, scripted):
    case = [c for c in scripted if c["name"] == "files"][0]
    keep = np.nonzero(~GOLD["files/raised"])[0]
    val, flag = GOLD["files/val"][keep], GOLD["files/flag"][keep]
    n, _, nd = val.shape
    ids = np.array(sorted("GHCN_" + case["files"][k][0] for k in keep))
    stns = np.zeros(n, ghcn.STN_DTYPE)
    stns["station_id"], stns["latitude"], stns["longitude"] = ids, 40.0 + np.arange(n), -100.0 - np.arange(n)
    stns["elevation"], stns["state"], stns["station_name"] = 100.0, "TX", ["NAME %d" % k for k in range(n)]
    a, b, d0, _ = ghcn._period(case["min_ymd"], case["max_ymd"])
    days = get_days_metadata(d0, d0 + (nd - 1) * (d0.resolution))
    assert days.size == nd and days[YMD][0] == a and days[YMD][-1] == b
    sm_v, sm_q = np.ascontiguousarray(val.transpose(1, 0, 2)), np.ascontiguousarray(flag.transpose(1, 0, 2))
    tobs = (np.arange(n * nd).reshape(n, nd) % 2400 - 1).astype(np.int16)
    db = str(tmp_path / "all.nc")
    ghcn.write_all_stations_db(db, stns, days, [(0, 3, sm_v[:, :3], sm_q[:, :3]), (3, n, sm_v[:, 3:], sm_q[:, 3:])],
                               tobs=tobs, format=fmt)
    assert ncio.file_format(db) == fmt
    for e, name in enumerate(ghcn.ELEMENTS):
        rs, _, rdays, obs = ncio.read_station_db_arrays(db, name)
        assert list(rs["station_id"]) == list(ids) and np.array_equal(rdays[YMD], days[YMD])
        assert obs.tobytes() == np.ascontiguousarray(val[:, e].T).tobytes()
        assert np.array_equal(rs["latitude"], stns["latitude"]) and list(rs["state"]) == ["TX"] * n
        assert list(rs["station_name"]) == list(stns["station_name"])
    with ncio.open_dataset(db, "r") as ds:
        for e, name in enumerate(ghcn.ELEMENTS):
            q = qa_temp.read_qflags(ds.variables["qflag_" + name])
            want = np.ascontiguousarray(flag[:, e].T).view("S1")
            assert np.array_equal(q, want) and (q != b"").sum() == (flag[:, e] != 0).sum()
            if fmt == "NETCDF4":
                assert ds.variables[name].chunking() == [nd, 1] and not ds.variables[name].filters()["zlib"]
        t = ds.variables["tobs_tmax"]
        assert np.dtype(t.dtype) == np.int16 and np.array_equal(t[:], tobs.T) and int(t.getncattr("missing_value")) == -1
    pl = qa_prcp.load_prcp_pool(db, qflags=True)
    want = np.where(val[:, 2] == -9999, np.nan, val[:, 2]).T
    assert np.array_equal(pl.prcp, want, equal_nan=True) and np.array_equal(pl.qflag_prcp, flag[:, 2].T.copy().view("S1"))
    with pytest.raises(ValueError, match="batch"):
        ghcn.write_all_stations_db(str(tmp_path / "bad.nc"), stns, days, [(0, 2, sm_v[:, :3], sm_q[:, :3])], format=fmt)


def test_argument_errors_come_before_any_device_work(tmp_path):
    """None of these reaches the device: they pass on a machine without one."""
    with pytest.raises(ValueError, match="not a date"):
        ghcn.parse_dly_files([], "1948-13-01x", 19481231)
    with pytest.raises(ValueError):
        ghcn.parse_dly_files([], 19480230, 19481231)
    with pytest.raises(ValueError, match="before it starts"):
        ghcn.parse_dly_files([], 19490101, 19481231)
    with pytest.raises(ValueError, match="sorted"):
        ghcn.parse_tobs_files([], ["B", "A"], 19480101, 19481231)
    with pytest.raises(ValueError, match="four characters"):
        ghcn.parse_tobs_files([], ["A"], 19480101, 19481231, element="TMAXX")
    stn = tmp_path / "ghcnd-stations.txt"
    stn.write_bytes(GC.stations_text())
    (tmp_path / "obs").mkdir()
    with pytest.raises(IOError, match="station GHCN_CA001011500: no observation file"):
        ghcn.create_all_stations_db(str(tmp_path / "x.nc"), str(stn), str(tmp_path / "obs"), 19480101, 19481231)
    assert not (tmp_path / "x.nc").exists()
    assert step04.main(["--stations", str(stn), "--dly-dir", str(tmp_path / "obs"), "--out", str(tmp_path / "x.nc"),
                        "--start", "19480101", "--end", "19481231"]) == 1
    assert step04.main(["--stations", str(tmp_path / "none.txt"), "--dly-dir", str(tmp_path), "--out", str(tmp_path / "x.nc"),
                        "--start", "19480101", "--end", "19481231"]) == 1
    for s in ("CA001011500", "CA001011501", "MXN00002001", "USC00010008", "USC00010009", "USW00094728"):
        (tmp_path / "obs" / (s + ".dly")).write_bytes(b"")
    with pytest.raises(IOError, match="no by-year file 1948"):
        ghcn.create_all_stations_db(str(tmp_path / "x.nc"), str(stn), str(tmp_path / "obs"), 19480101, 19481231,
                                    path_by_year=str(tmp_path))
    assert ghcn._batches([5, 5, 5, 20, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 5)] and ghcn.MAX_READERS <= 16
    assert ghcn._batches([1] * 5, 10, 2) == [(0, 2), (2, 4), (4, 5)] and ghcn._batches([], 10) == []
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    ok = dict(buf=b"abc\n", file_off=[0, 4], file_col=[0], nrows=1, min_ymd=19480101, max_ymd=19480110, ndays=10)
    for kw, exc, pat in ((dict(file_off=[0, 5]), ValueError, "buffer holds"), (dict(file_off=[1, 4]), ValueError, "from 0"),
                         (dict(file_col=[1]), ValueError, "distinct rows"), (dict(ndays=9), _qalib.QaError, "number of days"),
                         (dict(max_ymd=19480100), _qalib.QaError, "not a period"),
                         (dict(min_ymd=19480230, ndays=1), _qalib.QaError, "not a period")):
        with pytest.raises(exc, match=pat):
            _qalib.ghcn_parse_dly(**dict(ok, **kw))
    t = np.full((2, 10), -1, np.int16)
    tk = dict(buf=b"x\n", file_off=[0, 2], ids11=["A", "B"], element="TMAX", min_ymd=19480101, max_ymd=19480110, win0=0, tobs=t)
    for kw, exc, pat in ((dict(ids11=["B", "A"]), ValueError, "sorted"), (dict(tobs=t.astype(np.int32)), ValueError, "int16"),
                         (dict(win0=5), _qalib.QaError, "window"), (dict(element="TMA"), ValueError, "four")):
        with pytest.raises(exc, match=pat):
            _qalib.ghcn_parse_tobs(**dict(tk, **kw))


def test_unit_is_declared_bound_and_built():
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxgh_\w+)\s*\(", h))) == sorted(_qalib.GH_EXPORTS)
    assert int(re.search(r"#define TWXGH_NKERNELS (\d+)", h).group(1)) == len(_qalib.GH_KERNELS)
    assert int(re.search(r"#define TWXGH_FB_WORDS (\d+)", h).group(1)) == _qalib.GH_FB_WORDS
    assert int(re.search(r"#define TWXGH_MAX_BYTES \(\(int64_t\)(\d+)\)", h).group(1)) == _qalib.GH_MAX_BYTES
    assert "topowx_amd/qa/twx_ghcn.hip" in open(os.path.join(ROOT, "build.sh")).read()
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    import ctypes
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    assert all(hasattr(lib, n) for n in _qalib.GH_EXPORTS)
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    rows = {l.split("|")[0].strip(): [c.strip() for c in l.split("|")] for l in open(res) if l.startswith("k_gh_")}
    assert sorted(rows) == ["k_gh_count", "k_gh_dly<0>", "k_gh_dly<1>", "k_gh_fill", "k_gh_scan", "k_gh_starts", "k_gh_tobs<0>",
                            "k_gh_tobs<1>"]
    head = [c.strip() for c in open(res).readline().split("|")]
    k = [i for i, c in enumerate(head) if "scratch" in c.lower()]
    assert k and all(int(r[k[0]]) == 0 for r in rows.values())
