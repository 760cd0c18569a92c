"""The RAWS ingest (step04) without a GPU: the restatement against the executed reference (the golden fixture) on every
scripted case and the seeded pool, exception type and line included; the station table; the host's own line parser and its
settlement of the lists; the host-buffer pieces; argument errors before any device work; and the kernels' token and field
code (twx_raws_field.h) run on the CPU under the address and undefined-behaviour sanitizers as a program of its own.

The cases with duplicate dates are pinned by the restatement alone: the reference fails on them (make_golden_raws.py)."""
import ctypes as C
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
import raws_cases as RC  # noqa: E402
import restate_raws as RR  # noqa: E402
from topowx_amd import _qalib, ghcn, raws, step04  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "golden_raws_v1.npz"))


@pytest.fixture(scope="module")
def scripted():
    return RC.scripted_cases()


@pytest.fixture(scope="module")
def pool():
    return RC.pool_case()


def test_fixture_is_of_these_inputs():
    assert str(GOLD["input_hash"]) == RC.input_hash()
    assert os.path.getsize(os.path.join(HERE, "golden", "golden_raws_v1.npz")) < 100000
    assert float(GOLD["reference_mb_per_s"]) > 0


def test_restatement_equals_the_executed_reference(scripted, pool):
    seen = set()
    for case in scripted:
        if case["duplicates"]:
            assert case["name"] + "/val" not in GOLD.files
            continue
        val, raised, where = (GOLD[case["name"] + k] for k in ("/val", "/raised", "/line"))
        assert val.shape[0] == len(case["files"])
        for k, (stn, data) in enumerate(case["files"]):
            r = RR.parse_raws(data, case["min_ymd"], case["max_ymd"])
            assert (r["raised"] or ("", 0)) == (str(raised[k]), int(where[k])), (case["name"], stn)
            seen.add(str(raised[k]))
            if not raised[k]:
                assert r["val"].tobytes() == val[k].tobytes(), (case["name"], stn)
                assert (r["skipped"], r["values"], r["duplicates"]) == (GOLD[case["name"] + "/skipped"][k],
                                                                        GOLD[case["name"] + "/values"][k], 0), (case["name"], stn)
    assert seen == {"", "IndexError", "ValueError"}
    # what the cut case pins: a cut date is skipped, a cut line raises IndexError from its first byte in the period on,
    # a cut inside the last token is the shorter number
    full = RC.line(RC.date(40), b"30.25", b"-1.5", b"254", eol=b"")
    raised, v = GOLD["cut/raised"], GOLD["cut/val"]
    minus = full.index(b"-1.5") + 1                                # cut after the sign: float("-") comes before vals[14]
    assert len(raised) == len(full) + 1 and (raised[:10] == "").all() and raised[minus] == "ValueError"
    assert (np.delete(raised[10:len(full) - 2], minus - 10) == "IndexError").all() and (raised[len(full) - 2:] == "").all()
    assert [v[len(full) - 2 + k, 2, 40] for k in range(3)] == [np.float32(0.2), np.float32(2.5), np.float32(25.4)]
    assert v[len(full), 0, 40] == np.float32(-1.5) and v[len(full), 1, 40] == np.float32(30.25)
    # the numbers
    num = GOLD["numbers/val"][0]
    assert num[1, 200] == -9999 and num[2, 202] == -9999 and num[2, 205] == -9999 and np.signbit(num[1, 206]) and num[1, 206] == 0
    assert num[2, 208] == np.float32(-0.0 * 0.1) and num[1, 209] == 0.5 and num[1, 212] == 5.0 and num[1, 215] == 1.25
    for k, (stn, data) in enumerate(pool["files"]):
        r = RR.parse_raws(data, pool["min_ymd"], pool["max_ymd"])
        assert r["raised"] is None and r["duplicates"] == 0
        assert hashlib.sha256(r["val"].tobytes()).hexdigest() == str(GOLD["pool/sha"][k]), stn
        assert (r["values"], r["skipped"]) == (GOLD["pool/values"][k], GOLD["pool/skipped"][k])
        unc, rse, c = RR.device_view(data, pool["min_ymd"], pool["max_ymd"])
        assert unc == [] and rse == [] and c["values"] == r["values"]         # plain decimals only: a condition of the pool
    assert GOLD["pool/values"].sum() > 20000 and GOLD["pool/skipped"].sum() == 0


def test_duplicates_in_the_restatement(scripted):
    case = [c for c in scripted if c["name"] == "dups"][0]
    r = [RR.parse_raws(data, case["min_ymd"], case["max_ymd"]) for _, data in case["files"]]
    assert [x["duplicates"] for x in r] == [1, 1, 7] and all(x["raised"] is None for x in r)
    assert r[0]["val"][:, 5].tolist() == [-9999.0, 2.0, -9999.0]                  # the last line, all three values
    assert r[1]["val"][1, 0] == np.float32(77.5) and r[1]["val"][1, 1000] == 0.0
    assert r[2]["val"][1, 6] == 2.0 and r[2]["val"][1, 7] == 10.0


def _settled(case, files=None):
    """The module's host side on the restated device view of a batch: (val [3, nfiles, ndays], counts) or the exception."""
    files = case["files"] if files is None else files
    a, b, d0, nd = ghcn._period(case["min_ymd"], case["max_ymd"])
    off = np.zeros(len(files) + 1, np.int64)
    off[1:] = np.cumsum([len(d) for _, d in files])
    buf = b"".join(d for _, d in files)
    val = np.full((3, len(files), nd), -9999.0, np.float32)
    win = np.zeros((len(files), nd), np.uint32)
    unc, rse = [], []
    for f, (stn, data) in enumerate(files):
        u, r, c = RR.device_view(data, a, b, f=f, base=int(off[f]))
        unc, rse = unc + u, rse + r
        # what the kernels write: the decided lines, the last one of a day winning
        for pos, line in RR.body_of(data):
            toks = line.split()
            if toks and len(toks[0]) <= 40 and all(RR.device_int(s) for s in (toks[0][6:], toks[0][0:2], toks[0][3:5])):
                got = RR.parse_line(line, a, b, d0) if len(toks) >= 15 and all(RR.device_float(toks[j]) for j in (9, 10, 14)) else None
                if isinstance(got, tuple):
                    val[:, f, got[0]] = got[1:]
                    win[f, got[0]] = off[f] + pos + 1
    unc = np.array(unc, np.uint32).reshape(-1, 8)
    rse = np.array(rse, np.uint32).reshape(-1, 8)
    paths = [stn + ".txt" for stn, _ in files]
    return val, raws._settle(memoryview(buf), off, paths, val, win, unc, rse, a, b, d0)


def test_host_settlement_equals_the_executed_reference(scripted):
    """``raws._settle`` on the restated lists: the golden arrays, and the reference's exception naming file and line."""
    for case in scripted:
        for k, (stn, data) in enumerate(case["files"]):
            want = RR.parse_raws(data, case["min_ymd"], case["max_ymd"])
            if want["raised"]:
                exc = dict(IndexError=IndexError, ValueError=ValueError)[want["raised"][0]]
                assert case["duplicates"] or (str(GOLD[case["name"] + "/raised"][k]), GOLD[case["name"] + "/line"][k]) == want["raised"]
                with pytest.raises(exc, match=r"^%s\.txt, line %d: " % (stn, want["raised"][1])):
                    _settled(case, [(stn, data)])
                continue
            val, (added, dups, skipped) = _settled(case, [(stn, data)])
            assert val[:, 0].tobytes() == want["val"].tobytes(), (case["name"], stn)
            if not case["duplicates"]:
                assert val[:, 0].tobytes() == np.ascontiguousarray(GOLD[case["name"] + "/val"][k]).tobytes(), (case["name"], stn)
            c = RR.device_view(data, case["min_ymd"], case["max_ymd"])[2]
            assert (c["values"] + added, c["duplicates"] + dups, c["skipped"] + skipped) == (want["values"], want["duplicates"],
                                                                                             want["skipped"]), (case["name"], stn)


def test_first_error_is_in_station_then_line_order(scripted):
    case = [c for c in scripted if c["name"] == "numbers"][0]
    # file 1 raises ValueError on its line 9, file 14 IndexError... a batch raises what its first raising file raises
    with pytest.raises(ValueError, match=r"^NU01\.txt, line 9: "):
        _settled(case)
    with pytest.raises(IndexError, match=r"^NU17\.txt, line 9: "):
        _settled(case, [case["files"][0], case["files"][17], case["files"][1]])


def test_read_raws_stations_equals_get_stns(tmp_path):
    ids, meta, have = RC.station_files()
    (tmp_path / "ids.txt").write_bytes(ids)
    (tmp_path / "meta.txt").write_bytes(meta)
    obs = tmp_path / "obs"
    obs.mkdir()
    for s in have:
        (obs / (s + ".txt")).write_bytes(b"")
    st = {}
    stns = raws.read_raws_stations(str(tmp_path / "meta.txt"), str(tmp_path / "ids.txt"), str(obs), stats=st)
    assert list(stns["station_id"]) == list(GOLD["stns/id"]) == ["RAWS_CSQU", "RAWS_IBOI", "RAWS_NEXG", "RAWS_NEXH", "RAWS_UBRY"]
    assert np.array_equal(np.c_[stns["latitude"], stns["longitude"], stns["elevation"]], GOLD["stns/num"])
    assert list(stns["state"]) == list(GOLD["stns/state"]) == ["CA", "ID", "NV", "NV", "UT"]
    assert list(stns["station_name"]) == list(GOLD["stns/name"]) and st == {"raws_no_obs": 1}
    assert stns["station_name"][1] == "BOISE FIRE COLE" and stns["station_name"][0] == "" and stns["longitude"][3] == 121.0
    rows, missing = RR.get_stns(ids, meta, have)
    assert [r[0] for r in rows] == list(stns["station_id"]) and missing == 1
    kid, kmeta = RC.station_files_keyerror()
    (tmp_path / "kids.txt").write_bytes(kid)
    (tmp_path / "kmeta.txt").write_bytes(kmeta)
    assert str(GOLD["stns_keyerror"]) == "KeyError"
    with pytest.raises(KeyError, match="MT1"):
        raws.read_raws_stations(str(tmp_path / "kmeta.txt"), str(tmp_path / "kids.txt"), str(obs))


def test_host_buffer_pieces_and_argument_errors(tmp_path):
    """None of these reaches the device: they pass on a machine without one."""
    b = ghcn._HostBuffer(10)
    p = tmp_path / "a.txt"
    p.write_bytes(b"0123456789")
    ghcn._read_into(str(p), b.view[0:10])
    assert bytes(b.view) == b"0123456789" and raws._line_at(b.view, 3, 10) == b"3456789"
    b.close()
    long_line = b"x" * 9000 + b"\nrest"
    assert raws._line_at(memoryview(long_line), 1, len(long_line)) == b"x" * 8999
    assert raws._line_at(memoryview(b"ab\n"), 3, 3) == b""
    with pytest.raises(ValueError, match="not a date"):
        raws.parse_raws_files([], "2000-13-01x", 20001231)
    with pytest.raises(ValueError, match="before it starts"):
        raws.parse_raws_files([], 20010101, 20001231)
    with pytest.raises(ValueError, match="batch_bytes"):
        raws.parse_raws_files([str(p)], 20000101, 20001231, batch_bytes=0)
    assert raws.parse_raws_files([], 20000101, 20000110).shape == (3, 0, 10)
    with pytest.raises(IOError, match="station RAWS_NONE: no observation file"):
        raws._raws_paths(["RAWS_NONE"], str(tmp_path))
    # the command line: all three RAWS arguments or none
    with pytest.raises(SystemExit):
        step04.main(["--stations", "s", "--dly-dir", "d", "--out", "o", "--start", "20000101", "--end", "20000131", "--raws-ids", "i"])
    with pytest.raises(ValueError, match="raws must be"):
        stn = tmp_path / "ghcnd-stations.txt"
        stn.write_bytes(b"USC00010008  31.5703  -85.2483  139.0 AL ABBEVILLE\n")
        (tmp_path / "USC00010008.dly").write_bytes(b"")
        ghcn.create_all_stations_db(str(tmp_path / "x.nc"), str(stn), str(tmp_path), 20000101, 20000131, raws=("a", "b"))
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    ok = dict(buf=b"abc\n", file_off=[0, 4], min_ymd=20000101, max_ymd=20000110, ndays=10)
    for kw, exc, pat in ((dict(file_off=[0, 5]), ValueError, "buffer holds"), (dict(file_off=[1, 4]), ValueError, "from 0"),
                         (dict(ndays=9), _qalib.QaError, "number of days"), (dict(max_ymd=20000100), _qalib.QaError, "not a period"),
                         (dict(min_ymd=20000230, ndays=1), _qalib.QaError, "not a period"),
                         (dict(uncertain_cap=-1), ValueError, "capacities"), (dict(ndays=1 << 40), ValueError, "cells")):
        with pytest.raises(exc, match=pat):
            raws.raws_parse(**dict(ok, **kw))


def test_unit_is_declared_bound_and_built():
    h = open(os.path.join(ROOT, "include", "twx_raws.h")).read()
    assert sorted(set(re.findall(r"\b(twxrw_\w+)\s*\(", h))) == [raws.RW_ENTRY]
    # the prototype the module binds is the header's: as many arguments, a pointer where the header has one
    params = re.search(r"int twxrw_parse\(([^)]*)\)", h).group(1).split(",")
    restype, argtypes = raws.RW_PROTOTYPE
    scalar = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert restype is C.c_int and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        assert (t in (C.c_void_p, C.c_char_p)) if "*" in p else t is scalar[p.replace("const", " ").split()[0]], p
    assert int(re.search(r"#define TWXRW_NKERNELS (\d+)", h).group(1)) == len(raws.RW_KERNELS)
    assert int(re.search(r"#define TWXRW_ENTRY_WORDS (\d+)", h).group(1)) == raws.RW_ENTRY_WORDS
    assert int(re.search(r"#define TWXRW_C_N (\d+)", h).group(1)) == len(raws.RW_COUNTS)
    assert int(re.search(r"#define TWXRW_MAX_BYTES \(\(int64_t\)(\d+)\)", h).group(1)) == raws.RW_MAX_BYTES == _qalib.GH_MAX_BYTES
    f = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_raws_field.h")).read()
    assert int(re.search(r"#define RW_TOK_MAX (\d+)", f).group(1)) == RR.TOK_MAX
    # what the tests of the other units ask of a unit: named in the build script once, the shared scaffold, no clean-up of its own
    assert open(os.path.join(ROOT, "build.sh")).read().count("topowx_amd/qa/twxrw_raws.hip 2>") == 1
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twxrw_raws.hip")).read()
    assert '#include "twx_qa_common.h"' in src and '#include "twx_raws.h"' in src
    assert not any(owned in src for owned in ("hipFree(", "hipEventDestroy(", "hipGetErrorString("))
    for doc in ("README.md", "DESIGN.md"):
        assert "twxrw_parse" in open(os.path.join(ROOT, doc)).read()
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    import ctypes
    assert all(hasattr(ctypes.CDLL(_qalib.LIB_PATH), n) for n in [raws.RW_ENTRY])
    rows = {l.split("|")[0].strip(): [c.strip() for c in l.split("|")] for l in open(res) if l.startswith("k_rw_")}
    assert sorted(rows) == ["k_rw_body", "k_rw_fill", "k_rw_line<0>", "k_rw_line<1>", "k_rw_stop"]
    head = [c.strip() for c in open(res).readline().split("|")]
    k = [i for i, c in enumerate(head) if "scratch" in c.lower()]
    assert k and all(int(r[k[0]]) == 0 for r in rows.values())


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "raws_hostcheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "topowx_amd", "qa"), os.path.join(HERE, "tools", "raws_hostcheck.cpp"),
                           "-o", exe])
    return exe


def test_field_logic_on_the_cpu_under_sanitizers(hostcheck, scripted, pool, tmp_path):
    """Every scripted case and the pool through the kernels' own token and field code, as a stand-alone program: the values
    of the decided lines, the eight counts and both lists as the restatement gives them, a clean exit."""
    for case in scripted + [pool]:
        d = tmp_path / case["name"]
        d.mkdir()
        paths = []
        for stn, data in case["files"]:
            (d / (stn + ".txt")).write_bytes(data)
            paths.append(str(d / (stn + ".txt")))
        man, out = tmp_path / (case["name"] + ".manifest"), tmp_path / (case["name"] + ".bin")
        man.write_text("raws %d %d %d\n%s\n" % (case["min_ymd"], case["max_ymd"], len(paths), "\n".join(paths)))
        res = subprocess.run([hostcheck, str(man), str(out)], capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
        raw = out.read_bytes()
        nf, nd = np.frombuffer(raw, np.int64, 2)
        p = 16
        val = np.frombuffer(raw, np.float32, nf * 3 * nd, offset=p).reshape(nf, 3, nd)
        p += nf * 3 * nd * 4
        cnt = np.frombuffer(raw, np.int64, nf * 8, offset=p).reshape(nf, 8)
        p += nf * 64
        nu = int(np.frombuffer(raw, np.int64, 1, offset=p)[0])
        unc = np.frombuffer(raw, np.int64, nu * 8, offset=p + 8).reshape(nu, 8)
        p += 8 + nu * 64
        nr = int(np.frombuffer(raw, np.int64, 1, offset=p)[0])
        rse = np.frombuffer(raw, np.int64, nr * 8, offset=p + 8).reshape(nr, 8)
        want_u, want_r = [], []
        for k, (stn, data) in enumerate(case["files"]):
            u, r, c = RR.device_view(data, case["min_ymd"], case["max_ymd"], f=k)
            want_u, want_r = want_u + u, want_r + r
            assert cnt[k].tolist() == [c[n] for n in raws.RW_COUNTS], (case["name"], stn)
            if not u and not r:                                    # every line decided: the file's final values
                assert val[k].tobytes() == RR.parse_raws(data, case["min_ymd"], case["max_ymd"])["val"].tobytes(), (case["name"], stn)
        assert [tuple(e) for e in unc.tolist()] == want_u and [tuple(e) for e in rse.tolist()] == want_r, case["name"]
