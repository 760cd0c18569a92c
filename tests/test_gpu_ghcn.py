"""GPU: the GHCN-Daily ingest (``twxgh_parse_dly`` / ``twxgh_parse_tobs`` of libtwxqa, ``topowx_amd.ghcn``, ``python -m
topowx_amd.step04``) against the executed-reference golden (tests/golden/make_golden_ghcn.py) and the restatement
(tests/restate_ghcn.py).  Every comparison is for equality -- values bit for bit, flags, statuses, lists, counts: nothing is
computed but an exact division and one rounding."""
import gzip
import hashlib
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib, ghcn, ncio, step04, step05, step09
from topowx_amd.qa import qa_prcp, qa_temp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ghcn_cases as GC  # noqa: E402
import restate_ghcn as RG  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = _qalib.GH_NO_BAD_HEADER


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_ghcn_v1.npz"))
    assert str(g["input_hash"]) == GC.input_hash(), "case generator drifted: regenerate the golden"
    return g


@pytest.fixture(scope="module")
def scripted():
    return GC.scripted_cases()


@pytest.fixture(scope="module")
def restated(scripted):
    return {c["name"]: [RG.parse_dly(d, c["min_ymd"], c["max_ymd"]) for _, d in c["files"]] for c in scripted}


def _buffer(files):
    off = np.zeros(len(files) + 1, np.int64)
    off[1:] = np.cumsum([len(d) for _, d in files])
    return b"".join(d for _, d in files), off


def _raw(case, files=None, **kw):
    files = case["files"] if files is None else files
    buf, off = _buffer(files)
    _, _, _, nd = ghcn._period(case["min_ymd"], case["max_ymd"])
    return _qalib.ghcn_parse_dly(buf, off, np.arange(len(files), dtype=np.int32), len(files), case["min_ymd"], case["max_ymd"],
                                 nd, **kw)


def _write(tmp, case):
    d = tmp / case["name"]
    d.mkdir()
    out = []
    for stn, data in case["files"]:
        (d / (stn + ".dly")).write_bytes(data)
        out.append(str(d / (stn + ".dly")))
    return out


def test_kernels_on_every_scripted_case(gold, scripted, restated):
    """The whole case in one buffer (the cut case ends with the buffer inside a line at every length): the kernel's own
    outputs.  Headers: the position of the first line ``int()`` refuses, exactly where the reference raised.  Files without
    a field left to ``float()``: the golden's arrays.  The fallback list: the restatement's, exactly.  Two calls: the same
    bytes."""
    for case in scripted:
        val, flag, bad, fb, counts = _raw(case, fallback_cap=2)          # (too small on purpose: the call is repeated)
        again = _raw(case)
        for a, b in zip((val, flag, bad, fb, counts), again):
            assert a.tobytes() == b.tobytes(), case["name"]
        gv, gq, raised = (gold[case["name"] + k] for k in ("/val", "/flag", "/raised"))
        want_fb = []
        for k, r in enumerate(restated[case["name"]]):
            assert (bad[k] != NONE) == bool(raised[k]) and (not raised[k] or bad[k] == r["raised"]), (case["name"], k)
            if raised[k]:
                continue
            want_fb += [(k, pos, d) for pos, d in r["fallback"]]
            if not r["fallback"]:
                assert val[:, k].tobytes() == gv[k].tobytes() and np.array_equal(flag[:, k], gq[k]), (case["name"], k)
        assert [tuple(r) for r in fb[:, [0, 1, 3]].tolist()] == sorted(want_fb), case["name"]
        assert counts[2] == len(want_fb)
        good = [f for k, f in enumerate(case["files"]) if not raised[k]]
        c = _raw(case, good)[4]
        nfloat = sum(r["nvalues"] for k, r in enumerate(restated[case["name"]]) if not raised[k])
        nlater = 0
        for k, r in enumerate(restated[case["name"]]):
            if not raised[k]:
                for pos, d in r["fallback"]:
                    line = case["files"][k][1][pos:].split(b"\n")[0] + b"\n"
                    try:
                        float(line[21 + 8 * d:26 + 8 * d])
                        nlater += 1
                    except ValueError:
                        pass
        assert c[1] + nlater == nfloat, case["name"]


def test_module_on_every_scripted_case(gold, scripted, tmp_path):
    """``ghcn.parse_dly_files``: the page-locked buffer, the reader threads, the fields settled by ``float()``.  The files
    the reference parsed equal the golden everywhere, in one batch and in many; a file it raised on raises ``ValueError``
    naming the file and the line."""
    for case in scripted:
        paths = _write(tmp_path, case)
        gv, gq, raised = (gold[case["name"] + k] for k in ("/val", "/flag", "/raised"))
        keep = np.nonzero(~raised)[0]
        stats = {}
        val, flag = ghcn.parse_dly_files([paths[k] for k in keep], case["min_ymd"], case["max_ymd"], stats=stats)
        assert val.tobytes() == np.ascontiguousarray(gv[keep].transpose(1, 0, 2)).tobytes(), case["name"]
        assert flag.tobytes() == np.ascontiguousarray(gq[keep].transpose(1, 0, 2)).tobytes(), case["name"]
        assert stats["bytes"] == sum(len(case["files"][k][1]) for k in keep)
        for bb in (1, 3000):                                              # a file per batch; a few files per batch
            v2, q2 = ghcn.parse_dly_files([paths[k] for k in keep], case["min_ymd"], case["max_ymd"], batch_bytes=bb)
            assert v2.tobytes() == val.tobytes() and q2.tobytes() == flag.tobytes(), (case["name"], bb)
        bad = np.nonzero(raised)[0]
        if bad.size:
            k = int(bad[0])
            with pytest.raises(ValueError, match=r"%s\.dly, line \d+" % case["files"][k][0]):
                ghcn.parse_dly_files(paths, case["min_ymd"], case["max_ymd"])
            for k in bad[1::4]:
                with pytest.raises(ValueError, match=r"line \d+"):
                    ghcn.parse_dly_files([paths[k]], case["min_ymd"], case["max_ymd"], pinned=False)


def test_seeded_pool(gold, tmp_path):
    pool = GC.pool_case()
    paths = _write(tmp_path, pool)
    stats, tm = {}, {}
    val, flag = ghcn.parse_dly_files(paths, pool["min_ymd"], pool["max_ymd"], stats=stats, timing=tm)
    sha = [hashlib.sha256(val[:, k].tobytes() + flag[:, k].tobytes()).hexdigest() for k in range(len(paths))]
    assert sha == [str(s) for s in gold["pool/sha"]]
    assert stats["fallback"] == 0 and stats["values"] >= int(gold["pool/nvalues"].sum())
    assert stats["lines"] >= sum(d.count(b"\n") for _, d in pool["files"]) and set(tm) == {k + "_kernel_ms" for k in _qalib.GH_KERNELS}
    assert all(np.isfinite(v) and v >= 0 for v in tm.values()), tm
    v2, q2 = ghcn.parse_dly_files(paths, pool["min_ymd"], pool["max_ymd"], batch_bytes=400000)
    assert v2.tobytes() == val.tobytes() and q2.tobytes() == flag.tobytes()
    # rows may be given in any order: file f fills row file_col[f]
    buf, off = _buffer(pool["files"][:5])
    perm = np.array([3, 0, 4, 1, 2], np.int32)
    _, _, _, nd = ghcn._period(pool["min_ymd"], pool["max_ymd"])
    v3 = _qalib.ghcn_parse_dly(buf, off, perm, 5, pool["min_ymd"], pool["max_ymd"], nd)[0]
    assert v3[:, perm].tobytes() == val[:, :5].tobytes()


def _tobs_files(tmp, case, gz):
    out = []
    for k, data in enumerate(case["files"]):
        year = 1948 + k
        p = tmp / ("%s_%d.csv%s" % (case["name"], year, ".gz" if gz else ""))
        with (gzip.open(p, "wb") if gz else open(p, "wb")) as fh:
            fh.write(data)
        out.append((year, str(p)))
    return out


def test_times_of_observation(gold, tmp_path):
    for n, case in enumerate(GC.tobs_cases()):
        files = _tobs_files(tmp_path, case, gz=n % 2 == 0)
        want, exc = gold[case["name"] + "/tobs"], str(gold[case["name"] + "/raised"])
        r = RG.parse_tobs(case["files"], case["ids"], case["element"], case["min_ymd"], case["max_ymd"])
        if exc == "ValueError":
            with pytest.raises(ValueError, match=r"tobs_bad_700_1948\.csv.*, line 6"):
                ghcn.parse_tobs_files(files, case["ids"], case["min_ymd"], case["max_ymd"], element=case["element"])
            continue
        stats, tm = {}, {}
        got = ghcn.parse_tobs_files(files, ["GHCN_" + s for s in case["ids"]], case["min_ymd"], case["max_ymd"],
                                    element=case["element"], stats=stats, timing=tm)
        assert got.dtype == np.int16 and np.array_equal(got, r["tobs"]) and stats["outside"] == r["outside"], case["name"]
        assert all(np.isfinite(tm[k + "_kernel_ms"]) and tm[k + "_kernel_ms"] >= 0 for k in _qalib.GH_KERNELS), tm
        if exc == "":
            assert np.array_equal(got, want), case["name"]
        else:                                                              # the one deviation: skipped and counted
            assert stats["outside"] == 2 and np.array_equal(got, gold["tobs/tobs"])
        # no year given: one window over the period; pieces cut after newlines
        again = ghcn.parse_tobs_files([(None, p) for _, p in files], case["ids"], case["min_ymd"], case["max_ymd"],
                                      element=case["element"], piece_bytes=100)
        assert again.tobytes() == got.tobytes(), case["name"]


def test_step04_end_to_end_then_step05_and_step09(gold, tmp_path):
    """Generated files in a temporary directory -> ``python -m topowx_amd.step04 --by-year`` -> a database the readers
    open and that holds the golden's columns -> ``step05`` and ``step09`` run on it."""
    pool = GC.pool_case()
    obs, yrly = tmp_path / "ghcnd_all", tmp_path / "by_year"
    obs.mkdir(), yrly.mkdir()
    for stn, data in pool["files"]:
        (obs / (stn + ".dly")).write_bytes(data)
    pool_ids = sorted(s for s, _ in pool["files"])
    (tmp_path / "ghcnd-stations.txt").write_bytes(GC.stations_text(pool_ids))
    r = np.random.RandomState(5)
    by_year = []
    for year in range(1948, 1953):
        lines = []
        for day in range(1, 29):
            for s in pool_ids[::3] + ["USC00099999"]:
                lines.append(("%s,%d01%02d,TMAX,%5d,,,0,%s\n" % (s, year, day, r.randint(-300, 400),
                                                                  ("0700", "1800", "2400", "0800")[r.randint(4)])).encode())
        by_year.append(b"".join(lines))
        with gzip.open(yrly / ("%d.csv.gz" % year), "wb") as fh:
            fh.write(by_year[-1])
    db = str(tmp_path / "all.nc")
    args = ["--stations", str(tmp_path / "ghcnd-stations.txt"), "--dly-dir", str(obs), "--out", db, "--start", "19480101",
            "--end", "1952-12-31", "--by-year", str(yrly)]
    assert step04.main(args) == 1                                          # the scripted stations have no .dly file
    assert step04.main(args + ["--check-obs-exist"]) == 0
    order = [pool_ids.index(s) for s, _ in pool["files"]]
    stns, _, days, tmin = ncio.read_station_db_arrays(db, "tmin")
    assert list(stns["station_id"]) == ["GHCN_" + s for s in pool_ids] and days.size == 1827
    assert list(stns["station_name"][:2]) == ["POOL 0", "POOL 1"] and stns["longitude"][1] == -100.5
    pl = qa_prcp.load_prcp_pool(db, qflags=False)
    with ncio.open_dataset(db, "r") as ds:
        cols = {n: ds.variables[n][:] for n in ghcn.ELEMENTS}
        flags = {n: qa_temp.read_qflags(ds.variables["qflag_" + n]) for n in ghcn.ELEMENTS}
        tobs = ds.variables["tobs_tmax"][:]
    for k, j in enumerate(order):
        val = np.stack([cols[n][:, j] for n in ghcn.ELEMENTS]).astype(np.float32)
        flag = np.stack([flags[n][:, j] for n in ghcn.ELEMENTS])
        flag = np.ascontiguousarray(flag).view(np.uint8).reshape(3, -1)
        assert hashlib.sha256(val.tobytes() + flag.tobytes()).hexdigest() == str(gold["pool/sha"][k])
    assert np.array_equal(np.isnan(pl.prcp), cols["prcp"] == -9999)
    want = RG.parse_tobs(by_year, pool_ids, "TMAX", 19480101, 19521231)
    assert want["raised"] is None and np.array_equal(tobs, want["tobs"].T) and (tobs != -1).sum() > 1000
    assert step05.main(["--db", db, "--start", "19480101", "--end", "19521231"]) == 0
    out = str(tmp_path / "tobs_adj.nc")
    assert step09.main(["--db", db, "--out", out, "--start", "19480101", "--end", "19521231"]) == 0
    kept, _, _, tmax = ncio.read_station_db_arrays(out, "tmax")
    assert kept.size > 0 and np.isfinite(np.where(tmax == -9999, np.nan, tmax)).any()
    # the stand-alone file of create_tobs_db
    t = ghcn.create_tobs_db(str(yrly), str(tmp_path / "tobs.nc"), np.array(["GHCN_" + s for s in pool_ids]), 19480101, 19521231)
    with ncio.open_dataset(str(tmp_path / "tobs.nc"), "r") as ds:
        assert np.array_equal(ds.variables["tobs"][:], want["tobs"].T) and np.array_equal(t, want["tobs"])
