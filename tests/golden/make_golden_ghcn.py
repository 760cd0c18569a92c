#!/usr/bin/env python3
"""Golden vectors of the GHCN-Daily ingest (step04), made by EXECUTING the reference's source (build container only; needs
the reference tree, see make_golden.py):

    python tests/golden/make_golden_ghcn.py

Executed: twx/db/create_db_all_stations.py:991-1026 (the body of ``InsertGhcn.get_stns``), :711-715 (``is_obs_inbounds``),
:1028-1040 (``__convert_units``) and :1058-1103 (the body of ``parse_stn_obs``) under a class header of ours that holds the
class constants of :943-949 as data; :619-627 (the assignment of a station's records into the float32 / character chunks);
twx/homog/tobs.py:121-157 (``create_tobs_db``'s line loop) on a stand-in variable, fed the lines the ``grep`` chain of
``create_tobs_file`` (:61-62) keeps -- the chain itself is run with the system's ``grep``.

Shims: those of the other makers (``long``, ``np.int``, ``unicode``), and what Python 3's text / bytes split asks for:
``open`` reads latin-1 text without newline translation (Python 2's ``str`` lines), and the flag fields of the record and
of the chunks are ``U1`` (encoded latin-1 into the fixture's uint8).  ``unicode(x, errors='ignore')`` has no Python 3
counterpart: it is restated as "ASCII, other bytes dropped" -- the station NAME is the one field not pinned by execution.
In-memory edits, each asserted to hit exactly as often as stated: ``obs_dict.has_key(ymd)`` -> ``ymd in obs_dict`` (once);
the Python 2 ``print`` statements -> ``pass`` (twice, both in get_stns); the two commented-out ``prcp`` assignments of
:623 / :626 uncommented (the reference parses precipitation and leaves it out of its file; the port writes it).

Input: ``tests/ghcn_cases.py``, pinned by ``input_hash``.  The scripted cases are stored in full; the seeded pool as one
sha256 per station.  Prints the executed reference's rate in MB of .dly text per second.  No reference text is stored.
"""
import hashlib
import io
import os
import subprocess
import sys
import tempfile
import textwrap
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import ghcn_cases as GC  # noqa: E402
import restate_ghcn as RG  # noqa: E402

REL = "twx/db/create_db_all_stations.py"
OUT = os.path.join(HERE, "golden_ghcn_v1.npz")
DTYPE_STNOBS = [("year", int), ("month", int), ("day", int), ("ymd", int), ("tmin", np.float64), ("tmax", np.float64),
                ("prcp", np.float64), ("swe", np.float64), ("qflag_tmin", "U1"), ("qflag_tmax", "U1"), ("qflag_prcp", "U1")]
HEADER = '''class InsertGhcn(object):
    VALID_FIPS_CODES = ["US", "CA", "MX"]
    VALID_ELEMENTS = ["TMIN", "TMAX", "PRCP"]
    RM_STATES = ["HI", "AK"]
    RM_NETWORK_CODES = ["S", "R"]
    ELEMENT_INDICES = {"TMIN": (4, 8), "TMAX": (5, 9), "PRCP": (6, 10)}
    MONTH_DAYS = range(1, 32)
    OBS_COLUMN_SIZE = 8

    def __init__(self, path_stn_file, path_obs_files, min_ymd, max_ymd, check_obs_exist=False):
        self.path_stn_file, self.path_obs_files, self.check_obs_exist = path_stn_file, path_obs_files, check_obs_exist
        self.min_ymd, self.max_ymd = min_ymd, max_ymd

'''


def _edit(text, old, new, times):
    assert text.count(old) == times, (old, text.count(old))
    return text.replace(old, new)


def _drop_prints(text, times):
    lines, n = text.split("\n"), 0
    for k, l in enumerate(lines):
        if l.lstrip().startswith("print "):
            lines[k] = l[:len(l) - len(l.lstrip())] + "pass"
            n += 1
    assert n == times, n
    return "\n".join(lines)


def load_reference():
    import make_golden as mg
    if not hasattr(np, "int"):
        np.int = int

    def text_open(path, mode="r"):
        return io.open(path, mode, encoding="latin-1", newline="\n")

    ns = dict(np=np, os=os, datetime=__import__("datetime"), long=int, MISSING=-9999., DTYPE_STNOBS=DTYPE_STNOBS, open=text_open,
              unicode=lambda s, errors=None: "".join(c for c in s if ord(c) < 128))
    src = (HEADER + "    def get_stns(self):\n" + _drop_prints(mg._slice(REL, 991, 1026), 2) + "\n" + mg._slice(REL, 711, 715) + "\n" +
           mg._slice(REL, 1028, 1040) + "\n    def parse_stn_obs(self, stn_id):\n" +
           _edit(mg._slice(REL, 1058, 1103), "not obs_dict.has_key(ymd)", "not ymd in obs_dict", 1))
    exec(compile(src, "create_db_all_stations.py", "exec"), ns)
    assign = textwrap.dedent(mg._slice(REL, 619, 627))
    assign = _edit(assign, "# prcp_chk[time_idx,stn_cnt]", "prcp_chk[time_idx,stn_cnt]", 1)
    assign = _edit(assign, "# qprcp_chk[time_idx,stn_cnt]", "qprcp_chk[time_idx,stn_cnt]", 1)
    ns["_assign"] = compile(assign, "create_db_all_stations.py:619", "exec")
    tobs = "def tobs_loop(stnids, days, YMD, fpath_tobs_file, tobs, subprocess, StatusCheck):\n" + mg._slice("twx/homog/tobs.py", 121, 157)
    exec(compile(tobs, "tobs.py", "exec"), ns)
    return ns


def days_of(min_ymd, max_ymd):
    d0, n = RG.day_axis(min_ymd, max_ymd)
    import datetime
    ymd = np.array([int((d0 + datetime.timedelta(k)).strftime("%Y%m%d")) for k in range(n)], np.int64)
    days = np.zeros(n, dtype=[("YMD", np.int64)])
    days["YMD"] = ymd
    return days


def run_case(ns, case, tmp):
    """(val [nfiles, 3, ndays], flag, raised [nfiles]) through the reference's parse and its chunk assignment."""
    days = days_of(case["min_ymd"], case["max_ymd"])
    n = days["YMD"].size
    nf = len(case["files"])
    val = np.full((nf, 3, n), -9999.0, np.float32)
    flag = np.zeros((nf, 3, n), np.uint8)
    raised = np.zeros(nf, bool)
    d = os.path.join(tmp, case["name"])
    os.makedirs(d)
    ins = ns["InsertGhcn"](None, d, case["min_ymd"], case["max_ymd"])
    nbytes, t0 = 0, time.perf_counter()
    for k, (stn, data) in enumerate(case["files"]):
        with open(os.path.join(d, stn + ".dly"), "wb") as fh:
            fh.write(data)
        nbytes += len(data)
        try:
            obs = ins.parse_stn_obs("GHCN_" + stn)
        except ValueError:
            raised[k] = True
            continue
        loc = dict(np=np, days=days, YMD="YMD", obs=obs, stn_cnt=0,
                   tmin_chk=np.ones((n, 1), np.float32) * -9999.0, tmax_chk=np.ones((n, 1), np.float32) * -9999.0,
                   prcp_chk=np.ones((n, 1), np.float32) * -9999.0, qtmin_chk=np.zeros((n, 1), "U1"),
                   qtmax_chk=np.zeros((n, 1), "U1"), qprcp_chk=np.zeros((n, 1), "U1"))
        exec(ns["_assign"], loc)
        for e, (a, q) in enumerate((("tmin_chk", "qtmin_chk"), ("tmax_chk", "qtmax_chk"), ("prcp_chk", "qprcp_chk"))):
            val[k, e] = loc[a][:, 0]
            flag[k, e] = [ord(c) if c else 0 for c in loc[q][:, 0]]
    return val, flag, raised, nbytes, time.perf_counter() - t0


def column_sha(val, flag):
    return hashlib.sha256(np.ascontiguousarray(val).tobytes() + np.ascontiguousarray(flag).tobytes()).hexdigest()


class _Var(object):
    def __setitem__(self, key, value):
        self.value = np.array(value)


class _Chk(object):
    def __init__(self, *a):
        pass

    def increment(self, *a):
        pass


def run_tobs(ns, case, tmp):
    days = days_of(case["min_ymd"], case["max_ymd"])
    path = os.path.join(tmp, case["name"] + ".txt")
    with open(path, "wb") as out:
        for k, data in enumerate(case["files"]):
            src = os.path.join(tmp, "%s_%d.csv" % (case["name"], k))
            with open(src, "wb") as fh:
                fh.write(data)
            cmd = "grep '%s' %s | grep -E '^US|^CA|^MX' | grep '[0-9]$' | grep -v '2400$'" % (case["element"], src)
            out.write(subprocess.run(cmd, shell=True, stdout=subprocess.PIPE, env=dict(os.environ, LC_ALL="C")).stdout)
    var = _Var()
    ids = np.array(["GHCN_" + s for s in case["ids"]])
    try:
        ns["tobs_loop"](ids, days, "YMD", path, var, subprocess, _Chk)
    except (ValueError, IndexError) as e:
        return np.zeros((len(ids), days["YMD"].size), np.int16), type(e).__name__
    a = var.value
    assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 32767
    return np.ascontiguousarray(a.astype(np.int16).T), ""


def main():
    ns = load_reference()
    out = {"input_hash": np.array(GC.input_hash())}
    with tempfile.TemporaryDirectory() as tmp:
        total, secs = 0, 0.0
        for case in GC.scripted_cases():
            val, flag, raised, nb, dt = run_case(ns, case, tmp)
            total, secs = total + nb, secs + dt
            out[case["name"] + "/val"], out[case["name"] + "/flag"], out[case["name"] + "/raised"] = val, flag, raised
            for k, (stn, data) in enumerate(case["files"]):           # the restatement must agree before anything is stored
                r = RG.parse_dly(data, case["min_ymd"], case["max_ymd"])
                assert (r["raised"] is not None) == bool(raised[k]), (case["name"], stn)
                if not raised[k]:
                    assert val[k].tobytes() == r["val"].tobytes() and np.array_equal(flag[k], r["flag"]), (case["name"], stn)
            print("%-16s %4d files, %3d raised, %6d values" % (case["name"], len(case["files"]), raised.sum(), (val != -9999).sum()))
        pool = GC.pool_case()
        val, flag, raised, nb, dt = run_case(ns, pool, tmp)
        total, secs = total + nb, secs + dt
        assert not raised.any()
        out["pool/sha"] = np.array([column_sha(val[k], flag[k]) for k in range(val.shape[0])])
        out["pool/nvalues"] = np.array([(val[k] != -9999).sum() for k in range(val.shape[0])], np.int64)
        print("pool: %d stations, %d values; reference %.2f MB/s on one core" % (val.shape[0], (val != -9999).sum(),
                                                                              total / secs / 1e6))
        # get_stns, with and without check_obs_exist
        stn_file = os.path.join(tmp, "ghcnd-stations.txt")
        with open(stn_file, "wb") as fh:
            fh.write(GC.stations_text())
        have = os.path.join(tmp, "have")
        os.makedirs(have)
        for sid in ("USC00010008", "CA001011501", "USS0010B04S"):
            open(os.path.join(have, sid + ".dly"), "w").close()
        for tag, chk in (("stns", False), ("stns_checked", True)):
            rows = ns["InsertGhcn"](stn_file, have, 19480101, 19481231, chk).get_stns()
            order = np.argsort(np.array([r[0] for r in rows], dtype=object))          # :502-509
            rows = [rows[k] for k in order]
            assert rows == RG.get_stns(GC.stations_text(), {"USC00010008", "CA001011501", "USS0010B04S"} if chk else None)
            out[tag + "/id"] = np.array([r[0] for r in rows])
            out[tag + "/num"] = np.array([r[1:4] for r in rows], np.float64).reshape(len(rows), 3)
            out[tag + "/state"] = np.array([r[4] for r in rows])
            out[tag + "/name"] = np.array([r[5] for r in rows])
            print(tag, [r[0] for r in rows])
        for case in GC.tobs_cases():
            a, exc = run_tobs(ns, case, tmp)
            out[case["name"] + "/tobs"], out[case["name"] + "/raised"] = a, np.array(exc)
            r = RG.parse_tobs(case["files"], case["ids"], case["element"], case["min_ymd"], case["max_ymd"])
            if exc == "":
                assert r["raised"] is None and r["outside"] == 0 and np.array_equal(r["tobs"], a), case["name"]
            elif exc == "IndexError":
                assert r["raised"] is None and r["outside"] > 0, case["name"]
            else:
                assert r["raised"] is not None, case["name"]
            print("%-20s %-10s %d values" % (case["name"], exc or "ok", (a != -1).sum()))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
