#!/usr/bin/env python3
"""Golden vectors of the RAWS ingest (step04), made by EXECUTING the reference's source (build container only; needs the
reference tree, see make_golden.py):

    python tests/golden/make_golden_raws.py

Executed: twx/db/create_db_all_stations.py:1143-1175 (the body of ``InsertRaws.get_stns``), :711-715 (``is_obs_inbounds``)
and :1193-1233 (the body of ``parse_stn_obs``) under a class header of ours; :619-623 (the assignment of a station's
records into the float32 chunks).

Shims: those of make_golden_ghcn.py (``long``, ``np.int``, ``unicode`` restated as "ASCII, other bytes dropped": the station
NAME is the one field not pinned by execution).  ``get_stns`` reads latin-1 text without newline translation;
``parse_stn_obs`` reads BYTES, so that ``line.split()`` splits at the six ASCII whitespace bytes as Python 2's ``str.split``
does (Python 3's ``str.split`` knows more).  In-memory edits, each asserted to hit exactly as often as stated:
``"Copyright" in line`` -> ``b"Copyright" in line`` (once); the Python 2 ``print`` statements of get_stns -> ``pass`` (three
times); the ``print`` of a skipped date -> a counter (once); the commented-out ``prcp`` assignment of :623 uncommented (once:
the reference parses precipitation and leaves it out of its file; the port writes it).

The line of a recorded exception is found by executing the reference on the file cut after its n-th line, n ascending.
Cases with DUPLICATE DATES are not stored: the reference's assignment fails on them (asserted here), the port lets the last
line win, and the restatement alone (tests/restate_raws.py) pins them.

Input: ``tests/raws_cases.py``, pinned by ``input_hash``.  The scripted cases are stored in full; the seeded pool as one
sha256 per station.  Stores results and exception types only: no reference text.  Prints the executed reference's rate in
MB of listing text per second.
"""
import hashlib
import io
import os
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
import raws_cases as RC  # noqa: E402
import restate_raws as RR  # noqa: E402
from make_golden_ghcn import DTYPE_STNOBS, _drop_prints, _edit, days_of  # noqa: E402

REL = "twx/db/create_db_all_stations.py"
OUT = os.path.join(HERE, "golden_raws_v1.npz")
HEADER = '''class InsertRaws(object):
    def __init__(self, path_stn_file, path_stnid_file, path_obs_files, min_ymd, max_ymd):
        self.path_stn_file, self.path_stnid_file, self.path_obs_files = path_stn_file, path_stnid_file, path_obs_files
        self.min_ymd, self.max_ymd, self.nskipped = min_ymd, max_ymd, 0

'''


def load_reference():
    import make_golden as mg
    if not hasattr(np, "int"):
        np.int = int
    parse = _edit(mg._slice(REL, 1193, 1233), '"Copyright" in line', 'b"Copyright" in line', 1)
    parse = _edit(parse, 'print "RAWS: Error in parsing a observation for", stn_id', "self.nskipped += 1", 1)
    src = (HEADER + "    def get_stns(self):\n" + _drop_prints(mg._slice(REL, 1143, 1175), 3) + "\n" + mg._slice(REL, 711, 715) +
           "\n    def parse_stn_obs(self, stn_id):\n" + parse)
    out = {}
    for tag, opener in (("text", lambda p, mode="r": io.open(p, mode, encoding="latin-1", newline="\n")),
                        ("bytes", lambda p: io.open(p, "rb"))):
        ns = dict(np=np, os=os, datetime=__import__("datetime"), long=int, MISSING=-9999., DTYPE_STNOBS=DTYPE_STNOBS, open=opener,
                  unicode=lambda s, errors=None: "".join(c for c in s if ord(c) < 128))
        exec(compile(src, "create_db_all_stations.py", "exec"), ns)
        out[tag] = ns["InsertRaws"]
    assign = _edit(textwrap.dedent(mg._slice(REL, 619, 623)), "# prcp_chk[time_idx,stn_cnt]", "prcp_chk[time_idx,stn_cnt]", 1)
    out["assign"] = compile(assign, "create_db_all_stations.py:619", "exec")
    return out


def run_file(ref, d, stn, data, min_ymd, max_ymd):
    """(obs, skipped) of the executed ``parse_stn_obs``; lets its exception through."""
    with open(os.path.join(d, stn + ".txt"), "wb") as fh:
        fh.write(data)
    ins = ref["bytes"](None, None, d, min_ymd, max_ymd)
    return ins.parse_stn_obs("RAWS_" + stn), ins.nskipped


def assign(ref, obs, days):
    n = days["YMD"].size
    loc = dict(np=np, days=days, YMD="YMD", obs=obs, stn_cnt=0, tmin_chk=np.ones((n, 1), np.float32) * -9999.0,
               tmax_chk=np.ones((n, 1), np.float32) * -9999.0, prcp_chk=np.ones((n, 1), np.float32) * -9999.0)
    exec(ref["assign"], loc)
    return np.stack([loc["tmin_chk"][:, 0], loc["tmax_chk"][:, 0], loc["prcp_chk"][:, 0]])


def raising_line(ref, d, stn, data, min_ymd, max_ymd, exc_type):
    """The 1-based line the reference raises on: the first n for which the file cut after line n raises."""
    lines = RR.lines_of(data)
    for n in range(1, len(lines) + 1):
        end = lines[n][0] if n < len(lines) else len(data)
        try:
            run_file(ref, d, stn, data[:end], min_ymd, max_ymd)
        except exc_type:
            return n
    raise AssertionError("%s raises as a whole and at no line" % stn)


def run_case(ref, case, tmp):
    days = days_of(case["min_ymd"], case["max_ymd"])
    n, nf = days["YMD"].size, len(case["files"])
    val = np.full((nf, 3, n), -9999.0, np.float32)
    raised, where = np.zeros(nf, "U16"), np.zeros(nf, np.int64)
    skipped, values = np.zeros(nf, np.int64), np.zeros(nf, np.int64)
    d = os.path.join(tmp, case["name"])
    os.makedirs(d)
    nbytes, secs = 0, 0.0
    for k, (stn, data) in enumerate(case["files"]):
        t0 = time.perf_counter()
        try:
            obs, skipped[k] = run_file(ref, d, stn, data, case["min_ymd"], case["max_ymd"])
        except (IndexError, ValueError) as exc:
            raised[k] = type(exc).__name__
            where[k] = raising_line(ref, d, stn, data, case["min_ymd"], case["max_ymd"], type(exc))
            continue
        if case["duplicates"]:
            try:
                assign(ref, obs, days)
            except ValueError:
                raised[k] = "assignment"
            continue
        val[k] = assign(ref, obs, days)
        values[k] = obs.size
        nbytes, secs = nbytes + len(data), secs + time.perf_counter() - t0
    return val, raised, where, skipped, values, nbytes, secs


def main():
    ref = load_reference()
    out = {"input_hash": np.array(RC.input_hash())}
    with tempfile.TemporaryDirectory() as tmp:
        for case in RC.scripted_cases():
            val, raised, where, skipped, values, _, _ = run_case(ref, case, tmp)
            if case["duplicates"]:
                assert (raised == "assignment").all(), (case["name"], raised)
                print("%-10s %3d files: the reference's assignment fails on each; not stored" % (case["name"], len(raised)))
                continue
            for k, (stn, data) in enumerate(case["files"]):           # the restatement must agree before anything is stored
                r = RR.parse_raws(data, case["min_ymd"], case["max_ymd"])
                assert (r["raised"] or ("", 0)) == (str(raised[k]), int(where[k])), (case["name"], stn, r["raised"], raised[k], where[k])
                if not raised[k]:
                    assert val[k].tobytes() == r["val"].tobytes(), (case["name"], stn)
                    assert (r["skipped"], r["values"], r["duplicates"]) == (skipped[k], values[k], 0), (case["name"], stn)
            for key, a in (("val", val), ("raised", raised), ("line", where), ("skipped", skipped), ("values", values)):
                out[case["name"] + "/" + key] = a
            print("%-10s %3d files, %3d raised (%s), %5d skipped, %6d values" % (
                case["name"], len(raised), (raised != "").sum(), ",".join(sorted(set(raised) - {""})), skipped.sum(), values.sum()))
        pool = RC.pool_case()
        val, raised, where, skipped, values, nbytes, secs = run_case(ref, pool, tmp)
        assert not (raised != "").any()
        for k, (stn, data) in enumerate(pool["files"]):
            r = RR.parse_raws(data, pool["min_ymd"], pool["max_ymd"])
            assert r["raised"] is None and val[k].tobytes() == r["val"].tobytes() and r["duplicates"] == 0, stn
        out["pool/sha"] = np.array([hashlib.sha256(np.ascontiguousarray(val[k]).tobytes()).hexdigest() for k in range(val.shape[0])])
        out["pool/values"], out["pool/skipped"] = values, skipped
        out["reference_mb_per_s"] = np.array(nbytes / secs / 1e6)
        print("pool: %d stations, %d values; reference %.2f MB/s on one core" % (val.shape[0], values.sum(), nbytes / secs / 1e6))
        # get_stns
        ids, meta, have = RC.station_files()
        for name, data in (("ids.txt", ids), ("meta.txt", meta)):
            with open(os.path.join(tmp, name), "wb") as fh:
                fh.write(data)
        obs = os.path.join(tmp, "have")
        os.makedirs(obs)
        for sid in have:
            open(os.path.join(obs, sid + ".txt"), "w").close()
        rows = ref["text"](os.path.join(tmp, "meta.txt"), os.path.join(tmp, "ids.txt"), obs, 0, 0).get_stns()
        rows = [rows[k] for k in np.argsort(np.array([r[0] for r in rows], dtype=object))]          # :502-509
        assert rows == RR.get_stns(ids, meta, have)[0], (rows, RR.get_stns(ids, meta, have)[0])
        out["stns/id"], out["stns/state"] = np.array([r[0] for r in rows]), np.array([r[4] for r in rows])
        out["stns/num"] = np.array([r[1:4] for r in rows], np.float64).reshape(len(rows), 3)
        out["stns/name"] = np.array([r[5] for r in rows])
        print("stns", [r[0] for r in rows])
        kid, kmeta = RC.station_files_keyerror()
        for name, data in (("kids.txt", kid), ("kmeta.txt", kmeta)):
            with open(os.path.join(tmp, name), "wb") as fh:
                fh.write(data)
        try:
            ref["text"](os.path.join(tmp, "kmeta.txt"), os.path.join(tmp, "kids.txt"), obs, 0, 0).get_stns()
            out["stns_keyerror"] = np.array("")
        except KeyError:
            out["stns_keyerror"] = np.array("KeyError")
        print("an id without a state:", out["stns_keyerror"])
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
