"""GPU: the RAWS ingest (``twxrw_parse`` of libtwxqa, ``topowx_amd.raws``, ``python -m topowx_amd.step04 --raws-*``) against
the executed-reference golden (tests/golden/make_golden_raws.py) and the restatement (tests/restate_raws.py).  Every
comparison is for equality -- values bit for bit, counts, both lists, exception type and line: nothing is computed but an
exact division, one multiplication and one rounding.  The cases with duplicate dates are pinned by the restatement alone."""
import hashlib
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib, ghcn, h5nc, ncio, raws, step04, step05
from topowx_amd.qa import qa_temp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ghcn_cases as GC  # noqa: E402
import raws_cases as RC  # noqa: E402
import restate_raws as RR  # noqa: E402

pytestmark = pytest.mark.gpu
EXC = dict(IndexError=IndexError, ValueError=ValueError)


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_raws_v1.npz"))
    assert str(g["input_hash"]) == RC.input_hash(), "case generator drifted: regenerate the golden"
    return g


@pytest.fixture(scope="module")
def scripted():
    return RC.scripted_cases()


@pytest.fixture(scope="module")
def pool():
    return RC.pool_case()


@pytest.fixture(scope="module")
def restated(scripted, pool):
    """The reference of every test, computed once: per case and file the restatement's result."""
    return {c["name"]: [RR.parse_raws(d, c["min_ymd"], c["max_ymd"]) for _, d in c["files"]] for c in scripted + [pool]}


def _buffer(files):
    off = np.zeros(len(files) + 1, np.int64)
    off[1:] = np.cumsum([len(d) for _, d in files])
    return b"".join(d for _, d in files), off


def _raw(case, files=None, **kw):
    files = case["files"] if files is None else files
    buf, off = _buffer(files)
    _, _, _, nd = ghcn._period(case["min_ymd"], case["max_ymd"])
    return raws.raws_parse(buf, off, case["min_ymd"], case["max_ymd"], nd, **kw)


def _view(case, files=None):
    """The restated device view of a batch: (uncertain, raise, counts summed)."""
    files = case["files"] if files is None else files
    _, off = _buffer(files)
    unc, rse, tot = [], [], dict.fromkeys(raws.RW_COUNTS, 0)
    for f, (_, data) in enumerate(files):
        u, r, c = RR.device_view(data, case["min_ymd"], case["max_ymd"], f=f, base=int(off[f]))
        unc, rse = unc + u, rse + r
        for k in tot:
            tot[k] += c[k]
    return unc, rse, tot


def _write(tmp, case):
    d = tmp / case["name"]
    d.mkdir()
    out = []
    for stn, data in case["files"]:
        (d / (stn + ".txt")).write_bytes(data)
        out.append(str(d / (stn + ".txt")))
    return out


def test_kernels_on_every_scripted_case(gold, scripted, restated):
    """The whole case in one buffer (the cut case ends the buffer inside a line at every length): the kernels' own outputs.
    Both lists and the eight counts: the restatement's, exactly, with capacities of 1 (the call is repeated) and with room.
    Two calls: the same bytes.  Files whose every line the device decides: the golden's arrays."""
    for case in scripted:
        val, win, unc, rse, counts = _raw(case, uncertain_cap=1, raise_cap=1)
        again = _raw(case, uncertain_cap=1 << 16, raise_cap=1 << 16)
        for a, b in zip((val, unc, rse, counts), again[:1] + again[2:]):
            assert a.tobytes() == b.tobytes(), case["name"]
        assert (win is None) == (again[1] is None) and (win is None or win.tobytes() == again[1].tobytes())
        want_u, want_r, want_c = _view(case)
        assert [tuple(e) for e in unc.tolist()] == want_u, case["name"]
        assert [tuple(e) for e in rse.tolist()] == want_r, case["name"]
        assert counts.tolist() == [want_c[k] for k in raws.RW_COUNTS], case["name"]
        assert (win is not None) == (want_c["date_uncertain"] > 0)
        _, off = _buffer(case["files"])
        for k, ((stn, data), r) in enumerate(zip(case["files"], restated[case["name"]])):
            u, rr, c = RR.device_view(data, case["min_ymd"], case["max_ymd"])
            if not u and not rr:
                assert val[:, k].tobytes() == r["val"].tobytes(), (case["name"], stn)
                if not case["duplicates"]:
                    assert val[:, k].tobytes() == np.ascontiguousarray(gold[case["name"] + "/val"][k]).tobytes(), (case["name"], stn)


def test_module_on_every_scripted_case(gold, scripted, restated, tmp_path):
    """``raws.parse_raws_files``: the page-locked buffer, the reader threads, the lines settled by ``int()`` / ``float()``.
    The files the reference parsed equal the golden everywhere; a file it raised on raises the same exception naming the
    file and the line; the first error of a batch is the first in station order."""
    for case in scripted:
        paths = _write(tmp_path, case)
        res = restated[case["name"]]
        keep = [k for k, r in enumerate(res) if r["raised"] is None]
        stats = {}
        val = raws.parse_raws_files([paths[k] for k in keep], case["min_ymd"], case["max_ymd"], stats=stats)
        for j, k in enumerate(keep):
            assert val[:, j].tobytes() == res[k]["val"].tobytes(), (case["name"], k)
            if not case["duplicates"]:
                assert val[:, j].tobytes() == np.ascontiguousarray(gold[case["name"] + "/val"][k]).tobytes(), (case["name"], k)
        for key in ("lines", "body", "skipped", "values", "duplicates"):
            assert stats[key] == sum(res[k][key] for k in keep), (case["name"], key)
        if not case["duplicates"]:
            assert stats["skipped"] == gold[case["name"] + "/skipped"][keep].sum()
            assert stats["values"] == gold[case["name"] + "/values"][keep].sum()
        assert stats["bytes"] == sum(len(case["files"][k][1]) for k in keep)
        bad = [k for k, r in enumerate(res) if r["raised"] is not None]
        for n, k in enumerate(bad):
            name, line = res[k]["raised"]
            assert case["duplicates"] or (str(gold[case["name"] + "/raised"][k]), int(gold[case["name"] + "/line"][k])) == (name, line)
            with pytest.raises(EXC[name], match=r"%s\.txt, line %d: " % (case["files"][k][0], line)):
                raws.parse_raws_files([paths[k]], case["min_ymd"], case["max_ymd"], pinned=bool(n % 2))
        if bad:
            name, line = res[bad[0]]["raised"]
            with pytest.raises(EXC[name], match=r"%s\.txt, line %d: " % (case["files"][bad[0]][0], line)):
                raws.parse_raws_files(paths, case["min_ymd"], case["max_ymd"])


def test_seeded_pool(gold, pool, restated, tmp_path):
    """Plain decimals only: the uncertain count must be exactly 0, so every value here is the device's."""
    paths = _write(tmp_path, pool)
    stats, tm = {}, {}
    val = raws.parse_raws_files(paths, pool["min_ymd"], pool["max_ymd"], stats=stats, timing=tm)
    assert stats["uncertain"] == 0 and stats["duplicates"] == 0
    assert [hashlib.sha256(val[:, k].tobytes()).hexdigest() for k in range(len(paths))] == [str(s) for s in gold["pool/sha"]]
    assert stats["values"] == int(gold["pool/values"].sum()) and stats["skipped"] == int(gold["pool/skipped"].sum())
    assert stats["lines"] == sum(r["lines"] for r in restated["pool"]) and stats["body"] == sum(r["body"] for r in restated["pool"])
    assert set(tm) == {k + "_kernel_ms" for k in raws.RW_KERNELS} and all(np.isfinite(v) and v >= 0 for v in tm.values()), tm
    _, _, unc, rse, counts = _raw(pool)
    assert len(unc) == 0 and len(rse) == 0 and counts[5] == 0 and counts[3] == stats["values"]


def test_a_batch_split_at_every_file_boundary(scripted, pool, tmp_path):
    """One batch against a batch per file and a few files per batch: the same bytes, the same counts."""
    for case in [c for c in scripted if c["name"] in ("dates", "space", "copyright", "long", "dups", "sizes")] + [pool]:
        paths = _write(tmp_path, case)
        keep = [p for p, (_, d) in zip(paths, case["files"]) if RR.parse_raws(d, case["min_ymd"], case["max_ymd"])["raised"] is None]
        s1, s2, s3 = {}, {}, {}
        one = raws.parse_raws_files(keep, case["min_ymd"], case["max_ymd"], stats=s1)
        each = raws.parse_raws_files(keep, case["min_ymd"], case["max_ymd"], batch_bytes=1, stats=s2)
        some = raws.parse_raws_files(keep, case["min_ymd"], case["max_ymd"], batch_bytes=150000, pinned=False, stats=s3)
        assert one.tobytes() == each.tobytes() == some.tobytes(), case["name"]
        for k in ("bytes", "lines", "body", "skipped", "values", "duplicates", "uncertain"):
            assert s1[k] == s2[k] == s3[k], (case["name"], k)


def test_step04_with_both_networks_then_step05(gold, pool, restated, tmp_path):
    """Generated files -> ``python -m topowx_amd.step04 --raws-*`` in both containers -> a database the readers open, that
    holds both networks' columns in id order -> ``step05`` runs on it.  Without the RAWS arguments the file is byte for
    byte ``ghcn.create_all_stations_db``'s."""
    ghcn_ids = ["USC00010008", "USW00094728", "CA001011500"]
    obs, robs = tmp_path / "ghcnd_all", tmp_path / "raws_obs"
    obs.mkdir(), robs.mkdir()
    r = np.random.RandomState(9)
    for s in ghcn_ids:
        lines = [GC.dly_line(s, y, m, el, [int(x) for x in r.randint(-200, 400, 31)])
                 for y in (2000, 2001, 2002) for m in range(1, 13) for el in ("TMAX", "TMIN", "PRCP")]
        (obs / (s + ".dly")).write_bytes(b"\n".join(lines) + b"\n")
    (tmp_path / "ghcnd-stations.txt").write_bytes(GC.stations_text())
    npool = 12
    ids = b"".join(b"nv" + s.encode() + b"\n" for s, _ in pool["files"][:npool + 1])
    meta = b"".join(("%s  a  b  %.2f  %.2f  %d  POOL SITE %d\n" % (s, 38 + 0.1 * k, 115 + 0.1 * k, 1500 + k, k)).encode()
                    for k, (s, _) in enumerate(pool["files"][:npool + 1]))
    (tmp_path / "raws_ids.txt").write_bytes(ids)
    (tmp_path / "raws_meta.txt").write_bytes(meta)
    for s, data in pool["files"][:npool]:                         # (the last station of the table has no listing)
        (robs / (s + ".txt")).write_bytes(data)
    base = ["--stations", str(tmp_path / "ghcnd-stations.txt"), "--dly-dir", str(obs), "--start", "20000101", "--end", "2002-12-31",
            "--check-obs-exist"]
    rargs = ["--raws-stations", str(tmp_path / "raws_meta.txt"), "--raws-ids", str(tmp_path / "raws_ids.txt"), "--raws-obs", str(robs)]
    for fmt in (["NETCDF4"] if h5nc.available() else []) + ["NETCDF3_64BIT"]:
        db = str(tmp_path / ("all_%s.nc" % fmt))
        assert step04.main(base + rargs + ["--out", db, "--format", fmt]) == 0
        stns, _, days, tmin = ncio.read_station_db_arrays(db, "tmin")
        want_ids = sorted("GHCN_" + s for s in ghcn_ids) + ["RAWS_" + s for s, _ in pool["files"][:npool]]
        assert list(stns["station_id"]) == want_ids and days.size == 1096 and ncio.file_format(db) == fmt
        assert stns["station_name"][3] == "POOL SITE 0" and stns["longitude"][4] == -115.1 and stns["state"][3] == "NV"
        with ncio.open_dataset(db, "r") as ds:
            cols = {n: ds.variables[n][:] for n in ghcn.ELEMENTS}
            flags = {n: qa_temp.read_qflags(ds.variables["qflag_" + n]) for n in ghcn.ELEMENTS}
        for k in range(npool):
            val = np.stack([cols[n][:, 3 + k] for n in ghcn.ELEMENTS]).astype(np.float32)
            assert hashlib.sha256(val.tobytes()).hexdigest() == str(gold["pool/sha"][k])
            assert val.tobytes() == restated["pool"][k]["val"].tobytes()
            assert all((flags[n][:, 3 + k] == b"").all() for n in ghcn.ELEMENTS)
        assert (cols["tmax"][:, :3] != -9999).all()
        assert step05.main(["--db", db, "--start", "20000101", "--end", "20021231"]) == 0
    # without the RAWS arguments: the file of ghcn.create_all_stations_db, byte for byte (the history attribute is the date)
    a, b = str(tmp_path / "cli.nc"), str(tmp_path / "api.nc")
    assert step04.main(base + ["--out", a, "--format", "NETCDF3_64BIT"]) == 0
    ghcn.create_all_stations_db(b, str(tmp_path / "ghcnd-stations.txt"), str(obs), 20000101, 20021231, check_obs_exist=True,
                                format="NETCDF3_64BIT")
    assert open(a, "rb").read() == open(b, "rb").read()
    # a RAWS line the reference raises on ends the command with 1
    (robs / (pool["files"][0][0] + ".txt")).write_bytes(RC.listing([RC.line(RC.date(3), ntok=5)]))
    assert step04.main(base + rargs + ["--out", str(tmp_path / "bad.nc")]) == 1
