"""The series coder on the GPU (topowx_amd/qa/twxsd_serdeflate.hip through topowx_amd/series_deflate.py): every case of
tests/series_deflate_cases.py against ``zlib.decompress`` (no restatement involved) and, byte for byte and count for count,
against tests/restate_series_deflate.py; determinism, the sentinel band behind ``out_cap``, the batches; and the station
databases of step04 / step16-17 / step18 written with ``deflate="gpu"`` against today's route.

Sizes (restated on the CPU, equal to the GPU's bytes; ``zlib.compress(shuffled, 4)`` is what the host route stores), 16 rows x
25 203 float32 of the seeded pools of series_deflate_cases.pool:

    pool                                    this coder    zlib level 4    ratio
    observations in tenths, with gaps         414 662         466 653     0.889
    raw series, long missing stretches        181 344         185 431     0.978
    unrounded model values                  1 254 499       1 253 037     1.001
"""
import datetime
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import restate_series_deflate as R  # noqa: E402
import series_deflate_cases as SC  # noqa: E402
from topowx_amd import ncio, series_deflate as SD  # noqa: E402

pytestmark = pytest.mark.gpu

POOL_TOTALS = {"tenths": 414662, "raw": 181344, "model": 1254499}      # the restatement's totals (see the module docstring)
BAND = 4096


@pytest.fixture(scope="module")
def results():
    """Every case once: the restatement and the GPU's call into a buffer with a sentinel band behind ``out_cap``."""
    out = []
    for case in SC.cases():
        rows = case["rows"]
        want = R.deflate_call(rows)
        cap = sum(len(s) for s in want["streams"])
        buf = np.full(cap + BAND, 0xA5, np.uint8)
        _, off, counts = SD.deflate_rows(rows, out=buf[:cap])
        out.append((case, want, buf, off, counts))
    return out


def test_offsets_bound_and_inflate(results):
    for case, want, buf, off, counts in results:
        rows = case["rows"]
        nrows, n = rows.shape
        es = rows.dtype.itemsize
        assert off[0] == 0 and (np.diff(off) > 0).all(), case["name"]
        assert (np.diff(off) <= SD.bound(n, es)).all(), case["name"]
        for r in range(nrows):
            stream = buf[off[r]:off[r + 1]].tobytes()
            assert zlib.decompress(stream) == SD.shuffled(rows[r]).tobytes(), (case["name"], r)
            assert np.array_equal(R.inflate_row(stream, rows.dtype, n).view(np.uint8), rows[r].view(np.uint8)), (case["name"], r)


def test_bytes_and_counts_equal_the_restatement(results):
    for case, want, buf, off, counts in results:
        SC.check(case, R, want)
        rows = case["rows"]
        assert [int(x) for x in np.diff(off)] == [len(s) for s in want["streams"]], case["name"]
        assert buf[:off[-1]].tobytes() == b"".join(want["streams"]), case["name"]
        assert counts.tolist() == [want["blocks"], want["stored"]] + want["halvings"] + [rows.nbytes, int(off[-1])], case["name"]
        assert (buf[off[-1]:] == 0xA5).all(), case["name"]                      # the band behind out_cap
    assert any(c["halvings0"] for c in (dict(zip(SD.SD_COUNTS, r[4])) for r in results))


def test_second_call_is_identical_and_a_short_buffer_is_refused(results):
    for case, want, buf, off, counts in results:
        rows = case["rows"]
        again = np.full(buf.size, 0x5A, np.uint8)
        _, off2, counts2 = SD.deflate_rows(rows, out=again[:buf.size - BAND])
        assert np.array_equal(off, off2) and np.array_equal(counts, counts2), case["name"]
        assert again[:off[-1]].tobytes() == buf[:off[-1]].tobytes() and (again[off[-1]:] == 0x5A).all(), case["name"]
        short = np.full(buf.size, 0x3C, np.uint8)
        with pytest.raises(SD.SeriesDeflateCap, match="need %d bytes" % off[-1]) as exc:
            SD.deflate_rows(rows, out=short[:int(off[-1]) - 1])
        assert exc.value.needed == off[-1] and (short == 0x3C).all(), case["name"]


def test_batches_have_a_code_each():
    """A code per call: rows deflated in 1, 2 and 7 batches equal the restatement's calls over the same batches, row by row
    (and differ between the splits where the codes do)."""
    rows = SC.tenths(np.random.default_rng(5), 14, 4099)
    seen = set()
    for nb in (1, 2, 7):
        per = 14 // nb
        t = {}
        packed, off = SD.deflate_series(rows, batch_bytes=per * rows.shape[1] * 4, timing=t)
        want = R.deflate_batched(rows, per)
        assert t["sd_batches"] == nb and t["sd_bytes_in"] == rows.nbytes and t["sd_bytes_out"] == off[-1]
        assert [packed[off[r]:off[r + 1]].tobytes() for r in range(14)] == want
        seen.add(packed.tobytes())
    assert len(seen) == 3
    empty, off = SD.deflate_series(np.zeros((0, 5), np.float32))
    assert empty.size == 0 and off.tolist() == [0]


def test_pool_sizes():
    """The drift guard of the sizes in the module docstring: the GPU's total is the restatement's, at most the recorded
    total x 1.02, and no stream exceeds ``twxsd_bound``."""
    for kind, total in POOL_TOTALS.items():
        rows = SC.pool(kind)
        packed, off = SD.deflate_series(rows)
        assert int(off[-1]) == sum(len(s) for s in R.deflate_call(rows)["streams"]), kind
        assert off[-1] <= total * 1.02, (kind, int(off[-1]))
        assert (np.diff(off) <= SD.bound(rows.shape[1], 4)).all()


# ---- through files: 40 stations x 3 653 days ----------------------------------------------------------------------------------
NSTN, D0, D1 = 40, datetime.date(1948, 1, 1), datetime.date(1957, 12, 31)


def _days():
    from topowx_amd.dates import get_days_metadata
    days = get_days_metadata(D0, D1)
    assert days.size == 3653
    return days


def _describe(path):
    """Everything ``ncio`` / ``h5nc`` report of a file: dimensions, global attributes (the ``history`` date aside), and per
    variable dtype, dimensions, attributes, chunk shape, filter list and the values' bytes."""
    ds = ncio.open_dataset(path, "r")
    try:
        out = {"/dims": {k: int(v) for k, v in ds.dimensions.items()},
               "/attrs": {k: str(ds.getncattr(k)) for k in ds.ncattrs() if k != "history"}}
        for name, v in ds.variables.items():
            a = np.asarray(v[:])
            out[name] = dict(dtype=str(v.dtype), dims=tuple(v.dimensions), chunks=v.chunking(), filters=v.filters(),
                             attrs={k: repr(v.getncattr(k)) for k in v.ncattrs()},
                             values=[str(x) for x in a.ravel()] if a.dtype == object else a.tobytes())
    finally:
        ds.close()
    return out


def _peer_describe(path):
    import test_h5py_interop as HI
    if HI.PY is None:
        return None
    d = HI.peer("describe", path)
    d["/attrs"].pop("history", None)
    return d


def _chunks_are_the_streams(path, names, batch_rows=None):
    """``chunk_info``: every (0, j) chunk with filter mask 0 and the size of the stream the coder gives for its row."""
    ds = ncio.open_dataset(path, "r")
    try:
        for name in names:
            v = ds.variables[name]
            rows = np.ascontiguousarray(np.asarray(v[:]).T)
            rows = rows.view(np.uint8) if rows.dtype.kind == "S" else rows
            kw = {} if batch_rows is None else dict(batch_bytes=batch_rows * rows.shape[1] * rows.dtype.itemsize)
            _, off = SD.deflate_series(rows, **kw)
            info = v.chunk_info()
            assert sorted(info) == [(0, j) for j in range(rows.shape[0])], name
            assert [info[(0, j)][1:] for j in range(rows.shape[0])] == [(int(s), 0) for s in np.diff(off)], name
    finally:
        ds.close()


def _same(paths, filters=True):
    d = [_describe(p) for p in paths]
    for other in d[1:]:
        assert sorted(other) == sorted(d[0])
        for k in d[0]:
            a, b = d[0][k], other[k]
            if not filters and isinstance(a, dict) and "filters" in a:
                a, b = dict(a, filters=None), dict(b, filters=None)
            assert a == b, k
    if filters:
        p = [_peer_describe(x) for x in paths]
        assert all(x == p[0] for x in p[1:])


def _report(seed):
    rng = np.random.default_rng(seed)
    ids = np.array(["G%03d" % i for i in range(NSTN)])
    fnl = SC.tenths(rng, NSTN, 3653, gaps=False).astype(np.float64)
    model = SC.model(rng, NSTN, 3653).astype(np.float64)
    mask = rng.random((NSTN, 3653)) < 0.3
    mask[3, 100:2500] = True                                 # a run beyond five years: "all model"
    fnl[mask] = model[mask]
    fnl[5, 10:20] = np.nan
    return dict(ids=ids, fnl_tair=fnl, infill_tair=model, mask_infill=mask, mae=rng.random(NSTN), bias=rng.random(NSTN) - 0.5)


def _stns(ids):
    from topowx_amd import stationdb as sdb
    stns = np.empty(len(ids), dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = ids, -110.0, 45.0, 100.0
    return stns


def test_infill_and_serial_databases_through_the_gpu_route(tmp_path, capsys):
    from topowx_amd.infill import create_serially_complete_db, write_infill_db
    rep, days = _report(11), _days()
    stns = _stns(rep["ids"])
    p = {k: str(tmp_path / ("infill_%s.nc" % k)) for k in ("gpu", "host", "none", "none2")}
    for k, path in p.items():
        write_infill_db(path, stns, days, "tmin", rep, deflate=None if k.startswith("none") else k)
    _same([p["gpu"], p["host"], p["none"]])
    _chunks_are_the_streams(p["gpu"], ("tmin", "tmin_infilled", "flag_infilled"))
    assert open(p["none"], "rb").read() == open(p["none2"], "rb").read()          # the default route, written twice
    s = {k: str(tmp_path / ("serial_%s.nc" % k)) for k in p}
    recs = {k: create_serially_complete_db(p["none"], "tmin", path, deflate=None if k.startswith("none") else k) for k, path in s.items()}
    capsys.readouterr()
    assert recs["gpu"].all_infill[3] and all(np.array_equal(r.max_run, recs["none"].max_run) for r in recs.values())
    _same([s["gpu"], s["host"], s["none"]])
    _chunks_are_the_streams(s["gpu"], ("tmin", "flag_infilled"))
    assert open(s["none"], "rb").read() == open(s["none2"], "rb").read()
    assert os.path.getsize(s["gpu"]) < 1.1 * os.path.getsize(s["none"])


def test_step04_through_the_gpu_route(tmp_path, capsys):
    import ghcn_cases as GC
    from topowx_amd import step04
    r = np.random.RandomState(4)
    ids = ["USC%08d" % (200000 + k) for k in range(NSTN)]
    dly = tmp_path / "dly"
    dly.mkdir()
    (tmp_path / "ghcnd-stations.txt").write_bytes(GC.stations_text(ids))
    by_year = tmp_path / "by_year"
    by_year.mkdir()
    tob = {y: [] for y in range(D0.year, D1.year + 1)}
    for s, stn in enumerate(ids):
        lines = []
        for y in range(D0.year, D1.year + 1):
            for m in range(1, 13):
                for el in ("TMAX", "TMIN", "PRCP"):
                    if r.rand() < 0.1:
                        continue
                    v = r.randint(0, 2500, 31) if el == "PRCP" else r.randint(-450, 480, 31)
                    v[r.rand(31) < 0.08] = -9999
                    q = [bytes([c]) for c in r.choice(np.frombuffer(b"         DGIKX", np.uint8), 31)]
                    lines.append(GC.dly_line(stn, y, m, el, [int(x) for x in v], q))
                if s % 2 == 0:
                    for day in range(1, 29):
                        tob[y].append(("%s,%04d%02d%02d,TMAX,%5d,,,0,%s\n" % (stn, y, m, day, 100, ("0700", "1800")[(s // 2 + y) % 2])).encode())
        (dly / (stn + ".dly")).write_bytes(b"\n".join(lines) + b"\n")
    for y, lines in tob.items():
        (by_year / ("%d.csv" % y)).write_bytes(b"".join(lines))
    p = {k: str(tmp_path / ("all_%s.nc" % k)) for k in ("gpu", "host", "none", "none2")}
    for k, path in p.items():
        argv = ["--stations", str(tmp_path / "ghcnd-stations.txt"), "--dly-dir", str(dly), "--out", path, "--start", "19480101",
                "--end", "19571231", "--by-year", str(by_year), "--check-obs-exist"]
        assert step04.main(argv + ([] if k.startswith("none") else ["--deflate", k])) == 0
    capsys.readouterr()
    names = ("tmin", "tmax", "prcp", "qflag_tmin", "qflag_tmax", "qflag_prcp", "tobs_tmax")
    _same([p["gpu"], p["host"]])
    _same([p["gpu"], p["none"]], filters=False)                              # today's route: the same values, not compressed
    ds = ncio.open_dataset(p["gpu"], "r")
    try:
        assert int(ds.dimensions["station_id"]) == NSTN and int(ds.dimensions["time"]) == 3653
        for name in names:
            v = ds.variables[name]
            assert v.chunking() == [3653, 1] and v.filters()["zlib"] and v.filters()["shuffle"] == (v.dtype.itemsize > 1), name
        assert (np.asarray(ds.variables["tobs_tmax"][:]) > 0).any() and (np.asarray(ds.variables["tmin"][:]) != -9999).any()
    finally:
        ds.close()
    _chunks_are_the_streams(p["gpu"], names)
    assert open(p["none"], "rb").read() == open(p["none2"], "rb").read()          # the default route, written twice
    assert os.path.getsize(p["gpu"]) < 0.7 * os.path.getsize(p["none"])
