"""GHCN-Daily ingest (the reference's step04): the all-stations database from the files NOAA publishes.

``InsertGhcn`` / ``create_netcdf_db`` / ``insert_data_netcdf_db`` (twx/db/create_db_all_stations.py:320-660, 936-1103) and
``create_tobs_file`` / ``create_tobs_db`` (twx/homog/tobs.py:35-157).  The text is parsed on the GPU (``twxgh_parse_dly`` /
``twxgh_parse_tobs``, a lane per day field, integers only); the host reads the files of a batch into one page-locked
buffer on a thread pool and settles what only Python can: a value field that is not ``[+-]?[0-9]+`` goes through
``float()`` exactly as the reference's would, a header ``int()`` refuses raises ``ValueError`` naming the file and line.

The RAWS sites, which ``read_ghcn_stations`` drops as the reference does, come from their native source: ``raws.py``
(``InsertRaws``), through ``create_all_stations_db(..., raws=...)``.

Out of scope: ``InsertSnotel`` (it reads files "cleaned and formatted using the snotel_clean module", which the reference
does not contain, and parses them with ``pandas.read_csv``, whose number parser is not ``float()``), ``obsio``, and
downloading anything.

Deflate of the station variables is opt-in.  By default they are not compressed (``zlib=False``: a station's kernel row IS
a NetCDF-4 chunk and is written as one).  With ``deflate="gpu"`` the seven ``(time, station_id)`` variables are created
with ``zlib=True`` as the reference creates them, and every batch's kernel rows are shuffled and deflated on the GPU
(``series_deflate``, ``ncio.write_series_chunks``); ``deflate="host"`` leaves that to libhdf5.
"""
import datetime as _dt
import gzip
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _qalib, ncio
from . import stationdb as sdb
from .dates import get_days_metadata

__all__ = ["read_ghcn_stations", "parse_dly_files", "iter_dly_batches", "parse_tobs_files", "create_all_stations_db", "write_all_stations_db",
           "create_tobs_db", "ELEMENTS", "MISSING", "MAX_READERS"]

ELEMENTS = ("tmin", "tmax", "prcp")                # the kernel's element order: TMIN, TMAX, PRCP
MISSING = -9999.0                                  # create_db_all_stations.py:46
VALID_FIPS_CODES = ("US", "CA", "MX")              # :943-946
RM_STATES = ("HI", "AK")
RM_NETWORK_CODES = ("S", "R")
MAX_READERS = 16                                   # host threads that read / gunzip; never sized from os.cpu_count()
BATCH_BYTES = 256 << 20
MAX_BATCH_CELLS = 1 << 28                          # 3 x rows x days of one call: 9 bytes a cell on the device
STN_DTYPE = [(sdb.STN_ID, "U16"), (sdb.LAT, np.float64), (sdb.LON, np.float64), (sdb.ELEV, np.float64), ("state", "U2"),
             ("station_name", "U30")]
_WS = b" \t\n\r\x0b\x0c"


def _ymd(x):
    """yyyymmdd (int or str), yyyy-mm-dd or a date -> (int yyyymmdd, date); ValueError if it is no calendar day."""
    if isinstance(x, (_dt.date, _dt.datetime)):
        d = x.date() if isinstance(x, _dt.datetime) else x
    else:
        s = str(x).replace("-", "")
        if not re.match(r"\d{8}\Z", s):
            raise ValueError("not a date (yyyymmdd): %r" % (x,))
        d = _dt.date(int(s[:4]), int(s[4:6]), int(s[6:]))
    return d.year * 10000 + d.month * 100 + d.day, d


def _period(start, end):
    a, d0 = _ymd(start)
    b, d1 = _ymd(end)
    if d1 < d0:
        raise ValueError("the period ends (%d) before it starts (%d)" % (b, a))
    return a, b, d0, (d1 - d0).days + 1


def read_ghcn_stations(path_stn_file, path_obs_files=None, check_obs_exist=False):
    """``InsertGhcn.get_stns`` (:978-1026) on ghcnd-stations.txt: the US / CA / MX stations outside HI and AK that are not
    SNOTEL or RAWS sites, ids prefixed ``GHCN_``, sorted as ``insert_data_netcdf_db`` sorts them (:509).  With
    ``check_obs_exist`` only the stations with a ``.dly`` file under ``path_obs_files``.  The name is ASCII, other bytes
    dropped.  Returns a record array (station_id, latitude, longitude, elevation, state, station_name)."""
    if check_obs_exist and path_obs_files is None:
        raise ValueError("check_obs_exist needs path_obs_files")
    rows = []
    with open(path_stn_file, "rb") as fh:
        for raw in fh.read().split(b"\n"):
            line = raw.decode("latin-1")
            if line[0:2] not in VALID_FIPS_CODES:
                continue
            orig = line[0:11].strip()
            state = line[38:40].strip().upper()
            if state in RM_STATES or orig[2] in RM_NETWORK_CODES:
                continue
            if check_obs_exist and not os.path.exists(os.path.join(path_obs_files, orig + ".dly")):
                continue
            name = line[41:71].strip().encode("ascii", "ignore").decode()
            rows.append(("GHCN_" + orig, float(line[12:20]), float(line[21:30]), float(line[31:37]), state, name))
    rows.sort(key=lambda r: r[0])
    return np.array(rows, dtype=STN_DTYPE)


# ---- reading a batch of files into one buffer ----------------------------------------------------------------------
class _HostBuffer(object):
    """Ordinary host memory behind the interface of ``_qalib.PinnedBuffer``."""

    def __init__(self, nbytes):
        self._a = bytearray(max(int(nbytes), 1))
        self.view = memoryview(self._a)

    def close(self):
        self.view.release()


def _read_into(path, view):
    with open(path, "rb", buffering=0) as fh:
        got = 0
        while got < len(view):
            n = fh.readinto(view[got:])
            if not n:
                raise IOError("%s shrank while it was read" % path)
            got += n


def _batches(sizes, batch_bytes, max_files=None):
    """Consecutive runs of files of at most ``batch_bytes`` (a larger single file is a batch of its own) and at most
    ``max_files`` files (what bounds the call's output rows)."""
    out, i0, tot = [], 0, 0
    for i, s in enumerate(sizes):
        if s > _qalib.GH_MAX_BYTES:
            raise ValueError("file %d holds %d bytes; a call takes at most %d" % (i, s, _qalib.GH_MAX_BYTES))
        if i > i0 and (tot + s > batch_bytes or (max_files is not None and i - i0 >= max_files)):
            out.append((i0, i))
            i0, tot = i, 0
        tot += s
    if len(sizes) > i0:
        out.append((i0, len(sizes)))
    return out


def _dly_paths(stn_ids, path_obs_files):
    paths = []
    for s in stn_ids:
        s = str(s)
        p = os.path.join(path_obs_files, (s[5:] if s.startswith("GHCN_") else s) + ".dly")
        if not os.path.isfile(p):
            raise IOError("station %s: no observation file %s" % (s, p))
        paths.append(p)
    return paths


# ---- what only Python decides ------------------------------------------------------------------------------------------
def _convert(e, v):
    if v == MISSING:
        return v
    return v / 100.0 if e == 2 else v / 10.0


def _line_number(data, pos):
    return bytes(data[:pos]).count(b"\n") + 1


def _parse_dly_python(data, path, min_ymd, max_ymd, d0, ndays):
    """``parse_stn_obs`` line by line in Python: the route of a file with a header the kernel does not take as a number.
    Raises the reference's ``ValueError`` (naming file and line) if ``int()`` refuses it."""
    val = np.full((3, ndays), MISSING, np.float32)
    flag = np.zeros((3, ndays), np.uint8)
    nvalues, pos, data = 0, 0, bytes(data)
    names = (b"TMIN", b"TMAX", b"PRCP")
    while pos < len(data):
        end = data.find(b"\n", pos) + 1 or len(data)
        line = data[pos:end]
        try:
            year, month = int(line[11:15]), int(line[15:17])
        except ValueError as exc:
            raise ValueError("%s, line %d: %s" % (path, _line_number(data, pos), exc))
        pos = end
        el = line[17:21].strip(_WS)
        if el not in names:
            continue
        e = names.index(el)
        for day in range(1, 32):
            try:
                k = (_dt.date(year, month, day) - d0).days
            except ValueError:
                continue
            if not (min_ymd <= year * 10000 + month * 100 + day <= max_ymd):
                continue
            off = 21 + 8 * (day - 1)
            try:
                v = float(line[off:off + 5])
            except ValueError:
                continue
            q = line[off + 6:off + 7].strip(_WS)
            val[e, k] = _convert(e, v)
            flag[e, k] = q[0] if q else 0
            nvalues += 1
    return val, flag, nvalues


def _settle_dly(view, off, paths, val, flag, bad, fb, min_ymd, max_ymd, d0, ndays):
    """Apply the Python-side decisions to the rows of one batch; returns the values they added."""
    added = 0
    redone = set()
    for f in np.nonzero(bad != _qalib.GH_NO_BAD_HEADER)[0]:
        v, q, n = _parse_dly_python(view[off[f]:off[f + 1]], paths[f], min_ymd, max_ymd, d0, ndays)
        val[:, f], flag[:, f] = v, q
        redone.add(int(f))
    for f, pos, length, d, e, win, k, start in fb.tolist():             # in buffer order: a later line overrides an earlier
        if f in redone:
            continue
        a = off[f] + pos
        text = bytes(view[a + 21 + 8 * d:a + min(26 + 8 * d, length)])
        try:
            v = float(text)
        except ValueError:
            continue
        added += 1
        if start + 1 > win:
            q = bytes(view[a + 27 + 8 * d:a + min(28 + 8 * d, length)]).strip(_WS)
            val[e, f, k] = _convert(e, v)
            flag[e, f, k] = q[0] if q else 0
    return added


def iter_dly_batches(paths, start, end, batch_bytes=BATCH_BYTES, device=0, timing=None, pinned=True, stats=None):
    """Parse the ``.dly`` files ``paths`` over the period, a batch of at most ``batch_bytes`` per device call.  Yields ``(i0,
    i1, val [3, i1 - i0, ndays] float32, flag [3, i1 - i0, ndays] uint8)``: station-major rows of files i0 .. i1 - 1,
    ``MISSING`` / 0 where the file gives nothing.  ``stats`` (a dict) receives ``bytes``, ``lines``, ``values``,
    ``fallback``, ``read_s``, ``parse_s``; ``timing`` the kernel milliseconds."""
    import time
    min_ymd, max_ymd, d0, ndays = _period(start, end)
    if int(batch_bytes) < 1:
        raise ValueError("batch_bytes must be positive")
    sizes = [os.path.getsize(p) for p in paths]
    runs = _batches(sizes, int(batch_bytes), max(1, MAX_BATCH_CELLS // (3 * ndays)))
    st = stats if stats is not None else {}
    for k in ("bytes", "lines", "values", "fallback"):
        st.setdefault(k, 0)
    st.setdefault("read_s", 0.0), st.setdefault("parse_s", 0.0)
    if not runs:
        return
    cap = max(sum(sizes[a:b]) for a, b in runs)
    buf = (_qalib.PinnedBuffer if pinned else _HostBuffer)(max(cap, 1))
    try:
        with ThreadPoolExecutor(max_workers=MAX_READERS) as pool:
            for i0, i1 in runs:
                t0 = time.perf_counter()
                off = np.zeros(i1 - i0 + 1, np.int64)
                off[1:] = np.cumsum(sizes[i0:i1])
                list(pool.map(lambda j: _read_into(paths[i0 + j], buf.view[off[j]:off[j + 1]]), range(i1 - i0)))
                t1 = time.perf_counter()
                val, flag, bad, fb, counts = _qalib.ghcn_parse_dly(buf.view, off, np.arange(i1 - i0, dtype=np.int32), i1 - i0,
                                                                   min_ymd, max_ymd, ndays, device=device, timing=timing)
                added = _settle_dly(buf.view, off, paths[i0:i1], val, flag, bad, fb, min_ymd, max_ymd, d0, ndays)
                t2 = time.perf_counter()
                st["bytes"] += int(off[-1])
                st["lines"] += int(counts[0])
                st["values"] += int(counts[1]) + added
                st["fallback"] += int(counts[2])
                st["read_s"] += t1 - t0
                st["parse_s"] += t2 - t1
                yield i0, i1, val, flag
    finally:
        buf.close()


def parse_dly_files(paths, start, end, **kw):
    """All of ``iter_dly_batches`` at once: ``(val [3, nfiles, ndays] float32, flag [3, nfiles, ndays] uint8)``."""
    _, _, _, ndays = _period(start, end)
    val = np.full((3, len(paths), ndays), MISSING, np.float32)
    flag = np.zeros((3, len(paths), ndays), np.uint8)
    for i0, i1, v, q in iter_dly_batches(paths, start, end, **kw):
        val[:, i0:i1], flag[:, i0:i1] = v, q
    return val, flag


# ---- times of observation --------------------------------------------------------------------------------------------
def _read_maybe_gz(path):
    if path.endswith(".gz"):
        with gzip.open(path, "rb") as fh:
            return fh.read()
    with open(path, "rb") as fh:
        return fh.read()


def _by_year_files(path_ghcn_yrly, years):
    out = []
    for y in years:
        for name in ("%d.csv.gz" % y, "%d.csv" % y):
            p = os.path.join(path_ghcn_yrly, name)
            if os.path.isfile(p):
                out.append((y, p))
                break
        else:
            raise IOError("no by-year file %d.csv.gz (or %d.csv) in %s" % (y, y, path_ghcn_yrly))
    return out


def _pieces(data, limit):
    """``data`` cut after newlines into pieces of at most ``limit`` bytes."""
    out, a = [], 0
    while len(data) - a > limit:
        b = data.rfind(b"\n", a, a + limit) + 1
        if b <= a:
            raise ValueError("a line longer than %d bytes" % limit)
        out.append(data[a:b])
        a = b
    out.append(data[a:] if a else data)
    return out


def _tobs_python(data, name, idx, element, min_ymd, max_ymd, d0, tobs):
    """``create_tobs_db``'s loop in Python over one piece: the route of a piece with a line the kernel does not take."""
    el, pos = element.encode(), 0
    while pos < len(data):
        end = data.find(b"\n", pos) + 1 or len(data)
        body = data[pos:end].rstrip(b"\n")
        at = pos
        pos = end
        if len(body) < 25 or body[21:25] != el or body[:2] not in (b"US", b"CA", b"MX"):
            continue
        if not body[-1:].isdigit() or body.endswith(b"2400") or body[:11] not in idx:
            continue
        try:
            ymd = int(body[12:20])
            try:
                k = (_dt.date(ymd // 10000, ymd // 100 % 100, ymd % 100) - d0).days if min_ymd <= ymd <= max_ymd else -1
            except ValueError:
                k = -1
            if k < 0:
                continue
            v = int(body[-4:] + b"\n")
            if abs(v) > 32767:
                raise ValueError("%d does not fit int16" % v)
        except ValueError as exc:
            raise ValueError("%s, line %d: %s" % (name, _line_number(data, at), exc))
        tobs[idx[body[:11]], k] = v


def parse_tobs_files(files, stn_ids, start, end, element="TMAX", piece_bytes=1 << 30, device=0, timing=None, stats=None):
    """``create_tobs_file`` + ``create_tobs_db``: the times of observation of ``element`` of the stations ``stn_ids``
    (sorted, with or without ``GHCN_``) from the by-year files ``files`` = [(year or None, path)], in that order.  Returns
    tobs [nstn, ndays] int16, -1 = none.  A piece whose dates stay inside its file's year is parsed into that year's window
    only.  One deviation from the reference: a date that is no day of the period is skipped and counted
    (``stats['outside']``) where the reference dies with ``IndexError``."""
    min_ymd, max_ymd, d0, ndays = _period(start, end)
    ids = np.array([s[5:] if str(s).startswith("GHCN_") else str(s) for s in stn_ids])
    if ids.size < 1 or any(len(s) > 11 for s in ids) or np.any(ids[1:] <= ids[:-1]):
        raise ValueError("stn_ids must be sorted, distinct ids of at most 11 characters")
    if len(str(element)) != 4:
        raise ValueError("the element is four characters")
    ids11 = ids.astype("S11")
    idx = {bytes(s): k for k, s in enumerate(ids11)}
    full = np.full((ids.size, ndays), -1, np.int16)
    st = stats if stats is not None else {}
    for k in ("bytes", "lines", "values", "outside"):
        st.setdefault(k, 0)
    files = list(files)
    with ThreadPoolExecutor(max_workers=MAX_READERS) as pool:
        for (year, path), data in zip(files, pool.map(lambda f: _read_maybe_gz(f[1]), files)):
            w0, nwin = 0, ndays
            if year is not None:
                a = max(d0, _dt.date(int(year), 1, 1))
                b = min(d0 + _dt.timedelta(ndays - 1), _dt.date(int(year), 12, 31))
                if a <= b:
                    w0, nwin = (a - d0).days, (b - a).days + 1
            for piece in _pieces(data, min(int(piece_bytes), _qalib.GH_MAX_BYTES)):
                off = np.array([0, len(piece)], np.int64)
                win = np.ascontiguousarray(full[:, w0:w0 + nwin])
                bad, counts = _qalib.ghcn_parse_tobs(piece, off, ids11, element, min_ymd, max_ymd, w0, win, device=device,
                                                     timing=timing)
                if counts[3] > 0:
                    _tobs_python(piece, path, idx, str(element), min_ymd, max_ymd, d0, full)
                elif counts[2] > 0:                                    # a date of another year: the whole period's window
                    bad, counts = _qalib.ghcn_parse_tobs(piece, off, ids11, element, min_ymd, max_ymd, 0, full, device=device,
                                                         timing=timing)
                else:
                    full[:, w0:w0 + nwin] = win
                st["bytes"] += len(piece)
                st["lines"] += int(counts[4])
                st["values"] += int(counts[0])
                st["outside"] += int(counts[1])
    return full


# ---- the databases -------------------------------------------------------------------------------------------------------
_VARS = (("tmin", "f4", MISSING, "minimum air temperature", "C", "minimum_air_temperature"),
         ("tmax", "f4", MISSING, "maximum air temperature", "C", "maximum_air_temperature"),
         ("prcp", "f4", MISSING, "precipitation amount", "cm", "precipitation_amount"),
         ("qflag_tmin", "S1", "", "quality assurance flag tmin", None, "quality assurance flag tmin"),
         ("qflag_tmax", "S1", "", "quality assurance flag tmax", None, "quality assurance flag tmax"),
         ("qflag_prcp", "S1", "", "quality assurance flag prcp", None, "quality assurance flag prcp"))


def _create_db(path, stns, days, format, with_tobs, zlib=False):
    """``create_netcdf_db`` (:320-456) plus ``prcp`` / ``qflag_prcp`` (parsed and left out of the file by the reference) and,
    on request, ``tobs_tmax``: dimensions ``time`` and ``station_id``, chunks ``(ndays, 1)``, compressed only with ``zlib``."""
    ds = ncio.open_dataset(path, "w", format)
    ds.title = "Weather Station Database"
    ds.institution = "University of Montana Numerical Terradynamics Simulation Group"
    ds.history = "Created on: " + _dt.date.today().strftime("%Y-%m-%d")
    n, nd = int(stns.size), int(days.size)
    ds.createDimension("time", nd)
    ds.createDimension(sdb.STN_ID, n)
    tv = ds.createVariable("time", "f8", ("time",))
    tv.long_name, tv.units, tv.standard_name, tv.calendar = "time", ncio._units(ncio._date(days, 0)), "time", "standard"
    tv[:] = np.arange(nd, dtype=np.float64)
    v = ncio._write_ids(ds, sdb.STN_ID, sdb.STN_ID, stns[sdb.STN_ID])
    v.long_name = v.standard_name = "station id"
    for name, std in (("station_name", "name"), ("state", "state")):
        if ncio._is_nc4(ds):
            v = ncio._write_ids(ds, sdb.STN_ID, name, stns[name])
        else:                                                      # char arrays; a string<N> dimension may exist already
            width = max([1] + [len(s) for s in stns[name]])
            if "string%d" % width not in ds.dimensions:
                ds.createDimension("string%d" % width, width)
            v = ds.createVariable(name, "S1", (sdb.STN_ID, "string%d" % width))
            v[:] = np.array([list(s.ljust(width, "\0")) for s in stns[name]], "S1").reshape(n, width)
        v.long_name, v.standard_name = name.replace("_", " "), std
    for name, units in ((sdb.LAT, "degrees_north"), (sdb.LON, "degrees_east"), (sdb.ELEV, "m")):
        v = ds.createVariable(name, "f8", (sdb.STN_ID,), fill_value=MISSING)
        v.long_name, v.units, v.standard_name = name, units, name
        v[:] = stns[name]
    kw = dict(chunksizes=(nd, 1), zlib=bool(zlib)) if ncio._is_nc4(ds) and n else {}
    for name, dtype, fill, long_name, units, std in _VARS:
        v = ds.createVariable(name, dtype, ("time", sdb.STN_ID), fill_value=fill, **kw)
        v.long_name, v.standard_name = long_name, std
        if units:
            v.units, v.missing_value = units, np.float32(fill)
    if with_tobs:
        v = ds.createVariable("tobs_tmax", "i2", ("time", sdb.STN_ID), fill_value=np.int16(-1), **kw)
        v.long_name, v.missing_value = "time-of-observation", np.int16(-1)
    return ds


def write_all_stations_db(path, stns, days, batches, tobs=None, format=None, deflate=None, device=0, timing=None):
    """Write the database: ``batches`` yields ``(i0, i1, val [3, i1 - i0, ndays], flag [3, i1 - i0, ndays])`` station-major
    rows of the stations i0 .. i1 - 1 of ``stns`` (``iter_dly_batches``); ``tobs`` [nstn, ndays] int16 (or a callable that
    returns it, called after the observations are in) becomes ``tobs_tmax``.  In NetCDF-4 a station's row is written as
    the chunk it is (``write_chunk_raw``, no transpose); the classic container is filled from transposed arrays.
    ``deflate`` = ``"gpu"`` / ``"host"``: the variables are created with ``zlib=True`` and every batch goes through
    ``ncio.write_series_chunks``; ``None``: not compressed, the file as it always was."""
    if deflate not in (None, "gpu", "host"):
        raise ValueError("deflate must be None, 'gpu' or 'host', not %r" % (deflate,))
    n, ndays = int(stns.size), int(days.size)
    ds = _create_db(path, stns, days, format, tobs is not None, zlib=deflate is not None)
    try:
        raw = ncio._is_nc4(ds)
        packed = raw and deflate is not None and n > 0
        hold = None if raw else {name: (np.full((ndays, n), MISSING, "f4") if k < 3 else np.zeros((ndays, n), "S1"))
                                 for k, (name, *_) in enumerate(_VARS)}
        for i0, i1, val, flag in batches:
            val, flag = np.ascontiguousarray(val, np.float32), np.ascontiguousarray(flag, np.uint8)
            if val.shape != (3, i1 - i0, ndays) or flag.shape != val.shape or not 0 <= i0 <= i1 <= n:
                raise ValueError("a batch must be (i0, i1, val [3, i1 - i0, ndays], flag [3, i1 - i0, ndays])")
            for e in range(3):
                if packed:
                    ncio.write_series_chunks(ds.variables[_VARS[e][0]], val[e], i0, deflate, device=device, timing=timing)
                    ncio.write_series_chunks(ds.variables[_VARS[3 + e][0]], flag[e], i0, deflate, device=device, timing=timing)
                    continue
                for j in range(i0, i1):
                    if raw:
                        ds.variables[_VARS[e][0]].write_chunk_raw((0, j), val[e, j - i0])
                        ds.variables[_VARS[3 + e][0]].write_chunk_raw((0, j), flag[e, j - i0])
                    else:
                        hold[_VARS[e][0]][:, j] = val[e, j - i0]
                        hold[_VARS[3 + e][0]][:, j] = flag[e, j - i0].view("S1")
        if not raw:
            for name, a in hold.items():
                ds.variables[name][:] = a
        if tobs is not None:
            tobs = np.ascontiguousarray(tobs() if callable(tobs) else tobs, np.int16)
            if tobs.shape != (n, ndays):
                raise ValueError("tobs must be [nstn, ndays]")
            if packed:
                ncio.write_series_chunks(ds.variables["tobs_tmax"], tobs, 0, deflate, device=device, timing=timing)
            elif raw:
                for j in range(n):
                    ds.variables["tobs_tmax"].write_chunk_raw((0, j), tobs[j])
            else:
                ds.variables["tobs_tmax"][:] = np.ascontiguousarray(tobs.T)
    finally:
        ds.close()
    return path


def _with_raws(stns, raws, stats):
    """The station table of both networks, sorted by id as ``insert_data_netcdf_db`` sorts it (:509), and the RAWS part."""
    from . import raws as _raws
    rstns = _raws.read_raws_stations(*raws, stats=stats)
    width = max(stns.dtype["station_name"].itemsize, rstns.dtype["station_name"].itemsize) // 4
    dtype = [(n, "U%d" % width) if n == "station_name" else (n, t) for n, t in STN_DTYPE]
    both = np.concatenate([stns.astype(dtype), rstns.astype(dtype)])
    both = both[np.argsort(both[sdb.STN_ID], kind="stable")]
    ids = both[sdb.STN_ID]
    if np.any(ids[1:] == ids[:-1]):
        raise ValueError("station id %s is listed twice" % ids[1:][ids[1:] == ids[:-1]][0])
    # the prefixes make each network a contiguous run of rows: the writer relies on it
    assert all(s.startswith("GHCN_") for s in ids[:stns.size]) and all(s.startswith("RAWS_") for s in ids[stns.size:])
    return both, rstns


def create_all_stations_db(path, path_stn_file, path_obs_files, start, end, path_by_year=None, check_obs_exist=False,
                           format=None, batch_bytes=BATCH_BYTES, device=0, timing=None, stats=None, raws=None, deflate=None):
    """The reference's step04: the database every later step takes as ``--db``.  ``tmin`` / ``tmax`` / ``prcp`` and their
    GHCN quality flags of every station of ``read_ghcn_stations`` over the period, and with ``path_by_year`` the times of
    observation of Tmax as ``tobs_tmax`` (int16, -1 = none).  ``raws`` = (metadata file, id file, directory of the daily
    listings), the arguments of ``raws.read_raws_stations``, adds the RAWS sites: the table is the union of both networks
    sorted by id, the RAWS rows have empty flags and no time of observation; ``stats`` receives their counts as
    ``raws_*``.  Without ``raws`` the file is what it was before the RAWS ingest existed.  ``deflate`` = ``"gpu"``: the seven
    ``(time, station_id)`` variables are created with ``zlib=True`` and their rows deflated on the GPU batch by batch
    (``"host"``: by libhdf5); ``None``: not compressed, as before.  Every file is looked for before any device work.
    Returns the station table."""
    if deflate not in (None, "gpu", "host"):
        raise ValueError("deflate must be None, 'gpu' or 'host', not %r" % (deflate,))
    min_ymd, max_ymd, d0, ndays = _period(start, end)
    stns = read_ghcn_stations(path_stn_file, path_obs_files, check_obs_exist)
    if stns.size < 1:
        raise ValueError("%s lists no station to insert" % path_stn_file)
    paths = _dly_paths(stns[sdb.STN_ID], path_obs_files)
    nghcn, rpaths, allstns = int(stns.size), [], stns
    if raws is not None:
        from . import raws as _raws
        if len(tuple(raws)) != 3:
            raise ValueError("raws must be (metadata file, id file, directory of the daily listings)")
        allstns, rstns = _with_raws(stns, tuple(raws), stats)
        rpaths = _raws._raws_paths(rstns[sdb.STN_ID], raws[2])
    years = range(d0.year, (d0 + _dt.timedelta(ndays - 1)).year + 1)
    by_year = _by_year_files(path_by_year, years) if path_by_year is not None else None
    days = get_days_metadata(d0, d0 + _dt.timedelta(ndays - 1))

    def tobs():
        tstats = {}
        out = parse_tobs_files(by_year, stns[sdb.STN_ID], start, end, device=device, timing=timing, stats=tstats)
        if stats is not None:
            stats.update({"tobs_" + k: v for k, v in tstats.items()})
        if allstns.size > nghcn:                                   # a RAWS site has no time of observation
            out = np.concatenate([out, np.full((allstns.size - nghcn, ndays), -1, np.int16)])
        return out

    def batches():
        for b in iter_dly_batches(paths, start, end, batch_bytes=batch_bytes, device=device, timing=timing, stats=stats):
            yield b
        if rpaths:
            rstats = {}
            try:
                for i0, i1, val, flag in _raws.iter_raws_batches(rpaths, start, end, batch_bytes=batch_bytes, device=device,
                                                                 timing=timing, stats=rstats):
                    yield nghcn + i0, nghcn + i1, val, flag
            finally:
                if stats is not None:
                    stats.update({"raws_" + k: v for k, v in rstats.items()})

    write_all_stations_db(path, allstns, days, batches(), tobs=tobs if by_year is not None else None, format=format,
                          deflate=deflate, device=device, timing=timing)
    return allstns


def create_tobs_db(path_ghcn_yrly, fpath_db, stnids, min_date, max_date, element="TMAX", format=None, device=0):
    """``create_tobs_file`` + ``create_tobs_db`` (tobs.py:35-157): the reference's stand-alone time-of-observation file,
    ``tobs`` int16 on ``(time, stn_id)``, chunks ``(ndays, 50)``, fill and ``missing_value`` -1."""
    min_ymd, max_ymd, d0, ndays = _period(min_date, max_date)
    stnids = np.asarray(stnids)
    years = range(d0.year, (d0 + _dt.timedelta(ndays - 1)).year + 1)
    tobs = parse_tobs_files(_by_year_files(path_ghcn_yrly, years), stnids, min_date, max_date, element=element, device=device)
    ds = ncio.open_dataset(fpath_db, "w", format)
    try:
        ds.title = "Time-of-Observation Database"
        ds.institution = "University of Montana Numerical Terradynamics Simulation Group"
        ds.history = "Created on: " + _dt.date.today().strftime("%Y-%m-%d")
        ds.createDimension("time", ndays)
        ds.createDimension("stn_id", int(stnids.size))
        tv = ds.createVariable("time", "f8", ("time",))
        tv.long_name, tv.units, tv.standard_name, tv.calendar = "time", ncio._units(d0), "time", "standard"
        tv[:] = np.arange(ndays, dtype=np.float64)
        ncio._write_ids(ds, "stn_id", "stn_id", stnids).long_name = "station id"
        kw = dict(chunksizes=(ndays, min(50, int(stnids.size)))) if ncio._is_nc4(ds) else {}
        v = ds.createVariable("tobs", "i2", ("time", "stn_id"), fill_value=np.int16(-1), **kw)
        v.long_name, v.missing_value = "time-of-observation", np.int16(-1)
        v[:] = np.ascontiguousarray(tobs.T)
    finally:
        ds.close()
    return tobs
