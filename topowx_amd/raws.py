"""RAWS ingest (the reference's step04, second network): the WRCC daily listings of the RAWS sites, parsed on the GPU.

``InsertRaws`` (twx/db/create_db_all_stations.py:1106-1233).  GHCN-Daily's own copies of these sites are dropped by
``ghcn.read_ghcn_stations`` (network code ``R``), as the reference drops them; this module inserts them from their native
source.  The text is tokenised and decided on the GPU (``twxrw_parse``, a wavefront per line); the host reads the files of a
batch into one page-locked buffer on a thread pool and settles what only Python can: a line with a field that is not a
plain decimal goes through ``int()`` / ``float()`` exactly as the reference's would, and a line the reference dies on
raises its ``IndexError`` / ``ValueError`` naming the file and the line.

Three deviations from the reference, all stated here: when several lines of a file give the same day the LAST one wins
(the reference fails with ``ValueError`` in its chunk assignment) and the duplicates are counted; the station name is
ASCII with other bytes dropped (the one field not pinned by executing the reference); ``prcp`` is written (the reference
parses it and comments its write out).  Nothing is downloaded: the input is the listing as the reference's downloader
stores it (twx/db/download_stndata.py:599-628).
"""
import ctypes as C
import datetime as _dt
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _qalib, ghcn

__all__ = ["read_raws_stations", "iter_raws_batches", "parse_raws_files", "raws_parse", "MISSING", "SKIP_LINES"]

MISSING = ghcn.MISSING
SKIP_LINES = 7                                     # :1196
_WS = b" \t\n\r\x0b\x0c"
_LINES = re.compile(rb"[^\n]*\n|[^\n]+")            # readlines(): a last line without a newline is a line

# ---- the unit's one entry (twxrw_parse; TWXRW_* of include/twx_raws.h), bound here: the unit has a header of its own ----
RW_ENTRY = "twxrw_parse"
RW_PROTOTYPE = (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64] +
                [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int])
RW_KERNELS = ("rw_fill", "rw_index", "rw_body", "rw_claim", "rw_write")       # TWXRW_NKERNELS
RW_MAX_BYTES = 2147483584             # TWXRW_MAX_BYTES
RW_ENTRY_WORDS = 8                    # TWXRW_ENTRY_WORDS
RW_NO_DAY = 0xffffffff                # TWXRW_NO_DAY
RW_RAISE_EMPTY, RW_RAISE_FEW = 0, 1   # TWXRW_RAISE_*
RW_FIELDS = ("date", "tmax", "tmin", "prcp")                       # word 2 of an uncertain entry
RW_COUNTS = ("lines", "body", "skipped", "values", "duplicates", "uncertain", "raise", "date_uncertain")     # TWXRW_C_*


def _bind():
    """Give the entry its prototype in the loaded library; raises if the library lacks it (no fallback)."""
    lib = _qalib.load()
    if not hasattr(lib, RW_ENTRY):
        raise _qalib.QaError("%s has no %s: it is older than this binding, run ./build.sh" % (_qalib.LIB_PATH, RW_ENTRY))
    fn = getattr(lib, RW_ENTRY)
    fn.restype, fn.argtypes = RW_PROTOTYPE


def raws_parse(buf, file_off, min_ymd, max_ymd, ndays, uncertain_cap=4096, raise_cap=64, device=0, timing=None):
    """``twxrw_parse``: ``InsertRaws.parse_stn_obs`` (create_db_all_stations.py:1177-1233) of the daily listings laid end to
    end in ``buf`` (any object with the buffer protocol) at ``file_off`` [nfiles + 1]; file f fills row f.  Returns ``(val [3,
    nfiles, ndays] float32, win [nfiles, ndays] uint32 or None, uncertain [n, 8] uint32, raise [m, 8] uint32, counts [8]
    int64)`` as include/twx_raws.h describes them; ``win`` only when a date is left to Python.  The call is repeated once
    with room for every entry if a capacity was too small: no result depends on the capacities.  Arguments are checked
    before anything touches the device."""
    a, nbytes, off = _qalib._gh_buffer(buf, file_off)
    nfiles, ndays = off.size - 1, int(ndays)
    if ndays < 1:
        raise ValueError("ndays must be the number of days from min_ymd to max_ymd")
    ucap, rcap = int(uncertain_cap), int(raise_cap)
    if ucap < 0 or rcap < 0:
        raise ValueError("the capacities of the lists must not be negative")
    if 3 * nfiles * ndays > (1 << 31):                            # TWXRW_MAX_CELLS: refused before a buffer of that size is made
        raise ValueError("a call takes at most 3 nfiles ndays = 2^31 cells")
    _bind()
    while True:
        val = np.empty((3, nfiles, ndays), np.float32)
        win = np.empty((nfiles, ndays), np.uint32)
        unc = np.zeros((max(ucap, 1), RW_ENTRY_WORDS), np.uint32)
        rse = np.zeros((max(rcap, 1), RW_ENTRY_WORDS), np.uint32)
        counts = np.zeros(len(RW_COUNTS), np.int64)
        ms = _qalib._call(RW_ENTRY,
                          (int(device), a.ctypes.data if nbytes else None, nbytes, nfiles, off.ctypes.data, int(min_ymd),
                           int(max_ymd), ndays, val.ctypes.data, win.ctypes.data, unc.ctypes.data, ucap, rse.ctypes.data, rcap),
                          len(RW_KERNELS), counts)
        _qalib._put_times(timing, _qalib._ms_keys(RW_KERNELS), ms, add=True)
        if counts[5] <= ucap and counts[6] <= rcap:
            return (val, win if counts[7] > 0 else None, unc[:int(counts[5])].copy(), rse[:int(counts[6])].copy(), counts)
        ucap, rcap = max(ucap, int(counts[5])), max(rcap, int(counts[6]))


def read_raws_stations(path_stn_file, path_stnid_file, path_obs_files, stats=None):
    """``InsertRaws.get_stns`` (:1132-1175): the stations of the metadata file ``path_stn_file`` that have a listing
    ``<id>.txt`` under ``path_obs_files``, their state from the id file ``path_stnid_file``; ids prefixed ``RAWS_``, sorted
    as ``insert_data_netcdf_db`` sorts them (:509).  An id without a state raises ``KeyError``, as there.  The name is
    ASCII, other bytes dropped.  ``stats['raws_no_obs']`` counts the stations left out for want of a listing.  Returns a
    record array (station_id, latitude, longitude, elevation, state, station_name)."""
    states = {}
    with open(path_stnid_file, "rb") as fh:
        for line in _LINES.findall(fh.read()):
            states[line[2:6]] = line[0:2].upper()
    rows, missing = [], 0
    with open(path_stn_file, "rb") as fh:
        for line in _LINES.findall(fh.read()):
            orig = line[0:4].strip(_WS)
            vals = line.split()
            lat, lon, elev = float(vals[3]), -float(vals[4]), float(vals[5])
            if orig not in states:
                raise KeyError("%s: station %r has no state in %s" % (path_stn_file, orig.decode("latin-1"), path_stnid_file))
            name = b" ".join(vals[6:]).decode("ascii", "ignore")
            sid = orig.decode("latin-1")
            if os.path.exists(os.path.join(path_obs_files, "%s.txt" % sid)):
                rows.append(("RAWS_" + sid, lat, lon, elev, states[orig].decode("latin-1"), name))
            else:
                missing += 1
    if stats is not None:
        stats["raws_no_obs"] = stats.get("raws_no_obs", 0) + missing
    rows.sort(key=lambda r: r[0])
    dtype = [(n, "U%d" % max([30] + [len(r[5]) for r in rows])) if n == "station_name" else (n, t) for n, t in ghcn.STN_DTYPE]
    return np.array(rows, dtype=dtype)


def _raws_paths(stn_ids, path_obs_files):
    paths = []
    for s in stn_ids:
        s = str(s)
        p = os.path.join(path_obs_files, (s[5:] if s.startswith("RAWS_") else s) + ".txt")
        if not os.path.isfile(p):
            raise IOError("station %s: no observation file %s" % (s, p))
        paths.append(p)
    return paths


# ---- what only Python decides ------------------------------------------------------------------------------------------
def _parse_line_python(line, min_ymd, max_ymd, d0):
    """One body line as ``parse_stn_obs`` (:1207-1227) takes it: ``None`` for a date ``int()`` or the calendar refuses,
    ``()`` for a day outside the period, else ``(day index, tmin, tmax, prcp)``.  Raises the reference's ``IndexError`` /
    ``ValueError``."""
    vals = line.split()
    t = vals[0]
    try:
        year, month, day = int(t[6:]), int(t[0:2]), int(t[3:5])
        ymd = int("".join([str(year), "%02d" % (month,), "%02d" % (day,)]))
        date = _dt.date(year, month, day)
    except ValueError:
        return None
    if not (min_ymd <= ymd <= max_ymd):
        return ()
    tmax, tmin, prcp = float(vals[9]), float(vals[10]), float(vals[14])
    prcp = prcp * 0.1 if prcp != MISSING else MISSING
    return (date - d0).days, tmin, tmax, prcp


def _line_at(view, a, fend):
    """The bytes of the line that starts at ``a``, without its newline."""
    out, step = b"", 4096
    while a < fend:
        piece = bytes(view[a:min(fend, a + step)])
        k = piece.find(b"\n")
        if k >= 0:
            return out + piece[:k]
        out, a, step = out + piece, a + len(piece), step * 4
    return out


def _settle(view, off, paths, val, win, unc, rse, min_ymd, max_ymd, d0):
    """Apply the Python-side decisions to the rows of one batch, in position order; returns (values added, duplicates
    added, dates skipped).  Raises the first error of the batch in station order, then line order."""
    def where(f, pos):
        return "%s, line %d" % (paths[f], bytes(view[off[f]:off[f] + pos]).count(b"\n") + 1)

    first_raise = rse[0] if len(rse) else None
    added = dups = skipped = 0
    host_win, last = {}, -1
    for f, pos, field, toff, tlen, w, k, start in unc.tolist():
        if start == last:                                          # a further field of a line already settled
            continue
        last = start
        if first_raise is not None and start > first_raise[7]:
            break
        line = _line_at(view, int(off[f]) + pos, int(off[f + 1]))
        try:
            got = _parse_line_python(line, min_ymd, max_ymd, d0)
        except (IndexError, ValueError) as exc:
            raise type(exc)("%s: %s" % (where(f, pos), exc))
        if got is None:
            skipped += 1
        elif got:
            k, tmin, tmax, prcp = got
            w = max(int(w) if field != 0 else int(win[f, k]), host_win.get((f, k), 0))
            added += 1
            dups += w > 0
            if start + 1 > w:
                with np.errstate(over="ignore"):                   # beyond float32's range: inf, as in the reference
                    val[0, f, k], val[1, f, k], val[2, f, k] = np.float32(tmin), np.float32(tmax), np.float32(prcp)
                host_win[(f, k)] = start + 1
    if first_raise is not None:
        f, pos = int(first_raise[0]), int(first_raise[1])
        line = _line_at(view, int(off[f]) + pos, int(off[f + 1]))
        try:
            _parse_line_python(line, min_ymd, max_ymd, d0)
        except (IndexError, ValueError) as exc:
            raise type(exc)("%s: %s" % (where(f, pos), exc))
        raise RuntimeError("%s: listed to raise, and Python takes it" % where(f, pos))
    return added, dups, skipped


def iter_raws_batches(paths, start, end, batch_bytes=ghcn.BATCH_BYTES, device=0, timing=None, pinned=True, stats=None):
    """Parse the daily listings ``paths`` over the period, a batch of at most ``batch_bytes`` per device call.  Yields ``(i0,
    i1, val [3, i1 - i0, ndays] float32, flag [3, i1 - i0, ndays] uint8)``: station-major rows (tmin, tmax, prcp) of files
    i0 .. i1 - 1, ``MISSING`` where the file gives nothing; the flags are empty.  ``stats`` (a dict) receives ``bytes``,
    ``lines``, ``body``, ``skipped``, ``values``, ``duplicates``, ``uncertain``, ``read_s``, ``parse_s``, ``settle_s``;
    ``timing`` the kernel milliseconds."""
    min_ymd, max_ymd, d0, ndays = ghcn._period(start, end)
    if int(batch_bytes) < 1:
        raise ValueError("batch_bytes must be positive")
    sizes = [os.path.getsize(p) for p in paths]
    runs = ghcn._batches(sizes, int(batch_bytes), max(1, ghcn.MAX_BATCH_CELLS // (3 * ndays)))
    st = stats if stats is not None else {}
    for k in ("bytes", "lines", "body", "skipped", "values", "duplicates", "uncertain"):
        st.setdefault(k, 0)
    for k in ("read_s", "parse_s", "settle_s"):
        st.setdefault(k, 0.0)
    if not runs:
        return
    cap = max(sum(sizes[a:b]) for a, b in runs)
    buf = (_qalib.PinnedBuffer if pinned else ghcn._HostBuffer)(max(cap, 1))
    try:
        with ThreadPoolExecutor(max_workers=ghcn.MAX_READERS) as pool:
            for i0, i1 in runs:
                t0 = time.perf_counter()
                off = np.zeros(i1 - i0 + 1, np.int64)
                off[1:] = np.cumsum(sizes[i0:i1])
                list(pool.map(lambda j: ghcn._read_into(paths[i0 + j], buf.view[off[j]:off[j + 1]]), range(i1 - i0)))
                t1 = time.perf_counter()
                val, win, unc, rse, counts = raws_parse(buf.view, off, min_ymd, max_ymd, ndays, device=device, timing=timing)
                t2 = time.perf_counter()
                added, dups, skipped = _settle(buf.view, off, paths[i0:i1], val, win, unc, rse, min_ymd, max_ymd, d0)
                t3 = time.perf_counter()
                st["bytes"] += int(off[-1])
                st["lines"] += int(counts[0])
                st["body"] += int(counts[1])
                st["skipped"] += int(counts[2]) + skipped
                st["values"] += int(counts[3]) + added
                st["duplicates"] += int(counts[4]) + dups
                st["uncertain"] += int(counts[5])
                st["read_s"] += t1 - t0
                st["parse_s"] += t2 - t1
                st["settle_s"] += t3 - t2
                yield i0, i1, val, np.zeros(val.shape, np.uint8)
    finally:
        buf.close()


def parse_raws_files(paths, start, end, **kw):
    """All of ``iter_raws_batches`` at once: ``val [3, nfiles, ndays] float32`` (tmin, tmax, prcp)."""
    _, _, _, ndays = ghcn._period(start, end)
    val = np.full((3, len(paths), ndays), MISSING, np.float32)
    for i0, i1, v, _ in iter_raws_batches(paths, start, end, **kw):
        val[:, i0:i1] = v
    return val
