"""A Python / numpy restatement of the GHCN-Daily ingest: ``get_stns``, ``parse_stn_obs`` with ``__convert_units`` and the
assignment into the float32 / ``S1`` chunks (twx/db/create_db_all_stations.py:978-1103, 619-627), and ``create_tobs_db``'s
line loop (twx/homog/tobs.py:121-157).  The tests hold it against the golden fixture (the executed reference) everywhere;
the GPU tests then take from it what the fixture does not store: the list of fields only ``float()`` can decide, and the
counts.  Bytes in, bytes compared: whitespace is what ``bytes.strip`` / ``int`` / ``float`` strip.
"""
import datetime
import re

import numpy as np

ELEMENTS = (b"TMIN", b"TMAX", b"PRCP")
CANONICAL = re.compile(rb"[+-]?[0-9]+\Z")
MISSING = -9999.0


def day_axis(min_ymd, max_ymd):
    d0 = datetime.date(min_ymd // 10000, min_ymd // 100 % 100, min_ymd % 100)
    d1 = datetime.date(max_ymd // 10000, max_ymd // 100 % 100, max_ymd % 100)
    n = (d1 - d0).days + 1
    return d0, n


def lines_of(data):
    """(position, line with its newline) of a file's lines, as ``readline`` gives them."""
    out, p = [], 0
    while p < len(data):
        e = data.find(b"\n", p)
        e = len(data) if e < 0 else e + 1
        out.append((p, data[p:e]))
        p = e
    return out


def parse_dly(data, min_ymd, max_ymd):
    """One ``.dly`` file.  Returns ``dict(raised, val [3, ndays] float32, flag [3, ndays] uint8, fallback [(line position,
    day field 0 .. 30)], nvalues)``: ``raised`` is the position of the first line whose header ``int()`` refuses (the
    reference's ValueError), else None -- the arrays then hold what was parsed before it."""
    d0, n = day_axis(min_ymd, max_ymd)
    val = np.full((3, n), MISSING, np.float32)
    flag = np.zeros((3, n), np.uint8)
    fallback, nvalues = [], 0
    for pos, line in lines_of(data):
        try:
            year, month = int(line[11:15]), int(line[15:17])
        except ValueError:
            return dict(raised=pos, val=val, flag=flag, fallback=fallback, nvalues=nvalues)
        el = line[17:21].strip()
        if el not in ELEMENTS:
            continue
        e = ELEMENTS.index(el)
        for d in range(31):
            try:
                ymd = int(str(year) + "%02d" % month + "%02d" % (d + 1))
                date = datetime.date(year, month, d + 1)
            except ValueError:
                continue
            if not (min_ymd <= ymd <= max_ymd):
                continue
            text = line[21 + 8 * d:26 + 8 * d]
            if text.strip() and not CANONICAL.match(text.strip()):
                fallback.append((pos, d))
            try:
                v = float(text)
            except ValueError:
                continue
            if v != MISSING:
                v = v / 100.0 if e == 2 else v / 10.0
            q = line[27 + 8 * d:28 + 8 * d].strip().rstrip(b"\0")
            k = (date - d0).days
            val[e, k] = v                                          # float64 into float32: one rounding
            flag[e, k] = q[0] if q else 0
            nvalues += 1
    return dict(raised=None, val=val, flag=flag, fallback=fallback, nvalues=nvalues)


def get_stns(text, have=None):
    """``get_stns`` on the bytes of ghcnd-stations.txt; ``have``: the ids with a .dly file (``check_obs_exist``), or None.
    Rows ``(id, lat, lon, elev, state, name)`` sorted by id as ``insert_data_netcdf_db`` sorts them."""
    rows = []
    for line in text.decode("latin-1").split("\n"):
        if line[0:2] not in ("US", "CA", "MX"):
            continue
        orig = line[0:11].strip()
        state = line[38:40].strip().upper()
        name = "".join(c for c in line[41:71].strip() if ord(c) < 128)
        if state in ("HI", "AK") or orig[2] in ("S", "R"):
            continue
        if have is not None and orig not in have:
            continue
        rows.append(("GHCN_" + orig, float(line[12:20].strip()), float(line[21:30].strip()), float(line[31:37].strip()),
                     state, name))
    order = np.argsort(np.array([r[0] for r in rows], dtype=object), kind="stable")
    return [rows[k] for k in order]


def parse_tobs(files, ids, element, min_ymd, max_ymd):
    """``create_tobs_db``'s loop over the lines the ``zgrep`` chain of ``create_tobs_file`` keeps, the files in order.  ids:
    sorted, without prefix.  Returns ``dict(tobs [nstn, ndays] int16, raised (file, position) of the first line ``int()``
    refuses or None, outside, nvalues)``; a date that is no day of the period is skipped and counted (the one deviation)."""
    d0, n = day_axis(min_ymd, max_ymd)
    idx = {s.encode(): k for k, s in enumerate(ids)}
    tobs = np.full((len(ids), n), -1, np.int16)
    outside = nvalues = 0
    el = element.encode()
    for f, data in enumerate(files):
        for pos, line in lines_of(data):
            body = line[:-1] if line.endswith(b"\n") else line
            if len(body) < 25 or body[21:25] != el or body[0:2] not in (b"US", b"CA", b"MX"):
                continue
            if not body[-1:].isdigit() or body.endswith(b"2400"):
                continue
            if line[0:11] not in idx:
                continue
            try:
                ymd = int(line[12:20])
            except ValueError:
                return dict(tobs=tobs, raised=(f, pos), outside=outside, nvalues=nvalues)
            try:
                k = (datetime.date(ymd // 10000, ymd // 100 % 100, ymd % 100) - d0).days
            except ValueError:
                k = -1
            if not (min_ymd <= ymd <= max_ymd) or k < 0 or k >= n:
                outside += 1
                continue
            try:
                v = int((body + b"\n")[-5:])                    # grep ends every line it prints with a newline
            except ValueError:
                return dict(tobs=tobs, raised=(f, pos), outside=outside, nvalues=nvalues)
            tobs[idx[line[0:11]], k] = v
            nvalues += 1
    return dict(tobs=tobs, raised=None, outside=outside, nvalues=nvalues)
