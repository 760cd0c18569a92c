"""The rules of the RAWS ingest in plain Python: what ``InsertRaws.parse_stn_obs`` and ``get_stns``
(twx/db/create_db_all_stations.py:1132-1233) do to a daily listing, with the one stated deviation (of several lines that
give a day the last wins), and what the device decides of it (include/twx_raws.h, twxrw_parse).  No import of the package:
the tests compare the package, the kernels and the CPU program of the field code with this, and this with the executed
reference (tests/golden/golden_raws_v1.npz)."""
import datetime
import re

import numpy as np

MISSING = -9999.0
SKIP_LINES = 7
TOK_MAX = 40
FIELD_TOKEN = (0, 9, 10, 14)                        # date, tmax, tmin, prcp
NO_DAY = 0xffffffff
_INT = re.compile(rb"[+-]?[0-9]{1,9}\Z")
_FLOAT = re.compile(rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)\Z")
_TOKEN = re.compile(rb"[^ \t\n\r\x0b\x0c]+")


def day_axis(min_ymd, max_ymd):
    d0 = datetime.date(min_ymd // 10000, min_ymd // 100 % 100, min_ymd % 100)
    d1 = datetime.date(max_ymd // 10000, max_ymd // 100 % 100, max_ymd % 100)
    return d0, (d1 - d0).days + 1


def lines_of(data):
    """[(position, line without its newline)]: a line ends at \\n, a last line without one is a line, a newline that ends the
    file opens no further line."""
    out, pos = [], 0
    while pos < len(data):
        end = data.find(b"\n", pos)
        end = len(data) if end < 0 else end
        out.append((pos, data[pos:end]))
        pos = end + 1
    return out


def body_of(data):
    """The lines that take part: from the 8th on, before the first of them that contains ``Copyright``."""
    out = []
    for pos, line in lines_of(data)[SKIP_LINES:]:
        if b"Copyright" in line:
            break
        out.append((pos, line))
    return out


def calendar_day(year, month, day):
    if not (1 <= year <= 9999 and 1 <= month <= 12 and day >= 1):
        return False
    leap = (year % 4 == 0 and year % 100 != 0) or year % 400 == 0
    return day <= (31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[month - 1]


def parse_line(line, min_ymd, max_ymd, d0):
    """``"skip"``, ``"outside"`` or ``(day index, tmin, tmax, prcp)`` (float32 each); raises IndexError / ValueError."""
    vals = line.split()                                            # bytes: the six ASCII whitespace bytes
    t = vals[0]
    try:
        year, month, day = int(t[6:]), int(t[0:2]), int(t[3:5])
    except ValueError:
        return "skip"
    if not calendar_day(year, month, day):
        return "skip"
    ymd = year * 10000 + month * 100 + day
    if ymd < min_ymd or ymd > max_ymd:
        return "outside"
    tmax, tmin, prcp = float(vals[9]), float(vals[10]), float(vals[14])
    if prcp != MISSING:
        prcp = prcp * 0.1
    with np.errstate(over="ignore"):                              # a token beyond float32's range is inf, as in the reference
        return (datetime.date(year, month, day) - d0).days, np.float32(tmin), np.float32(tmax), np.float32(prcp)


def parse_raws(data, min_ymd, max_ymd):
    """One listing: ``val`` [3, ndays] float32 (tmin, tmax, prcp), ``raised`` = None or (exception name, 1-based line), and
    the counts ``lines``, ``body``, ``skipped``, ``values``, ``duplicates``.  After a raise nothing else is meaningful."""
    d0, ndays = day_axis(min_ymd, max_ymd)
    val = np.full((3, ndays), MISSING, np.float32)
    all_lines = lines_of(data)
    body = body_of(data)
    r = dict(val=val, raised=None, lines=len(all_lines), body=len(body), skipped=0, values=0, duplicates=0)
    seen = set()
    for pos, line in body:
        try:
            got = parse_line(line, min_ymd, max_ymd, d0)
        except (IndexError, ValueError) as exc:
            r["raised"] = (type(exc).__name__, data[:pos].count(b"\n") + 1)
            return r
        if got == "skip":
            r["skipped"] += 1
        elif got != "outside":
            k = got[0]
            r["values"] += 1
            r["duplicates"] += k in seen
            seen.add(k)
            val[0, k], val[1, k], val[2, k] = got[1:]
    return r


def device_int(s):
    return _INT.match(s) is not None


def device_float(s):
    if len(s) > TOK_MAX or _FLOAT.match(s) is None:
        return False
    digits = s.lstrip(b"+-").replace(b".", b"")
    decimals = len(s) - s.index(b".") - 1 if b"." in s else 0
    return len(digits.lstrip(b"0")) <= 15 and decimals <= 22


def device_view(data, min_ymd, max_ymd, f=0, base=0):
    """What ``twxrw_parse`` returns for this file as file ``f`` of a batch that has it at ``base``: the two lists (sorted, as
    tuples of 8) and the eight counts."""
    d0, _ = day_axis(min_ymd, max_ymd)
    unc, rse, decided = [], [], {}
    c = dict(lines=len(lines_of(data)), body=0, skipped=0, values=0, duplicates=0, uncertain=0, date_uncertain=0)
    c["raise"] = 0
    pending = []
    for pos, line in body_of(data):
        c["body"] += 1
        toks = [(m.start(), m.group()) for m in _TOKEN.finditer(line)]
        start = base + pos
        if not toks:
            rse.append((f, pos, 0, 0, 0, 0, NO_DAY, start))
            continue
        off, t = toks[0]
        if len(t) > TOK_MAX or not (device_int(t[6:]) and device_int(t[0:2]) and device_int(t[3:5])):
            unc.append((f, pos, 0, off, min(len(t), TOK_MAX + 1), 0, NO_DAY, start))
            c["date_uncertain"] += 1
            continue
        year, month, day = int(t[6:]), int(t[0:2]), int(t[3:5])
        if not calendar_day(year, month, day):
            c["skipped"] += 1
            continue
        if not (min_ymd <= year * 10000 + month * 100 + day <= max_ymd):
            continue
        k = (datetime.date(year, month, day) - d0).days
        if len(toks) < 15:
            rse.append((f, pos, 1, 0, len(toks), 0, k, start))
            continue
        bad = [q for q in (1, 2, 3) if not device_float(toks[FIELD_TOKEN[q]][1])]
        if bad:
            pending.append((pos, k, [(q, toks[FIELD_TOKEN[q]][0], min(len(toks[FIELD_TOKEN[q]][1]), TOK_MAX + 1)) for q in bad]))
            continue
        c["values"] += 1
        c["duplicates"] += k in decided
        decided[k] = start + 1
    for pos, k, fields in pending:
        unc += [(f, pos, q, off, n, decided.get(k, 0), k, base + pos) for q, off, n in fields]
    c["uncertain"], c["raise"] = len(unc), len(rse)
    return sorted(unc, key=lambda e: (e[7], e[2])), rse, c


def get_stns(ids_text, meta_text, have):
    """``InsertRaws.get_stns``: [(id, lat, lon, elev, state, name)] sorted by id, and how many were left out."""
    def lines(data):
        return re.findall(rb"[^\n]*\n|[^\n]+", data)

    states = {l[2:6]: l[0:2].upper() for l in lines(ids_text)}
    rows, missing = [], 0
    for l in lines(meta_text):
        orig, vals = l[0:4].strip(b" \t\n\r\x0b\x0c"), l.split()
        row = ("RAWS_" + orig.decode("latin-1"), float(vals[3]), -float(vals[4]), float(vals[5]), states[orig].decode("latin-1"),
               b" ".join(vals[6:]).decode("ascii", "ignore"))
        if orig.decode("latin-1") in have:
            rows.append(row)
        else:
            missing += 1
    return sorted(rows), missing
