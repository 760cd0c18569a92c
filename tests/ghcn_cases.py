"""Inputs of the GHCN-Daily ingest tests: station lists, ``.dly`` text and by-year CSV text, all generated here (our own
text in NOAA's published fixed-width layouts), scripted to the smallest inputs at which the parse kernels can go wrong,
plus a seeded pool of canonical text.  ``input_hash()`` pins them in the golden fixture.

A case is ``dict(name, min_ymd, max_ymd, files=[(station id without prefix, bytes), ...])``; every file of a case is parsed
over the case's period.  ``tobs_cases()`` are ``dict(name, min_ymd, max_ymd, ids, element, files=[bytes, ...])``.
"""
import hashlib

import numpy as np

BLANK = b"     "


def field(v):
    """The five value characters: an int right-justified, or five raw bytes."""
    if isinstance(v, bytes):
        assert len(v) == 5, v
        return v
    return b"%5d" % v


def dly_line(stn, year, month, elem, values, qflags=None, mflag=b" ", sflag=b"0"):
    """One ``.dly`` line without its newline (269 bytes): id(11) year(4) month(2) element(4), then 31 x value(5) mflag qflag
    sflag.  year / month / elem may be raw bytes of the field's width."""
    y = year if isinstance(year, bytes) else b"%04d" % year
    m = month if isinstance(month, bytes) else b"%02d" % month
    e = elem if isinstance(elem, bytes) else elem.encode()
    assert len(stn) == 11 and len(y) == 4 and len(m) == 2 and len(e) == 4
    out = [stn.encode() if isinstance(stn, str) else stn, y, m, e]
    for d in range(31):
        q = b" " if qflags is None else qflags[d]
        out.append(field(values[d]) + mflag + q + sflag)
    line = b"".join(out)
    assert len(line) == 269
    return line


def _vals(seed, lo=-400, hi=450):
    r = np.random.RandomState(seed)
    return [int(x) for x in r.randint(lo, hi, 31)]


def _stn(k):
    return "USC%08d" % k


def scripted_cases():
    cases = []
    # ---- one full line cut at every length 0 .. 270 (the newline is byte 269) ----
    v = _vals(1)
    v[0], v[1], v[14], v[15], v[30] = 200, -9999, 200, 5, 123
    q = [b" "] * 31
    q[14], q[15], q[30] = b"G", b"X", b"I"
    full = dly_line(_stn(1), 1948, 1, "TMAX", v, q) + b"\n"
    cases.append(dict(name="cut", min_ymd=19480101, max_ymd=19480205,
                      files=[(_stn(1000 + n), full[:n]) for n in range(271)]))
    # the same cuts with a second, whole line behind: the cut line is no longer the file's last
    tail = dly_line(_stn(1), 1948, 2, "TMIN", _vals(2)) + b"\n"
    cases.append(dict(name="cut_then_line", min_ymd=19480101, max_ymd=19480205,
                      files=[(_stn(2000 + n), full[:n] + b"\n" + tail) for n in (0, 10, 14, 16, 20, 21, 22, 25, 26, 27, 28, 29,
                                                                                 63, 64, 65, 255, 256, 257, 268, 269)]))
    # ---- dates ----
    for year in (1900, 1948, 2000, 2015):
        lines = [dly_line(_stn(3), year, mth, el, _vals(year + k)) for k, (mth, el) in enumerate(
            ((2, "TMIN"), (2, "TMAX"), (4, "PRCP"), (4, "TMIN"), (b"00", "TMAX"), (13, "TMAX"), (3, "PRCP"), (5, "TMAX")))]
        lines.append(dly_line(_stn(3), b"0000", 2, "TMAX", _vals(7)))
        cases.append(dict(name="dates%d" % year, min_ymd=year * 10000 + 201, max_ymd=year * 10000 + 505,
                          files=[(_stn(3), b"\n".join(lines) + b"\n")]))
    lines = [dly_line(_stn(4), y, m, el, _vals(y + m)) for (y, m) in ((1947, 12), (1948, 1), (1948, 2), (1948, 3))
             for el in ("TMIN", "TMAX", "PRCP")]
    cases.append(dict(name="midmonth", min_ymd=19480115, max_ymd=19480216, files=[(_stn(4), b"\n".join(lines) + b"\n")]))
    # ---- value fields ----
    texts = [b"-9999", b"99999", b"   -0", b"  +12", b"    0", b"12   ", b" 12  ", b"\t  12", b"1    ", b"    1", b"   12",
             b"  123", b" 1234", b"12345", b" 1.5e", b"  1e3", b"  nan", b"  1_0", b" 12 3", b"  - 1", BLANK, b"  1.5",
             b" -999", b"+9999", b"  inf", b"1\x002  ", b"-0000", b"   +0", b"    -", b"\x0b\x0c 7 ", b"00012"]
    assert len(texts) == 31
    files = []
    for k, el in enumerate(("TMIN", "TMAX", "PRCP")):
        body = dly_line(_stn(5 + k), 1948, 1, el, texts[k:] + texts[:k])
        files.append((_stn(5 + k), body + b"\n"))
    crlf = [dly_line(_stn(8), 1948, 1, "TMAX", _vals(8)), dly_line(_stn(8), 1948, 1, "PRCP", _vals(9, 0, 900))]
    files.append((_stn(8), b"\r\n".join(crlf) + b"\r\n"))
    files.append((_stn(9), crlf[0][:21 + 8 * 9 + 3] + b"\r\n" + crlf[1][:21 + 8 * 9 + 5] + b"\r\n" + crlf[1][:21 + 8 * 2 + 6] + b"\r"))
    cases.append(dict(name="values", min_ymd=19480101, max_ymd=19480131, files=files))
    # ---- duplicates ----
    a, b, c = _vals(10), _vals(11), _vals(12)
    b[3], c[4] = -9999, -9999
    qa, qb = [b"A"] * 31, [b" "] * 31
    filler = [dly_line(_stn(20), 1948, 1 + (k % 2), "SNOW", _vals(k)) for k in range(2100)]
    fb1, fb2 = list(b), list(b)
    fb1[5], fb1[6], fb2[7] = b" 1.5e", b"  1e3", b"  2e1"
    files = [
        (_stn(20), b"\n".join([dly_line(_stn(20), 1948, 1, "TMAX", a, qa), dly_line(_stn(20), 1948, 1, "TMAX", b, qb)]) + b"\n"),
        (_stn(21), b"\n".join([dly_line(_stn(21), 1948, 1, "TMIN", a, qa), dly_line(_stn(21), 1948, 1, "TMIN", b, qb),
                               dly_line(_stn(21), 1948, 1, "TMIN", c, qa)]) + b"\n"),
        (_stn(22), b"\n".join([dly_line(_stn(22), 1948, 1, "PRCP", a, qa)] + filler +
                              [dly_line(_stn(22), 1948, 1, "PRCP", b, qb)] + filler[:1100] +
                              [dly_line(_stn(22), 1948, 1, "PRCP", c)]) + b"\n"),
        (_stn(23), b"\n".join([dly_line(_stn(23), 1948, 1, "TMAX", a, qa), dly_line(_stn(23), 1948, 1, "TMAX", b, qb)[:21 + 8 * 19 + 2],
                               dly_line(_stn(23), 1948, 2, "TMAX", c)]) + b"\n"),
        (_stn(24), b"\n".join([dly_line(_stn(24), 1948, 1, "TMAX", a, qa), dly_line(_stn(24), 1948, 1, "TMAX", fb1, qb),
                               dly_line(_stn(24), 1948, 1, "TMIN", a)]) + b"\n"),
        (_stn(25), b"\n".join([dly_line(_stn(25), 1948, 1, "TMAX", a, qa), dly_line(_stn(25), 1948, 1, "TMAX", fb1, qb),
                               dly_line(_stn(25), 1948, 1, "TMAX", fb2, qa), dly_line(_stn(25), 1948, 1, "TMAX", c[:6] + [BLANK] * 25)])),
    ]
    cases.append(dict(name="dups", min_ymd=19480101, max_ymd=19480229, files=files))
    # ---- elements and flags ----
    lines = [dly_line(_stn(30), 1948, 1, el, _vals(30 + k)) for k, el in enumerate(
        ("TMIN", "TMAX", "PRCP", "TOBS", "SNOW", "tmax", b"TMX ", b" TMA", b"PRCP"))]
    qf = [b" ", b"G", b"\xe9", b"\t", b"\x00", b"z", b"0", b"S"] * 4
    lines.append(dly_line(_stn(30), 1948, 2, "TMAX", _vals(40), qf[:31]))
    lines.append(dly_line(_stn(30), 1948, 2, "PRCP", _vals(41, 0, 3000), list(reversed(qf[:31]))))
    cases.append(dict(name="elements_flags", min_ymd=19480101, max_ymd=19480229, files=[(_stn(30), b"\n".join(lines) + b"\n")]))
    # ---- files: empty, one line without a newline, line counts either side of a wavefront and of a workgroup ----
    def many(k, n):
        out, y, m = [], 1946, 1
        while len(out) < n:
            out.append(dly_line(_stn(k), y, m, ("TMIN", "TMAX", "PRCP")[len(out) % 3], _vals(len(out) + k)))
            if len(out) % 3 == 0:
                m += 1
                if m > 12:
                    y, m = y + 1, 1
        return b"\n".join(out) + b"\n"
    files = [(_stn(50), b""), (_stn(51), dly_line(_stn(51), 1948, 6, "TMAX", _vals(51))), (_stn(52), b"")]
    files += [(_stn(60 + k), many(60 + k, n)) for k, n in enumerate((1, 63, 64, 65, 1025))]
    files += [(_stn(70), b"\n"), (_stn(71), many(71, 2) + b"\n"), (_stn(72), b"")]
    cases.append(dict(name="files", min_ymd=19480101, max_ymd=19501231, files=files))
    return cases


def pool_case(seed=20240517, nstn=40):
    """40 stations x 1948-1952: canonical text only (the fallback count must be 0), months missing at random, -9999 and
    flags sprinkled, a few repeated (month, element) lines, and lines outside the period."""
    r = np.random.RandomState(seed)
    files = []
    for s in range(nstn):
        stn = "%s%09d" % (("US", "CA", "MX")[s % 3], 100000 + s)
        lines = []
        for y in range(1947, 1954):
            for m in range(1, 13):
                for el in ("TMAX", "TMIN", "PRCP", "SNOW"):
                    if r.rand() < 0.15:
                        continue
                    v = r.randint(0, 2500, 31) if el in ("PRCP", "SNOW") else r.randint(-450, 480, 31)
                    v[r.rand(31) < 0.08] = -9999
                    q = [bytes([c]) for c in r.choice(np.frombuffer(b"       DGIKX", np.uint8), 31)]
                    lines.append(dly_line(stn, y, m, el, [int(x) for x in v], q))
                    if r.rand() < 0.02:
                        lines.append(dly_line(stn, y, m, el, [int(x) for x in v[::-1]]))
        files.append((stn, b"\n".join(lines) + (b"\n" if s % 5 else b"")))
    return dict(name="pool", min_ymd=19480101, max_ymd=19521231, files=files)


STATION_LINES = [
    # id          lat       lon      elev   st name                           gsn hcn wmo
    ("USC00010008", 31.5703, -85.2483, 139.0, "AL", "ABBEVILLE"),
    ("USW00094728", 40.7789, -73.9692, 39.6, "NY", "NEW YORK CNTRL PK TWR"),
    ("USS0010B04S", 45.2667, -111.4167, 2465.8, "MT", "SNOTEL SITE"),
    ("USR0000ABAN", 34.3931, -117.0736, 1402.1, "CA", "RAWS SITE"),
    ("USC00500026", 64.7000, -147.1000, 200.0, "AK", "ALASKA SITE"),
    ("USC00510055", 21.3000, -157.8000, 5.0, "HI", "HAWAII SITE"),
    ("CA001011500", 48.9333, -123.7500, 75.0, "BC", "CHEMAINUS"),
    ("MXN00002001", 32.5500, -116.9500, 100.0, "  ", "TIJUANA \xe9 AEROPUERTO"),
    ("ASN00001000", -14.3, 126.6, 23.0, "  ", "AUSTRALIAN SITE"),
    ("USC00010009", 31.0, -85.0, -999.9, "al", "lower case state"),
    ("CA001011501", 49.0, -123.0, 12.5, "  ", ""),
]


def stations_text(extra_ids=()):
    """ghcnd-stations.txt lines (85 columns) of STATION_LINES, out of id order, then ``extra_ids`` at made-up places."""
    rows = list(STATION_LINES[::-1]) + [(i, 30.0 + 0.25 * k, -100.0 - 0.5 * k, 100.0 + k, "TX", "POOL %d" % k)
                                        for k, i in enumerate(extra_ids)]
    out = []
    for sid, lat, lon, elev, st, name in rows:
        out.append(("%-11s %8.4f %9.4f %6.1f %-2s %-30s %-3s %-3s %5s" % (sid, lat, lon, elev, st, name[:30], "", "", ""))
                   .encode("latin-1"))
    return b"\n".join(out) + b"\n"


def tobs_cases():
    ids = ["CA001011500", "MXN00002001", "USC00010008", "USC00010009"]              # sorted, as create_tobs_db wants them

    def ln(stn, ymd, el, val, hhmm, nl=True):
        return ("%s,%08d,%s,%5d,,,0,%s" % (stn, ymd, el, val, hhmm)).encode() + (b"\n" if nl else b"")
    y48 = [ln(ids[0], 19480101, "TMAX", 200, "0700"), ln(ids[0], 19480101, "TMIN", 100, "0800"),
           ln(ids[0], 19480102, "TMAX", 210, "0000"), ln(ids[1], 19480102, "TMAX", 215, "2400"),
           ln("USC00099999", 19480102, "TMAX", 215, "0700"), ln(ids[2], 19480103, "TMAX", 1, "700"),
           ln(ids[3], 19480103, "TMAX", 1, "1800"), ln(ids[3], 19480103, "TMAX", 2, "1700"),
           ln(ids[1], 19480104, "TMAX", 5, "070A"), ln("ASN00001000", 19480104, "TMAX", 5, "0700"),
           ln(ids[1], 19471231, "TMAX", 5, "0600"), ln(ids[1], 19480230, "TMAX", 5, "0600"),
           ("%s,19480105,TMAX,   11,,," % ids[1]).encode() + b"\n", ln(ids[2], 19480105, "PRCP", 0, "0900"),
           ln(ids[1], 19480106, "TMAX", 5, "0730").replace(b"\n", b"\r\n"),
           ln(ids[2], 19480107, "TMAX", 5, "-100"), ln(ids[2], 19480108, "TMAX", 5, "+630"),
           ln(ids[0], 19480110, "TMAX", 5, "0900", nl=False)]
    y49 = [ln(ids[0], 19490101, "TMAX", 200, "0800"), ln(ids[0], 19480101, "TMAX", 1, "1600"),
           ln(ids[3], 19490301, "TMAX", 2, "0000"), ln(ids[0], 19490302, "TMAX", 5, "12345", nl=False)]
    outside = [10, 11]                     # a date before the period, a date that is no date: the reference's IndexError
    bad = [5]                              # "700": the last five characters start with a comma
    good = dict(name="tobs", min_ymd=19480101, max_ymd=19491231, ids=ids, element="TMAX",
                files=[b"".join(l for k, l in enumerate(y48) if k not in outside + bad), b"".join(y49)])
    out = dict(name="tobs_outside", min_ymd=19480101, max_ymd=19491231, ids=ids, element="TMAX",
               files=[b"".join(l for k, l in enumerate(y48) if k not in bad), b"".join(y49)])
    bad3 = dict(name="tobs_bad_700", min_ymd=19480101, max_ymd=19491231, ids=ids, element="TMAX", files=[b"".join(y48[:6])])
    badnl = dict(name="tobs_last_line", min_ymd=19480101, max_ymd=19491231, ids=ids, element="TMAX",
                 files=[y48[0] + y48[17]])
    tmin = dict(name="tobs_tmin", min_ymd=19480101, max_ymd=19480131, ids=ids, element="TMIN", files=[b"".join(y48[:4])])
    empty = dict(name="tobs_empty", min_ymd=19480101, max_ymd=19480131, ids=ids, element="TMAX", files=[b"", b"\n", b""])
    return [good, out, bad3, badnl, tmin, empty]


def input_hash():
    h = hashlib.sha256()
    for case in scripted_cases() + [pool_case()]:
        h.update(("%s %d %d" % (case["name"], case["min_ymd"], case["max_ymd"])).encode())
        for stn, data in case["files"]:
            h.update(stn.encode() + b"\0" + data + b"\0")
    for case in tobs_cases():
        h.update(("%s %d %d %s %s" % (case["name"], case["min_ymd"], case["max_ymd"], case["element"], ",".join(case["ids"]))).encode())
        for data in case["files"]:
            h.update(data + b"\0")
    h.update(stations_text())
    return h.hexdigest()
