"""Inputs of the RAWS ingest tests: scripted daily listings and a seeded pool, as bytes.  Shared by the golden maker
(tests/golden/make_golden_raws.py), the restatement's tests and the GPU tests; ``input_hash`` pins the fixture to them.

The layout is the WRCC daily listing's as ``InsertRaws.parse_stn_obs`` reads it: 7 lines of heading, then one line a day
whose token 0 is ``MM/DD/YYYY``, token 9 the maximum and token 10 the minimum air temperature, token 14 the precipitation
in mm, then a line with ``Copyright``.  The files are GENERATED: no real listing is stored.

A case is ``dict(name, min_ymd, max_ymd, files=[(station, bytes)], duplicates=bool)``; the cases with duplicate dates are
pinned by the restatement alone (the reference fails on them)."""
import datetime
import hashlib

import numpy as np

MIN_YMD, MAX_YMD = 20000101, 20021231              # 1096 days: room for a file of 1025 distinct days
D0 = datetime.date(2000, 1, 1)
HEAD = (b" Example Gulch Nevada\n\n:       Daily Summary\n: Date  Year  Day  Run  Solar Wind  Dir  Max  Ave  Max  Min ...\n"
        b"01/01/2000 not a data line\n:----\n: mm/dd/yyyy\n")
TAIL = b"Copyright: Western Regional Climate Center\n trailer\n\n"
WS = (b" ", b"\t", b"\n", b"\r", b"\x0b", b"\x0c")
SIZES = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
assert HEAD.count(b"\n") == 7


def date(k):
    """Token 0 of day k of the period."""
    return (D0 + datetime.timedelta(int(k))).strftime("%m/%d/%Y").encode()


def line(tok0, tmax=b"21.5", tmin=b"-3.2", prcp=b"12", sep=b" ", ntok=15, eol=b"\n", lead=b""):
    toks = [tok0, b"2000", b"17", b"17", b"123.4", b"2.5", b"180", b"7.1", b"10.5", tmax, tmin, b"55", b"80", b"30", prcp]
    toks += [b"x%d" % k for k in range(15, ntok)]
    return lead + sep.join(t for t in toks[:ntok] if t is not None) + eol


def listing(body, head=HEAD, tail=TAIL):
    return head + b"".join(body) + tail


def _case(name, files, duplicates=False):
    return dict(name=name, min_ymd=MIN_YMD, max_ymd=MAX_YMD, files=[("%s%02d" % (name[:2].upper(), k) if isinstance(f, bytes) else f[0],
                                                                      f if isinstance(f, bytes) else f[1])
                                                                     for k, f in enumerate(files)], duplicates=duplicates)


def scripted_cases():
    cases = []
    # one body line cut at every length (a cut that would raise is an expected exception), no newline after the cut
    full = line(date(40), b"30.25", b"-1.5", b"254", eol=b"")
    files = [("C%03d" % n, HEAD + full[:n]) for n in range(len(full) + 1)]
    cases.append(dict(name="cut", min_ymd=MIN_YMD, max_ymd=MAX_YMD, files=files, duplicates=False))
    # token 0 of every length 0 .. 12 (length 0: the line starts with its separator)
    t = b"02/05/2000XX"
    cases.append(_case("tok0", [listing([line(t[:n], lead=b" " if n == 0 else b"")]) for n in range(13)]))
    # the date slices: signs, letters, the unread bytes 2 and 5, leap days, years 0 and 10000
    toks = [b"+1/06/2000", b"-1/06/2000", b"a1/06/2000", b"01/+7/2000", b"01/-7/2000", b"01/b7/2000", b"01/08/+2000",
            b"01/08/-2000", b"01/09/20c0", b"01x10y2000", b"01\xff11\x002001", b"02/29/2000", b"02/29/2001", b"02/29/1900",
            b"02/30/2000", b"13/01/2000", b"00/10/2000", b"01/00/2000", b"01/01/0", b"01/01/0000", b"01/01/10000", b"1/12/2000",
            b"01/1/22000", b"01/13/2000", b"01/14/02001", b"1_/15/2000", b"01/15/2_000", b"01/16/2000.", b"12/31/1999",
            b"01/01/2003", b"12/31/2002", b"01/01/2000", b"\xb2\xb3/17/2000", b"01/18/" + b"0" * 40 + b"2000", b"01/19/000002000"]
    cases.append(_case("dates", [listing([line(t, tmax=b"%d.5" % k) for k, t in enumerate(toks)])]))
    # separators: each of the whitespace bytes (a newline splits the line), runs of them, CRLF, no final newline
    seps = [b" ", b"\t", b"\r", b"\x0b", b"\x0c", b"  \t ", b"\r\x0b\x0c ", b"\t\t"]
    files = [listing([line(date(50 + k), sep=s, tmax=b"%d" % k) for k, s in enumerate(seps)]),
             listing([line(date(60), sep=b"\n")]),
             listing([line(date(61)), line(date(62), lead=b" \t"), line(date(63), eol=b" \t \n")]).replace(b"\n", b"\r\n"),
             HEAD + line(date(64)) + line(date(65), eol=b""),
             HEAD + line(date(66)) + line(date(67), eol=b"\r")]
    cases.append(_case("space", files))
    # files of 0 .. 9 lines, with and without a final newline
    lines9 = [line(date(70 + k), tmax=b"%d" % k) for k in range(9)]
    files = [b"".join(lines9[:n]) for n in range(10)] + [b"".join(lines9[:n])[:-1] for n in (1, 7, 8, 9)] + [b"\n" * 7, b"\n" * 8]
    cases.append(_case("nlines", files))
    # Copyright: inside the first 7 lines, a whole line, inside a longer token, twice, followed by malformed lines
    ok = [line(date(80 + k), tmax=b"%d" % k) for k in range(4)]
    bad = [b"\n", b"  \n", line(date(90), ntok=3), line(date(91), tmax=b"abc")]
    files = [HEAD.replace(b"Daily", b"Copyright") + b"".join(ok) + TAIL,
             listing(ok[:2] + [b"Copyright\n"] + ok[2:] + bad, tail=b""),
             listing(ok[:2] + [line(date(82), tmin=b"xxCopyrightyy")] + ok[3:] + bad),
             listing(ok[:1] + [b" (c) Copyright\n"] + ok[1:2] + [b"Copyright\n"] + bad),
             listing(ok[:3] + [b"copyright COPYRIGHT Copyrigh t\n"] + ok[3:]),
             listing(ok + [b"x" * 1500 + b" Copyright"], tail=b""),
             listing(ok, tail=b"Copyrigh"),
             HEAD[:-1] + b" Copyright\n" + b"".join(ok) + b"Copyright"]
    cases.append(_case("copyright", files))
    # lines of 14, 15 and 40 tokens; an out-of-period line may be as short as it likes
    files = [listing([line(date(100), ntok=15), line(date(101), ntok=40), line(b"06/01/1999", ntok=1), line(b"06/01/2005", ntok=9)]),
             listing([line(date(102), ntok=14)]), listing([line(date(103), ntok=10)]), listing([line(date(104), ntok=9)]),
             listing([line(date(105), ntok=12, tmin=b"abc")]), listing([line(date(106), ntok=1)]),
             listing([line(date(107)), b"\n", line(date(108), ntok=2)]), listing([line(date(109)), b" \t \r\n"])]
    cases.append(_case("ntokens", files))
    # token 14 beyond bytes 256, 1 024 and 4 096, padded byte by byte so that token boundaries fall on every window edge
    body, k = [], 0
    for pad in list(range(230, 262)) + list(range(990, 1050)) + list(range(4060, 4100, 3)):
        body.append(line(date(120 + k), tmax=b"%d.25" % (k % 50), tmin=b" " * (pad // 2) + b"-7.5", prcp=b" " * (pad - pad // 2) + b"%d" % k))
        k += 1
    body.append(line(date(120 + k), sep=b" " * 100, ntok=40))
    body.append(b" ".join([date(121 + k)] + [b"y" * 700] * 8 + [b"1.5", b"-2.5", b"z" * 2100, b"q", b"r", b"33"]) + b"\n")
    body.append(b" " * 3000 + line(date(122 + k)))
    cases.append(_case("long", [listing(body), listing(body[::-1])]))
    # duplicate dates, adjacent and a thousand lines apart: the last line wins (restatement only)
    far = [line(date(k), tmax=b"%d" % (k % 40)) for k in range(1001)]
    files = [listing([line(date(5), tmax=b"1"), line(date(5), tmax=b"2", tmin=b"-9999", prcp=b"-9999")]),
             listing(far + [line(date(0), tmax=b"77.5")]),
             listing([line(date(6), tmax=b"1e1"), line(date(6), tmax=b"2"), line(date(7), tmax=b"3"), line(date(7), tmax=b"4e0"),
                      line(date(7), tmax=b"5"), line(date(7), tmax=b"6_0"), line(b"01/08/2_000",tmax=b"8"),
                      line(date(7), tmax=b"9"), line(b"01/08/2_000",tmax=b"10")])]
    cases.append(_case("dups", files, duplicates=True))
    # the numbers the device decides, and the ones it leaves to float()
    nums = [b"-9999", b"-9999.0", b"-0", b".5", b"5.", b"+1.25", b"0", b"-0.0", b"007", b"123456789012345", b"1234567890123456",
            b"0.123456789012345", b"0.1234567890123456", b"0." + b"0" * 21 + b"1", b"0." + b"0" * 22 + b"1", b"1." + b"0" * 22,
            b"1." + b"0" * 23, b"000000000000000000012.5", b"1e1", b"1E-2", b"nan", b"inf", b"-inf", b"+nan", b"Infinity", b"1_0",
            b"1_0.5", b"99999999999999.9", b"999999999999999.9", b"4503599627370497.5", b"0.3", b"2.675", b"-9999.00",
            b"9" * 39 + b".", b"9" * 41, b"1" + b"0" * 30]
    body = []
    for k, t in enumerate(nums):
        body += [line(date(200 + 3 * k), tmax=t), line(date(201 + 3 * k), tmin=t), line(date(202 + 3 * k), prcp=t)]
    refused = [b"abc", b"1.2.3", b"--1", b".", b"+", b"1e", b"0x10", b"1,5", b"\xb2", b"1\x005", b"_1", b"1__0", b"M"]
    files = [listing(body)] + [listing([line(date(10)), line(date(11 + (k % 3)), **{("tmax", "tmin", "prcp")[k % 3]: t}), line(date(20))])
                               for k, t in enumerate(refused)]
    files.append(listing([line(date(12), tmax=b"a", tmin=b"b", prcp=b"c")]))
    files.append(listing([line(date(13), tmax=b"1e1", tmin=b"b")]))
    files.append(listing([line(b"01/1_4/2000", tmax=b"x")]))
    files.append(listing([line(b"01/1_4/2000", ntok=3), line(date(15), ntok=2)]))
    cases.append(_case("numbers", files))
    # files of 1 .. 1025 body lines
    files = []
    for n in SIZES:
        files.append(listing([line(date(k), tmax=b"%d.%d" % (k % 45, n % 10), tmin=b"-%d" % (k % 30), prcp=b"%d" % ((k * 7) % 300))
                              for k in range(n)]))
    cases.append(_case("sizes", files))
    return cases


def pool_case(nstn=40, seed=20260):
    """About 40 stations over the 3 years in the plain-decimal grammar only: the device decides every field."""
    rng = np.random.RandomState(seed)
    ndays = (datetime.date(2002, 12, 31) - D0).days + 1
    files = []
    for s in range(nstn):
        first, last = sorted(rng.randint(0, ndays, 2))
        if s % 5 == 0:
            first, last = 0, ndays - 1
        body = []
        for k in range(first - min(first, 3), min(ndays + 3, last + 4)):
            if rng.rand() < 0.03:
                continue
            tok0 = (D0 + datetime.timedelta(int(k) - (3 if s % 7 == 0 else 0))).strftime("%m/%d/%Y").encode()
            t = 15.0 + 12.0 * np.sin(k / 58.0) + rng.randn() * 3
            vals = [(rng.choice(["%.1f", "%.2f", "%d", "%.0f.", "+%.1f"]) if v >= 0 else rng.choice(["%.1f", "%d"])) % v
                    for v in (t + 6 + rng.rand() * 4, t - 6 - rng.rand() * 4)]
            vals.append(rng.choice(["%d", "%.1f", "%.3f"]) % (0 if rng.rand() < 0.7 else rng.gamma(1.0, 40.0)))
            for j in range(3):
                if rng.rand() < 0.02:
                    vals[j] = rng.choice(["-9999", "-9999.0", "-9999.00"])
            gap = [b" " * rng.randint(1, 5) for _ in range(15)]
            toks = [tok0, b"%d" % (2000 + k // 366), b"%d" % (k % 366 + 1), b"%d" % (k + 1), b"%.1f" % (rng.rand() * 700), b"%.2f" % (rng.rand() * 9),
                    b"%d" % rng.randint(0, 360), b"%.1f" % (rng.rand() * 20), b"%.1f" % t, vals[0].encode(), vals[1].encode(),
                    b"%d" % rng.randint(5, 100), b"%d" % rng.randint(50, 101), b"%d" % rng.randint(1, 50), vals[2].encode()]
            if rng.rand() < 0.3:
                toks += [b"%.1f" % rng.rand(), b"0"]
            body.append(b"".join(g + t_ for g, t_ in zip(gap, toks))[len(gap[0]) * (s % 2):] + (b"\r\n" if s % 11 == 0 else b"\n"))
        files.append(("P%03d" % s, listing(body, tail=TAIL if s % 3 else b"")))
    return dict(name="pool", min_ymd=MIN_YMD, max_ymd=MAX_YMD, files=files, duplicates=False)


def station_files():
    """(id file, metadata file, ids with a listing): the inputs of ``get_stns``."""
    ids = b"nvNEXG\nutUBRY\ncaCSQU\nidIBOI\nmtMT1\nnvNEXH\nOrOXYZ"
    meta = (b"NEXG  x  y  39.5  117.25  1890  EXAMPLE GULCH\n"
            b"UBRY  x  y  37.6401  112.1701  2412.5  BRYCE   CANYON  \n"
            b"CSQU  a  b  36  118.5  640\n"
            b"IBOI  a  b  43.6  116.2  825  BOISE\tFIRE \xe9COLE\n"
            b"OXYZ  a  b  44.0  121.0  900  NO LISTING\n"
            b"NEXH  a  b  -44.0  -121.0  -9  SOUTH  EAST")
    return ids, meta, ("NEXG", "UBRY", "CSQU", "IBOI", "NEXH")


def station_files_keyerror():
    """An id of three characters: the id file's key ``line[2:6]`` holds the newline, the lookup does not."""
    return b"mtMT1\nnvNEXG\n", b"NEXG  x  y  39.5  117.25  1890  EXAMPLE GULCH\nMT1   a  b  47.0  110.0  1200  SHORT ID\n"


def input_hash():
    h = hashlib.sha256()
    for case in scripted_cases() + [pool_case()]:
        h.update(case["name"].encode())
        for stn, data in case["files"]:
            h.update(stn.encode() + b"\0" + data + b"\0")
    for part in station_files()[:2]:
        h.update(part)
    return h.hexdigest()
