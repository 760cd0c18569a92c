"""The host scaffold the units of libtwxqa.so share (topowx_amd/qa/twx_qa_common.h) and the day-axis calendar of
topowx_amd/qa/twx_qa_series.h without a GPU: the error formatter, the date helpers and the calendar run as programs of their
own (tests/tools/qa_common_hostcheck.cpp, qa_series_hostcheck.cpp), and the text of the units shows that none of them has
grown a copy of the scaffold, of the calendar or of the series helpers again."""
import calendar
import datetime
import glob
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QA = os.path.join(ROOT, "topowx_amd", "qa")
HEADER = "twx_qa_common.h"
SERIES = "twx_qa_series.h"                                         # includes HEADER; the units that use it include it instead
SERIES_UNITS = ("twx_nonspatial.hip", "twx_corrob.hip", "twx_prcpqa.hip", "twx_prcpcorrob.hip")
OWN_DESIGN = "twx_mosaic.hip"                                      # errors and events of a persistent object: not a copy
DATES = [(1583, 1, 1), (1900, 2, 28), (1900, 3, 1), (1948, 1, 1), (1970, 1, 1), (2000, 2, 29), (2016, 12, 31)]


def _program(tmp_path_factory, name):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("hostcheck") / name)
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + QA,
                        os.path.join(HERE, "tools", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _program(tmp_path_factory, "qa_common_hostcheck")


@pytest.fixture(scope="module")
def seriescheck(tmp_path_factory):
    return _program(tmp_path_factory, "qa_series_hostcheck")


def test_fail_and_calendar_as_a_program(hostcheck):
    args = [str(v) for ymd in DATES for v in ymd]
    res = subprocess.run([hostcheck] + args, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    out = {}
    dates = []
    for line in res.stdout.splitlines():
        key, rest = line.split(" ", 1)
        if key == "date":
            dates.append([int(v) for v in rest.split()])
        else:
            out[key] = rest
    errstr = re.fullmatch(r"\[(.+)\]", out["errstr"]).group(1)
    assert out["plain"] == "-1 [twxqa_demo: need n >= 1]"                    # "%s"
    assert out["hip"] == "-1 [hipMalloc(&p, n): %s]" % errstr               # "%s: %s" with the runtime's text
    assert out["macro"] == "-1 [e: %s]" % errstr and out["macro_ok"] == "0"  # QACHK: the stringised call, or falls through
    assert out["short"] == "-1 [0123456] len 7 guards 1"                      # truncated, NUL-terminated, nothing past the end
    assert out["none"] == "-1 -1 -1 [keep]"                                   # null / zero / negative length: no write
    assert len(dates) == len(DATES)
    for (y, m, d), got in zip(DATES, dates):
        want = [y, m, d, datetime.date(y, m, d).toordinal() - 719163, int(calendar.isleap(y))]
        assert got == want, (got, want)


def test_the_copies_are_gone_and_every_unit_includes_the_header():
    units = sorted(p for p in glob.glob(os.path.join(QA, "twx_*.hip")) if os.path.basename(p) != OWN_DESIGN)
    assert len(units) == 18
    for path in units:
        src = open(path).read()
        assert '#include "%s"' % HEADER in src or '#include "%s"' % SERIES in src, path
        for owned in ("hipFree(", "hipEventDestroy(", "hipGetErrorString("):
            assert owned not in src, (path, owned)
    ndef = 0
    for path in glob.glob(os.path.join(QA, "*.hip")) + glob.glob(os.path.join(QA, "*.h")):
        ndef += len(re.findall(r"days_from_civil\(int64_t y, int mth, int day\)\s*(?://[^\n]*)?\n\{", open(path).read()))
    assert ndef == 1
    assert '#include "%s"' % HEADER in open(os.path.join(QA, SERIES)).read()
    common = open(os.path.join(QA, HEADER)).read()
    assert common.count("qa_days_from_civil(int64_t y, int mth, int day)") == 1


# ---- the day-axis calendar ------------------------------------------------------------------------------------------
def _axis(first, ndays):
    return [first + datetime.timedelta(days=i) for i in range(ndays)]


def _ymd(dates):
    return [d.year * 10000 + d.month * 100 + d.day for d in dates]


def _calendar(seriescheck, tmp_path, ymd):
    path = tmp_path / "axis.txt"
    path.write_text(" ".join(str(v) for v in ymd))
    res = subprocess.run([seriescheck, str(path)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    out = {}
    for line in res.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out[key] = rest
    return out


def _ints(text):
    return [int(v) for v in text.split()]


AXES = {
    "one_day": (datetime.date(1987, 6, 5), 1),
    "one_year_to_31_december": (datetime.date(1999, 1, 1), 365),                 # no trailing empty year
    "from_29_february": (datetime.date(1992, 2, 29), 366),
    "mid_month_of_a_leap_year_to_1_january": (datetime.date(1996, 5, 17), 230),  # the last year has one day
    "five_months": (datetime.date(1990, 7, 15), 111),                            # .. 1990-11-02: check 6 skips month 4
    "over_every_year_cap": (datetime.date(1800, 1, 1), 54786),                   # 150 years .. 1949-12-31: the walk is still safe
}


@pytest.mark.parametrize("name", sorted(AXES))
def test_calendar_tables_equal_datetime(seriescheck, tmp_path, name):
    first, ndays = AXES[name]
    dates = _axis(first, ndays)
    if name == "one_year_to_31_december":
        assert dates[-1] == datetime.date(1999, 12, 31)
    if name == "mid_month_of_a_leap_year_to_1_january":
        assert dates[-1] == datetime.date(1997, 1, 1)
    if name == "five_months":
        assert dates[-1] == datetime.date(1990, 11, 2)
    out = _calendar(seriescheck, tmp_path, _ymd(dates))
    years = list(range(first.year, dates[-1].year + 1))
    ny = len(years)
    assert out["years"] == "0 %d []" % ny and out["walk"] == "0 []"
    want_cap = "0 []" if ny * 31 <= 62 else ("-1 [twxqa_demo: the series touches %d years; the demo sorts at most DEMO_CAP = 62 "
                                              "values of a calendar month (31 per year, 2 years)]" % ny)
    assert out["cap"] == want_cap
    assert int(out["ndistinct"]) == len({d.month for d in dates})
    yday = [d.timetuple().tm_yday - 1 for d in dates]
    leap = [int(calendar.isleap(d.year)) for d in dates]
    assert _ints(out["yr"]) == [v for y in years for v in ((datetime.date(y, 1, 1) - first).days, int(calendar.isleap(y)))]
    assert _ints(out["row"]) == yday
    assert _ints(out["normrow"]) == [r + 365 * lp for r, lp in zip(yday, leap)]
    assert _ints(out["mday"]) == [(datetime.date(2004, d.month, d.day) - datetime.date(2004, 1, 1)).days for d in dates]
    assert _ints(out["month"]) == [d.month for d in dates]
    assert _ints(out["yidx"]) == [d.year - first.year for d in dates]
    ystart, ylen, mstart, mlen = [0] * ny, [0] * ny, [0] * (ny * 12), [0] * (ny * 12)
    for i, d in enumerate(dates):
        k = d.year - first.year
        seg = k * 12 + d.month - 1
        if ylen[k] == 0:
            ystart[k] = i
        if mlen[seg] == 0:
            mstart[seg] = i
        ylen[k] += 1
        mlen[seg] += 1
    assert (_ints(out["ystart"]), _ints(out["ylen"])) == (ystart, ylen)
    assert (_ints(out["mstart"]), _ints(out["mlen"])) == (mstart, mlen)


def test_calendar_failures_name_the_day(seriescheck, tmp_path):
    ymd = _ymd(_axis(datetime.date(1995, 12, 20), 30))
    ymd[7] = ymd[6]                                                  # one repeated day
    out = _calendar(seriescheck, tmp_path, ymd)
    assert out["years"] == "0 2 []" and "yr" not in out
    assert out["walk"] == "-1 [twxqa_demo: ymd[7] = %d: the days are not consecutive calendar days]" % ymd[7]
    out = _calendar(seriescheck, tmp_path, [19901301, 19901302])
    assert out["years"] == "-1 0 [twxqa_demo: ymd[0] is not a date]" and "walk" not in out


def test_the_series_copies_are_gone():
    text = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(QA, "*.hip")) + glob.glob(os.path.join(QA, "*.h"))}
    everything = "\n".join(text.values())
    for once in ("3.40282346638528859812e38f", "for (int k = 2; k <= np2; k <<= 1)", "q == 59 && !y.y"):
        assert everything.count(once) == 1 and text[SERIES].count(once) == 1, once
    for unit in SERIES_UNITS:
        src = text[unit]
        assert '#include "%s"' % SERIES in src, unit
        for gone in ("the days are not consecutive calendar days", "struct NsCal", "struct PqCal", "ns_calendar(", "pq_calendar(",
                     "cb_calendar(", "pc_calendar("):
            assert gone not in src, (unit, gone)
    assert '#include "%s"' % SERIES in text["twx_infillmat.hip"] and "qa_finitef(" in text["twx_infillmat.hip"]
    assert len(re.findall(r"\bstruct QaCal\b", everything)) == 1 and len(re.findall(r"\bstruct QaCalendar\b", everything)) == 1
