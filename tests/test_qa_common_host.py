"""The host scaffold the units of libtwxqa.so share (topowx_amd/qa/twx_qa_common.h) without a GPU: its error formatter and
its calendar helpers run as a program of their own (tests/tools/qa_common_hostcheck.cpp), and the text of the units shows
that none of them has grown a copy of the scaffold again."""
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
OWN_DESIGN = "twx_mosaic.hip"                                      # errors and events of a persistent object: not a copy
DATES = [(1583, 1, 1), (1900, 2, 28), (1900, 3, 1), (1948, 1, 1), (1970, 1, 1), (2000, 2, 29), (2016, 12, 31)]


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "qa_common_hostcheck")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + QA,
                        os.path.join(HERE, "tools", "qa_common_hostcheck.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


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
        assert '#include "%s"' % HEADER in src, path
        for owned in ("hipFree(", "hipEventDestroy(", "hipGetErrorString("):
            assert owned not in src, (path, owned)
    ndef = 0
    for path in glob.glob(os.path.join(QA, "*.hip")) + glob.glob(os.path.join(QA, "*.h")):
        ndef += len(re.findall(r"days_from_civil\(int64_t y, int mth, int day\)\s*(?://[^\n]*)?\n\{", open(path).read()))
    assert ndef == 1
    common = open(os.path.join(QA, HEADER)).read()
    assert common.count("qa_days_from_civil(int64_t y, int mth, int day)") == 1
