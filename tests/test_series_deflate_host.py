"""The series coder (topowx_amd/series_deflate.py, topowx_amd/qa/twxsd_serdeflate.hip) without a GPU: the restatement inflates
to the shuffled rows on every case and every case has the property it exists for; the restatement's numpy tokens are the
oracle's; the binding refuses bad arguments before a library is loaded; ``ncio.write_series_chunks`` refuses a variable that is
not chunked ``(ndays, 1)`` with shuffle + deflate and its host route writes what the plain assignment writes; header, binding,
build script and documents agree; the kernels use no scratch; and the coder's own token, table and bit-string functions, run
on the CPU under the address and undefined-behaviour sanitizers as a program of its own, give the restatement's streams."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import restate_series_deflate as R  # noqa: E402
import series_deflate_cases as SC  # noqa: E402
from topowx_amd import _qalib, ghcn, h5nc, ncio, series_deflate as SD  # noqa: E402
from topowx_amd.infill import post_infill  # noqa: E402

# LDS bytes per work-group as the build's resource table names them: the plane's pieces (256 x 68), + the histograms of es
# planes / the scan words, sums and code lengths / the assembled block (16 400) and the code words
LDS = {"k_sd_hist<1>": 18516, "k_sd_hist<2>": 19624, "k_sd_hist<4>": 21840, "k_sd_count<1>": 17728, "k_sd_count<2>": 17728,
       "k_sd_count<4>": 17728, "k_sd_emit<1>": 34944, "k_sd_emit<2>": 34944, "k_sd_emit<4>": 34944, "k_sd_scan": 0}


@pytest.fixture(scope="module")
def restated():
    return [(c, R.deflate_call(c["rows"])) for c in SC.cases()]


def test_restated_streams_inflate_to_the_shuffled_rows(restated):
    props = set()
    for case, r in restated:
        rows = case["rows"]
        n, es = rows.shape[1], rows.dtype.itemsize
        for k, s in enumerate(r["streams"]):
            assert s[:2] == b"\x78\x01" and s[-9:-4] == b"\x01\x00\x00\xff\xff", case["name"]
            assert zlib.decompress(s) == SD.shuffled(rows[k]).tobytes() == R.shuffled(rows[k]).tobytes(), (case["name"], k)
            assert len(s) <= R.bound(n, es) == SD.bound(n, es), case["name"]
        SC.check(case, R, r)
        props.add(case["prop"])
    assert props == set(SC.PROPS)
    # the cases cover what the issue lists: every size, 1 / 2 / 65 rows, the three element sizes at every alignment
    shapes = {(c["rows"].shape, c["rows"].dtype.itemsize) for c, _ in restated}
    assert {s[1] for s, _ in shapes} >= set(SC.SIZES) and {s[0] for s, _ in shapes} >= {1, 2, 65}
    for es in (1, 2, 4):
        assert {n for (nr, n), e in shapes if e == es and nr >= 2} >= set(SC.SIZES)
    assert any(r["halvings"][0] >= 1 for _, r in restated)


def test_numpy_tokens_are_the_oracles(restated):
    for case, _ in restated:
        rows = case["rows"]
        if rows.shape[1] > 300 and case["prop"] not in ("runs", "all_fill"):
            continue
        for k in (0, rows.shape[0] - 1):
            for plane in R.shuffled(rows[k]):
                for s0 in range(0, plane.size, R.SEG):
                    s1 = min(plane.size, s0 + R.SEG)
                    got = R.tokens(plane, s0, s1)
                    assert list(zip(*[x.tolist() for x in got])) == R.DO.tokens(plane, s0, s1), (case["name"], k, s0)
    assert R.halvings([0] * R.NSYM) == 0
    assert [R.bound(n, es) for n, es in ((0, 1), (5, 3), (1 << 31, 1), (1 << 29, 4), (25203, 4))] == [-1, -1, -1, -1, 100863]


def test_binding_refuses_bad_arguments_before_a_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_qalib, "load", no_library)
    ok = np.zeros((3, 10), np.float32)
    for bad in (ok[0], ok[:, ::2], ok.astype(np.float64), np.zeros((3, 0), np.int16), [[1, 2]], ok.T):
        with pytest.raises(ValueError, match="rows must be|n >= 1"):
            SD.deflate_series(bad)
    with pytest.raises(ValueError, match="batch_bytes"):
        SD.deflate_series(ok, batch_bytes=0)
    with pytest.raises(ValueError, match="device"):
        SD.deflate_rows(ok, device=-1)
    with pytest.raises(ValueError, match="writable"):
        SD.deflate_rows(ok, out=b"abc")
    for n, es in ((0, 4), (10, 3), (1 << 31, 1), (1 << 29, 4)):
        with pytest.raises(ValueError):
            SD.bound(n, es)
    with pytest.raises(AssertionError, match="the library was loaded"):           # good arguments do reach the loader
        SD.deflate_series(ok)
    for fn, kw in ((post_infill.write_infill_db, dict(path="x", stns=None, days=None, tair_var="tmin", result=None)),
                   (post_infill.create_serially_complete_db, dict(fpath_infill_db="x", tair_var="tmin", fpath_out_serial_db="y")),
                   (ghcn.create_all_stations_db, dict(path="x", path_stn_file="s", path_obs_files="d", start=20000101, end=20000102))):
        with pytest.raises(ValueError, match="deflate must be"):
            fn(deflate="zlib", **kw)


def _quick_db(path, nstn, ndays, variables, format=None):
    from topowx_amd.dates import get_days_metadata
    import datetime
    stns = np.zeros(nstn, dtype=ghcn.STN_DTYPE)
    stns["station_id"] = ["S%03d" % i for i in range(nstn)]
    days = get_days_metadata(datetime.date(2000, 1, 1), datetime.date(2000, 1, 1) + datetime.timedelta(ndays - 1))
    ncio.create_quick_db(path, stns, days, variables, format=format)
    return ncio.open_dataset(path, "a")


VARS = [("tmin", "f4", float(ncio.FILL_F4), "minimum air temperature", "C"), ("flag_infilled", "i1", -127, "infilled flag", "")]


@pytest.mark.skipif(not h5nc.available(), reason="no libhdf5")
def test_write_series_chunks_checks_the_variable_and_its_host_route_is_the_assignment(tmp_path):
    nstn, nd = 5, 40
    rows = SC.tenths(np.random.default_rng(3), nstn, nd)
    flag = (rows == SC.MISSING).astype(np.int8)
    ds = _quick_db(str(tmp_path / "a.nc"), nstn, nd, VARS)
    try:
        ncio.write_series_chunks(ds.variables["tmin"], rows[1:4], i0=1, deflate="host")
        ncio.write_series_chunks(ds.variables["flag_infilled"], flag, deflate="host")
        assert np.array_equal(np.asarray(ds.variables["tmin"][:, 1:4]), rows[1:4].T)
        assert np.array_equal(np.asarray(ds.variables["flag_infilled"][:]), flag.T)
        assert (np.asarray(ds.variables["tmin"][:, 0]) == ncio.FILL_F4).all()
        for kw, pat in ((dict(rows=rows[:, :-1]), "rows must be"), (dict(rows=rows, i0=1), "rows must be"),
                        (dict(rows=rows.astype(np.float64)), "do not fit"), (dict(rows=rows, deflate="zlib"), "deflate must be")):
            with pytest.raises(ValueError, match=pat):
                ncio.write_series_chunks(ds.variables["tmin"], **dict(dict(deflate="host"), **kw))
        # variables that are not (ndays, 1) shuffle + deflate: the message names what was found
        for name, kw, pat in (("wide", dict(chunksizes=(nd, 2), zlib=True), r"found chunks \[40, 2\]"),
                              ("plain", dict(chunksizes=(nd, 1), zlib=False), "'zlib': False"),
                              ("noshuf", dict(chunksizes=(nd, 1), zlib=True, shuffle=False), "'shuffle': False"),
                              ("contig", dict(), "found chunks contiguous")):
            v = ds.createVariable(name, "f4", ("time", "station_id"), **kw)
            for how in ("gpu", "host"):
                with pytest.raises(ValueError, match=pat):
                    ncio.write_series_chunks(v, rows, deflate=how)
    finally:
        ds.close()
    # the classic container has no filter: the plain assignment, whatever deflate says
    ds = _quick_db(str(tmp_path / "c.nc"), nstn, nd, VARS, format="NETCDF3_64BIT")
    try:
        ncio.write_series_chunks(ds.variables["tmin"], rows, deflate="gpu")
        assert np.array_equal(np.asarray(ds.variables["tmin"][:]), rows.T)
    finally:
        ds.close()


def test_unit_is_declared_bound_and_built():
    h = open(os.path.join(ROOT, "include", "twx_series_deflate.h")).read()
    assert sorted(set(re.findall(r"\b(twxsd_\w+)\s*\(", h))) == sorted(SD.SD_PROTOTYPES) == [SD.SD_BOUND, SD.SD_ENTRY]
    scalar = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, (restype, argtypes) in SD.SD_PROTOTYPES.items():
        m = re.search(r"(\w+)\s+%s\(([^)]*)\)" % name, h)
        params = m.group(2).split(",")
        assert restype is scalar[m.group(1)] and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            p = re.sub(r"/\*.*?\*/", "", p)
            assert (t in (C.c_void_p, C.c_char_p)) if "*" in p else t is scalar[p.replace("const", " ").split()[0]], (name, p)
    assert int(re.search(r"#define TWXSD_NKERNELS (\d+)", h).group(1)) == len(SD.SD_KERNELS)
    assert int(re.search(r"#define TWXSD_NTIMES (\d+)", h).group(1)) == len(SD.SD_KERNELS) + len(SD.SD_HOST_TIMES)
    assert int(re.search(r"#define TWXSD_C_N (\d+)", h).group(1)) == len(SD.SD_COUNTS)
    assert int(re.search(r"#define TWXSD_E_CAP (\d+)", h).group(1)) == SD.SD_E_CAP
    # the entries are the unit's own: not in the shared header, not in the shared table
    assert "twxsd_" not in open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert not any(k.startswith("twxsd_") for k in _qalib._PROTOTYPES)
    hh = open(os.path.join(ROOT, "topowx_amd", "qa", "twx_serdeflate_host.h")).read()
    assert int(re.search(r"#define TWXSD_SEG (\d+)", hh).group(1)) == SD.SD_SEG == R.SEG
    assert (int(re.search(r"#define TWXSD_SAMPLE_SEG (\d+)", hh).group(1)), int(re.search(r"#define TWXSD_SAMPLE_ROW (\d+)", hh).group(1))) \
        == (R.SAMPLE_SEG, R.SAMPLE_ROW)
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert build.count("topowx_amd/qa/twxsd_serdeflate.hip") == 1
    assert build.index("topowx_amd/qa/twxsd_serdeflate.hip") < build.index("topowx_amd/qa/twxrw_raws.hip 2>")
    src = open(os.path.join(ROOT, "topowx_amd", "qa", "twxsd_serdeflate.hip")).read()
    assert '#include "twx_qa_common.h"' in src and '#include "twx_series_deflate.h"' in src and '#include "../csrc/twx_deflate.h"' in src
    assert not any(owned in src for owned in ("hipFree(", "hipEventDestroy(", "hipGetErrorString("))
    assert not re.search(r"\b(float|double)\b(?! \*kernel_ms| ms\[| \*ms)", re.sub(r"//[^\n]*", "", src))      # integers only
    for doc in ("README.md", "DESIGN.md"):
        assert "twxsd_deflate" in open(os.path.join(ROOT, doc)).read(), doc
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    lib = C.CDLL(_qalib.LIB_PATH)
    assert all(hasattr(lib, n) for n in SD.SD_PROTOTYPES)
    lib.twxsd_bound.restype, lib.twxsd_bound.argtypes = SD.SD_PROTOTYPES[SD.SD_BOUND]
    for n, es in ((1, 1), (16384, 2), (16385, 4), (25203, 4), (0, 1), (5, 3), (1 << 31, 1), (1 << 29, 4), ((1 << 29) - 1, 4)):
        assert lib.twxsd_bound(n, es) == R.bound(n, es), (n, es)
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    table = {k: v for k, v in isa_resources.parse(res).items() if k.startswith("k_sd_")}
    assert sorted(table) == sorted(LDS)
    for k, v in table.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["lds"] == LDS[k], (k, v)


def test_entry_refuses_bad_arguments_before_any_device_work():
    """Call-level failures (the library is needed, a GPU is not)."""
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    lib = SD._bind()
    buf = C.create_string_buffer(256)
    rows, out = np.zeros((2, 8), np.float32), np.zeros(400, np.uint8)
    off, cnt = np.zeros(3, np.int64), np.zeros(8, np.int64)
    ok = [0, rows.ctypes.data, 2, 8, 4, out.ctypes.data, 400, off.ctypes.data, cnt.ctypes.data, None, buf, 256]
    for at, val, pat in ((4, 3, "es must be"), (3, 0, "n must be"), (3, 1 << 29, r"below 2\^31"), (2, -1, "nrows"), (1, None, "NULL"),
                         (5, None, "NULL"), (7, None, "NULL"), (8, None, "NULL"), (6, -1, "out_cap"), (0, -1, "device"),
                         (2, 1 << 31, "items")):
        args = list(ok)
        args[at] = val
        assert lib.twxsd_deflate(*args) == -1 and re.search(pat, buf.value.decode()), (at, buf.value)
    off[:] = 7
    assert lib.twxsd_deflate(*(ok[:1] + [None, 0] + ok[3:5] + [None, 0] + ok[7:])) == 0 and off[0] == 0 and not cnt.any()


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "serdeflate_hostcheck")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(HERE, "tools", "hipstub"), "-I" + os.path.join(ROOT, "topowx_amd", "qa"),
                           "-I" + os.path.join(ROOT, "topowx_amd", "csrc"), os.path.join(HERE, "tools", "serdeflate_hostcheck.cpp"),
                           "-o", exe])
    return exe


def test_host_arithmetic_under_sanitizers(hostcheck):
    res = subprocess.run([hostcheck, "arith"], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    lines = [ln.split() for ln in res.stdout.splitlines()]
    bounds = [ln for ln in lines if ln[0] == "bound"]
    assert len(bounds) == 72
    for _, n, es, b in bounds:
        assert int(b) == R.bound(int(n), int(es)), (n, es)
    for _, n, nseg, _, last in (ln for ln in lines if ln[0] == "nseg"):
        assert int(nseg) == -(-int(n) // R.SEG) and int(last) == int(n) - (int(nseg) - 1) * R.SEG
    for _, a, es, h, h2 in (ln for ln in lines if ln[0] == "head"):
        want = ((16 - int(a) % 16) % 16) // int(es)
        assert (int(h), int(h2)) == (want, min(want, 2)) and (int(a) + int(h) * int(es)) % 16 == 0
    for _, r, s0, s16, s17 in (ln for ln in lines if ln[0] == "sampled"):
        assert [int(s0), int(s16), int(s17)] == [int(R.sampled(int(r), s)) for s in (0, 16, 17)]
    text = res.stdout
    assert text.count("dims_bad accepted") == 0 and text.count("dims_bad") == 6
    assert "dims_ok accepted 2 8 24000 100863 1209744000" in text and "dims_empty accepted 0 0" in text
    assert "offsets ok 0 17 47 59" in text and "offsets_long a deflated row" in text and "offsets_short a deflated row" in text


def test_the_coders_own_functions_on_the_cpu_give_the_restated_streams(hostcheck, restated, tmp_path):
    """A subset of the cases (every property, the three element sizes, one and many rows) through df_piece, df_step_tokens,
    df_build_table and DfBits as a stand-alone program: the restatement's streams and counts, a clean exit."""
    names = {"tenths_n1", "flags_n2", "tobs_n3", "tenths_n63", "tobs_n64", "flags_n65", "tenths_n257", "tobs_n16385", "flags_n16383",
             "tenths_n25203", "tenths_1row", "tobs_65rows", "fill_f4", "fill_i2", "fill_u1", "random_uint8_n1", "random_uint32_n3",
             "random_uint16_n257", "random_uint32_n25203", "nan_negzero", "no_equal_uint32", "one_symbol_plane", "runs", "halving",
             "mixed"}
    done = set()
    for case, want in restated:
        if case["name"] not in names:
            continue
        rows = case["rows"]
        src, dst = tmp_path / (case["name"] + ".in"), tmp_path / (case["name"] + ".out")
        with open(src, "wb") as fh:
            fh.write(np.array([rows.shape[0], rows.shape[1], rows.dtype.itemsize], np.int64).tobytes())
            fh.write(rows.tobytes())
        res = subprocess.run([hostcheck, "encode", str(src), str(dst)], capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", (case["name"], res.stderr[-2000:])
        raw = dst.read_bytes()
        counts = np.frombuffer(raw, np.int64, 8)
        off = np.frombuffer(raw, np.int64, rows.shape[0] + 1, offset=64)
        data = raw[64 + 8 * (rows.shape[0] + 1):]
        assert [data[off[r]:off[r + 1]] for r in range(rows.shape[0])] == want["streams"], case["name"]
        assert counts.tolist() == [want["blocks"], want["stored"]] + want["halvings"] + [rows.nbytes, len(data)], case["name"]
        done.add(case["prop"])
    assert done == set(SC.PROPS)
