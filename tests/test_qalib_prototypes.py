"""CPU: the binding of libtwxqa.so (topowx_amd/_qalib.py) against include/twx_qa.h, without a library and without a GPU.

* the prototype table ``_qalib._PROTOTYPES`` against the header's prototypes: names, argument count, the kind of every
  argument, the return type -- and the comparison itself on a table with one wrong entry;
* the call helper ``_call`` and the timing helper ``_put_times`` against a Python callable in place of an entry;
* every public entry of the binding at the smallest inputs its validation admits, through a stand-in for the library that
  records what it is called with: as many arguments as the header has, a Python int / float / address where the header has
  an integer / a floating-point number / a pointer, and in ``timing`` exactly the keys the entry promises, assigned or
  accumulated over two calls as the entry promises.

``run_entries`` returns the record of that last part as plain data, so that two versions of the binding can be compared."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from topowx_amd import _qalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}


def header_prototypes():
    """{name: (return kind, [argument kind])} of every ``twx<unit>_<name>(...)`` prototype of include/twx_qa.h; a kind is a
    key of ``SCALAR``, "pointer" or (a return only) "void"."""
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    h = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", h, flags=re.S))

    def kind(decl, with_name):
        decl = " ".join(decl.replace("const", " ").split())
        if "*" in decl:
            return "pointer"
        return decl.rsplit(" ", 1)[0] if with_name else decl

    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \*]*?)\b(twx[a-z]+_\w+)\s*\(([^;{()]*)\)\s*;", h, flags=re.M):
        assert name not in out, name
        out[name] = (kind(ret, False), [kind(p, True) for p in params.split(",")])
    return out


def is_pointer_type(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def table_mismatches(table, protos):
    """What differs between a prototype table and the header, one line per difference, each with the name and position."""
    bad = ["%s: only in the %s" % (n, "table" if n in table else "header") for n in sorted(set(table) ^ set(protos))]
    for name in sorted(set(table) & set(protos)):
        (restype, argtypes), (ret, kinds) = table[name], protos[name]
        if not (restype is None if ret == "void" else is_pointer_type(restype) if ret == "pointer" else restype is SCALAR[ret]):
            bad.append("%s: returns %s, the table has %r" % (name, ret, restype))
        if len(argtypes) != len(kinds):
            bad.append("%s: %d arguments, the table has %d" % (name, len(kinds), len(argtypes)))
            continue
        for i, (t, k) in enumerate(zip(argtypes, kinds)):
            if not (is_pointer_type(t) if k == "pointer" else t is SCALAR[k]):
                bad.append("%s: argument %d is %s, the table has %s" % (name, i, k, getattr(t, "__name__", t)))
    return bad


PROTOS = header_prototypes()


def test_the_table_is_the_header():
    assert len(PROTOS) == 45 and PROTOS["twxgh_host_free"] == ("void", ["pointer"])
    assert PROTOS["twxsc_series_check"][1][3:7] == ["pointer", "float", "double", "double"]
    assert table_mismatches(_qalib._PROTOTYPES, PROTOS) == []
    t = _qalib._PROTOTYPES
    assert t["twxgh_host_alloc"][0] is C.c_void_p and t["twxgh_host_free"][0] is None and t["twxmo_destroy"][0] is None
    assert t["twxmo_last_error"][0] is C.c_char_p and t["twxmo_deflate"][1][3] is C.POINTER(_qalib.TwxmoStreams)
    exports = [n for k in sorted(vars(_qalib)) if k == "EXPORTS" or k.endswith("_EXPORTS") for n in getattr(_qalib, k)]
    assert sorted(exports) == sorted(t)


def test_the_comparison_can_fail():
    wrong = dict(_qalib._PROTOTYPES)
    restype, argtypes = wrong["twxsc_series_check"]
    wrong["twxsc_series_check"] = (restype, argtypes[:5] + [C.c_float] + argtypes[6:])       # pen is a double
    wrong["twxhm_obs_cnt"] = (restype, wrong["twxhm_obs_cnt"][1][:-1])
    wrong["twxgh_host_free"] = (C.c_int, [C.c_int64])
    del wrong["twxqa_spatial_nmonths"]
    wrong["twxqa_nothing"] = (C.c_int, [])
    assert table_mismatches(wrong, PROTOS) == [
        "twxqa_nothing: only in the table", "twxqa_spatial_nmonths: only in the header",
        "twxgh_host_free: returns void, the table has %r" % C.c_int,
        "twxgh_host_free: argument 0 is pointer, the table has %s" % C.c_int64.__name__,
        "twxhm_obs_cnt: 13 arguments, the table has 12",
        "twxsc_series_check: argument 5 is double, the table has c_float"]


def test_load_names_the_export_a_stale_library_lacks(monkeypatch):
    stale = types.SimpleNamespace(**{n: (lambda *a: 0) for n in _qalib._PROTOTYPES if n != "twxtz_locate"})
    monkeypatch.setattr(_qalib, "_LIB", None)
    monkeypatch.setattr(_qalib, "LIB_PATH", __file__)
    monkeypatch.setattr(C, "CDLL", lambda path: stale)
    with pytest.raises(_qalib.QaError, match=r"twxtz_locate.*\./build\.sh"):
        _qalib.load()
    assert _qalib._LIB is None


def test_call_and_timing_helpers(monkeypatch):
    seen = []

    def entry(a, b, counts, kernel_ms, errbuf, errlen):
        seen.append((a, b, errlen))
        (C.c_float * 3).from_address(kernel_ms)[:] = [1.5, 2.5, 3.5]
        (C.c_int32 * 2).from_address(counts)[:] = [4, 5]
        errbuf.value = b"the message"
        return entry.rc

    def plain(a, kernel_ms, errbuf, errlen):
        (C.c_float * 1).from_address(kernel_ms)[0] = 0.25
        return 0

    monkeypatch.setattr(_qalib, "_LIB", types.SimpleNamespace(twxzz_entry=entry, twxzz_plain=plain))
    entry.rc = 0
    counts = np.zeros(2, np.int32)
    ms = _qalib._call("twxzz_entry", (7, None), 3, counts)
    assert ms == [1.5, 2.5, 3.5] and all(type(v) is float for v in ms) and counts.tolist() == [4, 5] and seen == [(7, None, 512)]
    assert _qalib._call("twxzz_plain", [1], 1) == [0.25]
    keys = ("a_kernel_ms", None, "c_ms")
    assert _qalib._ms_keys(("a", "b"), ("c",)) == ("a_kernel_ms", "b_kernel_ms", "c_ms")
    # assign: the dict describes the last call
    timing = {"other": 1}
    for _ in range(2):
        _qalib._put_times(timing, keys, ms, z_rounds=int(counts[0]))
    assert timing == {"other": 1, "a_kernel_ms": 1.5, "c_ms": 3.5, "z_rounds": 4}
    # accumulate: the sums over the calls
    timing = {}
    for _ in range(2):
        _qalib._put_times(timing, keys, ms, add=True, z_batches=int(counts[1]), z_calls=1)
    assert timing == {"a_kernel_ms": 3.0, "c_ms": 7.0, "z_batches": 10, "z_calls": 2}
    assert type(timing["a_kernel_ms"]) is float and type(timing["z_calls"]) is int
    assert _qalib._put_times(None, keys, ms) is None and _qalib._put_times(None, keys, ms, add=True, z_calls=1) is None
    # a return value that is not expected raises with the entry's name and the library's message
    entry.rc = 1
    with pytest.raises(_qalib.QaError) as e:
        _qalib._call("twxzz_entry", (7, None), 3, counts)
    assert str(e.value) == "twxzz_entry failed: the message"
    assert _qalib._call("twxzz_entry", (7, None), 3, counts, ok=(0, 1)) == [1.5, 2.5, 3.5]


# ---- every public entry through a stand-in for the library ----
I32, I64 = C.c_int32, C.c_int64
# export -> (floats of kernel_ms, type and number of counts): what the stand-in writes through the tail of a timed entry
TAILS = {"twxqa_outlier_wls": (1, None, 0), "twxqa_spatial_regress": (2, None, 0), "twxqa_doy_norms": (1, None, 0),
         "twxqa_spatial_only": (6, None, 0), "twxqa_non_spatial": (8, None, 0), "twxif_infill_matrix": (6, I32, 1),
         "twxxv_infill_matrix": (6, I32, 1), "twxem_mean_variance": (4, I32, 2), "twxpp_ppca_fit": (4, I32, 2),
         "twxck_infill_check": (3, I32, 2), "twxxv_holdout": (1, None, 0), "twxxv_score": (1, None, 0),
         "twxsc_serial_complete": (4, I32, 2), "twxsc_series_check": (4, I32, 2), "twxnr_components": (5, None, 0),
         "twxhm_obs_cnt": (4, I32, 2), "twxhm_monthly_means": (4, I32, 2), "twxhm_tobs_shift": (4, I32, 2),
         "twxhm_homog_daily": (4, I32, 2), "twxrv_sample": (3, None, 0), "twxrv_nearest_data": (3, None, 0),
         "twxrv_dup_classes": (3, None, 0), "twxrv_col_count": (3, I32, 2), "twxpq_non_spatial": (7, None, 0),
         "twxpq_percentiles": (1, None, 0), "twxpc_spatial_corrob": (4, None, 0), "twxpc_pors_counts": (1, None, 0),
         "twxgh_parse_dly": (4, I64, 3), "twxgh_parse_tobs": (4, I64, 5), "twxns_subset": (3, I64, 3),
         "twxtz_locate": (5, I64, 4)}


def describe(name, args):
    """The arguments of one call as text: the value of a scalar, the kind of thing a pointer is (addresses differ from run to
    run)."""
    out = []
    for k, a in zip(PROTOS[name][1], args):
        out.append(repr(a) if k != "pointer" or a is None or isinstance(a, bytes) else
                   "address" if type(a) is int else type(a).__name__)
    return out


class StandIn(object):
    """In place of the loaded library: every export is a Python function that records its arguments, writes 1, 2, ... through
    ``kernel_ms`` and ``counts`` of a timed entry (``TAILS``) and returns 0.  The few entries whose result the binding reads
    before it returns write that, too.  The functions take attributes, as those of ``ctypes.CDLL`` do."""

    def __init__(self):
        self.calls, self.keep, self.fail = [], [], None

    def __getattr__(self, name):
        if name not in PROTOS:
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.answer(name, args)
        fn.__name__ = name
        self.__dict__[name] = fn
        return fn

    def answer(self, name, args):
        if name == self.fail:
            return 1
        if name in TAILS:
            ntimes, ctype, ncounts = TAILS[name]
            (C.c_float * ntimes).from_address(args[-3])[:] = [float(k + 1) for k in range(ntimes)]
            if ncounts:
                (ctype * ncounts).from_address(args[-4])[:] = list(range(1, ncounts + 1))
        if name == "twxqa_spatial_nmonths":
            return 1
        if name == "twxrv_nearest_data":                          # one start, and no winner to decide again on the host
            I32.from_address(args[15]).value = _qalib.RV_NO_DATA_ANYWHERE
        if name == "twxgh_host_alloc":
            self.keep.append(C.create_string_buffer(args[0]))
            return C.addressof(self.keep[-1])
        if name == "twxmo_last_error":
            return b"the object's message"
        if name == "twxmo_create":
            args[6]._obj.value = 1
        if name == "twxmo_staging":
            self.keep.append(C.create_string_buffer(args[1]))
            args[2]._obj.value = C.addressof(self.keep[-1])
        if name == "twxmo_deflate":                               # one stream of one byte
            s = args[3]._obj
            self.keep += [(I64 * 2)(0, 1), C.create_string_buffer(1)]
            s.offset, s.data, s.nstreams, s.slot_bytes = self.keep[-2], C.addressof(self.keep[-1]), 1, 1
        return None if PROTOS[name][0] == "void" else 0


def _keys(kernels=(), host=(), *more):
    return {k + "_kernel_ms" for k in kernels} | {h + "_ms" for h in host} | set(more)


def entries(q):
    """[(label, exports called, call(timing), the keys of ``timing`` or None, accumulate?)] at 2 stations x 31 days, one target,
    one item with one column and one extra column, a 2 x 2 raster."""
    ymd = np.arange(20000101, 20000132, dtype=np.int32)
    lon, lat = np.array([-110.0, -109.5]), np.array([45.0, 45.5])
    obs = np.zeros((2, 31), np.float32)
    grp, one = np.zeros(31, np.int8), np.zeros((1, 31), np.float32)
    sets = [(0, np.zeros((31, 1)))]
    first, nd = np.array([0], np.int32), np.array([31], np.int32)
    raster, geo_t = np.zeros((2, 2), np.float32), [-111.0, 1.0, 0.0, 46.0, 0.0, -1.0]
    box = np.array([[0, 0, 1, 0], [1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 0, 0]], np.float64)
    hm = _keys((), ("hm_upload", "hm_download"), "hm_batches", "hm_calls")
    rv = _keys((), ("rv_upload", "rv_download"), "rv_calls")
    return [
        ("outlier_wls", ["twxqa_outlier_wls"], lambda t: q.outlier_wls(
            lon, lat, lon, np.zeros((13, 2)), np.zeros((13, 2)), np.zeros((1, 29)), np.zeros((1, 1), np.int32), np.ones((1, 1)),
            [0], timing=t), {"kernel_ms"}, False),
        ("spatial_nmonths", ["twxqa_spatial_nmonths"], lambda t: q.spatial_nmonths(ymd), None, False),
        ("spatial_regress", ["twxqa_spatial_nmonths", "twxqa_spatial_regress"], lambda t: q.spatial_regress(
            lon, lat, obs, obs, ymd, [0], details=True, timing=t), {"radius_kernel_ms", "regress_kernel_ms"}, False),
        ("doy_norms", ["twxqa_doy_norms"], lambda t: q.doy_norms(obs, ymd, timing=t), {"kernel_ms"}, False),
        ("spatial_only", ["twxqa_spatial_only"], lambda t: q.spatial_only(lon, lat, obs, obs, ymd, [0], timing=t),
         _keys(q.SPATIAL_ONLY_KERNELS), False),
        ("non_spatial", ["twxqa_non_spatial"], lambda t: q.non_spatial(obs, obs, ymd, details=True, timing=t),
         _keys(q.NON_SPATIAL_KERNELS), False),
        ("infill_matrix", ["twxif_infill_matrix"], lambda t: q.infill_matrix(
            lon, lat, obs, ymd, [1, 1], [0], grp, [1], [[1]], timing=t),
         _keys(q.INFILL_MATRIX_KERNELS, q.INFILL_MATRIX_HOST_TIMES, "rounds"), False),
        ("infill_matrix(exclude_idx)", ["twxxv_infill_matrix"], lambda t: q.infill_matrix(
            lon, lat, obs, ymd, [1, 1], [0], grp, [1], [[1]], timing=t, exclude_idx=[-1]),
         _keys(q.INFILL_MATRIX_KERNELS, q.INFILL_MATRIX_HOST_TIMES, "rounds"), False),
        ("em_mean_variance", ["twxem_mean_variance"], lambda t: q.em_mean_variance(
            obs, grp, [0], [0], [0, 1], [1], sets=sets, item_set=[0], matrix_status=[0], full=True, timing=t),
         _keys(q.EM_KERNELS, q.EM_HOST_TIMES, "em_rounds", "em_batches"), False),
        ("ppca_fit", ["twxpp_ppca_fit"], lambda t: q.ppca_fit(
            obs, grp, [0], [0], [1], [0, 1], [1], np.zeros(3), np.ones(3), sets=sets, item_set=[0], full=True, timing=t),
         _keys(q.PP_KERNELS, q.PP_HOST_TIMES, "pp_rounds", "pp_batches", "pp_calls"), True),
        ("infill_check", ["twxck_infill_check"], lambda t: q.infill_check([0, 1], [0.0], [0.0], timing=t),
         _keys(q.CK_KERNELS, q.CK_HOST_TIMES, "ck_batches", "ck_calls"), True),
        ("holdout", ["twxxv_holdout"], lambda t: q.holdout(obs, [0], 1, timing=t), {"xv_holdout_kernel_ms"}, False),
        ("xval_score", ["twxxv_score"], lambda t: q.xval_score(np.zeros((1, 31)), one, one != 0, grp, timing=t),
         {"xv_score_kernel_ms"}, False),
        ("serial_complete", ["twxsc_serial_complete"], lambda t: q.serial_complete(
            one, one, np.zeros((1, 31), np.int8), group_first=first, group_ndays=nd, timing=t),
         _keys(q.SC_KERNELS, q.SC_HOST_TIMES, "sc_batches", "sc_calls"), True),
        ("series_check", ["twxsc_series_check"], lambda t: q.series_check(one, timing=t),
         {"sc_series_kernel_ms", "sc_series_upload_ms", "sc_series_download_ms", "sc_series_batches", "sc_series_calls"}, True),
        ("nnr_components_batched", ["twxnr_components"], lambda t: q.nnr_components_batched(one, [0, 1], [0], grp, timing=t),
         _keys(q.NR_KERNELS, q.NR_HOST_TIMES, "nr_calls"), True),
        ("obs_cnt", ["twxhm_obs_cnt"], lambda t: q.obs_cnt(obs, np.ones(31, np.int8), 0, 30, timing=t),
         hm | {"hm_cnt_kernel_ms"}, True),
        ("monthly_means", ["twxhm_monthly_means"], lambda t: q.monthly_means(obs, first, nd, timing=t),
         hm | {"hm_means_kernel_ms"}, True),
        ("tobs_shift", ["twxhm_tobs_shift"], lambda t: q.tobs_shift(obs, obs, timing=t), hm | {"hm_tobs_kernel_ms"}, True),
        ("homog_daily", ["twxhm_homog_daily"], lambda t: q.homog_daily(
            obs, np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int16), np.zeros((2, 1), np.int32), [20000101], first, nd,
            [0, 0, 0], [], [], [], timing=t), hm | {"hm_delta_kernel_ms", "hm_apply_kernel_ms"}, True),
        ("raster_sample", ["twxrv_sample"], lambda t: q.raster_sample(raster, geo_t, -1.0, lon[:1], lat[:1], timing=t),
         rv | {"rv_sample_kernel_ms"}, True),
        ("raster_nearest_data", ["twxrv_nearest_data"], lambda t: q.raster_nearest_data(raster, geo_t, -1.0, [0], [0], timing=t),
         rv | {"rv_ring_kernel_ms"}, True),
        ("dup_classes", ["twxrv_dup_classes"], lambda t: q.dup_classes(lon, lat, timing=t), rv | {"rv_dup_kernel_ms"}, True),
        ("col_count", ["twxrv_col_count"], lambda t: q.col_count(np.zeros((31, 2), np.int8), timing=t),
         rv | {"rv_colcount_kernel_ms", "rv_batches"}, True),
        ("prcp_non_spatial", ["twxpq_non_spatial"], lambda t: q.prcp_non_spatial(obs, obs, ymd, details=True, timing=t),
         _keys(q.PQ_KERNELS), False),
        ("prcp_percentiles", ["twxpq_percentiles"], lambda t: q.prcp_percentiles(obs, ymd, timing=t),
         {"pq_pctiles_kernel_ms"}, False),
        ("prcp_spatial_corrob", ["twxpc_spatial_corrob"], lambda t: q.prcp_spatial_corrob(
            lon, lat, obs, ymd, [0], np.ones((1, 31), np.uint8), details=True, timing=t), _keys(q.PC_KERNELS), False),
        ("prcp_pors_counts", ["twxpc_pors_counts"], lambda t: q.prcp_pors_counts(obs, ymd, timing=t),
         {"pc_rowcounts_kernel_ms"}, False),
        ("ghcn_parse_dly", ["twxgh_parse_dly"], lambda t: q.ghcn_parse_dly(
            b"abcd", [0, 4], [0], 1, 20000101, 20000131, 31, timing=t), _keys(q.GH_KERNELS), True),
        ("ghcn_parse_tobs", ["twxgh_parse_tobs"], lambda t: q.ghcn_parse_tobs(
            b"abcd", [0, 4], [b"USC00000001"], "TOBS", 20000101, 20000131, 0, np.zeros((1, 1), np.int16), timing=t),
         _keys(q.GH_KERNELS), True),
        ("PinnedBuffer", ["twxgh_host_alloc", "twxgh_host_free"], lambda t: q.PinnedBuffer(8).close(), None, False),
        ("ns_subset", ["twxns_subset"], lambda t: q.ns_subset(
            np.zeros((1, 1, 2, 2), np.int16), 1.0, 0.0, (None, None), [0], [0], 1, [0, 1], [0, 1], [dict(slot=0, levels=[0])],
            timing=t), _keys((), q.NS_KERNELS), True),
        ("tz_locate", ["twxtz_locate"], lambda t: q.tz_locate([0.5], [0.5], [0, 4], [[0, 0, 1, 1]], box, timing=t),
         _keys((), q.TZ_PHASES, "tz_calls"), True),
        ("mosaic_sizes", ["twxmo_sizes"], lambda t: q.mosaic_sizes(1, 2, 2, 2, 2), None, False),
        ("Mosaic", ["twxmo_sizes", "twxmo_create", "twxmo_clear", "twxmo_staging", "twxmo_place", "twxmo_monthly",
                    "twxmo_deflate", "twxmo_download", "twxmo_timing", "twxmo_destroy"], lambda t: _mosaic(q), None, False),
    ]


def _mosaic(q):
    with q.Mosaic(1, 2, 2, 2, 2) as m:
        m.clear(1)
        m.staging((1, 2, 2))
        m.place(np.zeros((1, 2, 2), np.int16), 0, 0)
        m.monthly(1, [1])
        m.deflate(1)
        m.download(1)
        m.timing()


def run_entries(q):
    """Every entry of ``entries(q)`` twice into one ``timing`` dict, the library replaced by a ``StandIn``: a list of
    (label, [(export, described arguments)], timing after the first call, timing after the second)."""
    lib, saved, out = StandIn(), q._LIB, []
    q._LIB = lib
    try:
        for label, exports, call, keys, add in entries(q):
            del lib.calls[:]
            timing = {}
            call(None)                                            # no dict: nothing to write to, and nothing raises
            ncalls = len(lib.calls)
            call(timing)
            once = dict(timing)
            call(timing)
            out.append((label, [(n, describe(n, a)) for n, a in lib.calls[ncalls:2 * ncalls]], once, dict(timing)))
            assert [n for n, _ in lib.calls] == exports * 3, label
            for name, args in lib.calls:
                assert len(args) == len(PROTOS[name][1]), (label, name)
                for i, (k, a) in enumerate(zip(PROTOS[name][1], args)):
                    if k in ("float", "double"):
                        ok = type(a) is float
                    elif k != "pointer":
                        ok = type(a) is int
                    else:   # an address, nothing, a ctypes buffer or a reference to one; bytes for a ``const char *`` string
                        ok = a is None or type(a) in (int, bytes, type(C.byref(I32()))) or \
                            isinstance(a, (C.Array, C.Structure, C._SimpleCData))
                    assert ok, "%s: argument %d of %s (%s) is %r" % (label, i, name, k, a)
    finally:
        q._LIB = saved
    return out


def test_every_entry_through_a_stand_in():
    record = run_entries(_qalib)
    spec = {label: (keys, add) for label, _, _, keys, add in entries(_qalib)}
    assert sorted({n for _, calls, _, _ in record for n, _ in calls} | {"twxmo_last_error"}) == sorted(PROTOS)
    for label, calls, once, twice in record:
        keys, add = spec[label]
        assert set(once) == set(twice) == (keys or set()), label
        for k, v in once.items():
            assert v > 0 and twice[k] == (2 * v if add else v), (label, k)
            assert type(v) is (float if k.endswith("_ms") else int), (label, k)
    # the times arrive in the order of the entry's tuples; the counters are the entry's counts, or the number of calls
    by = {label: once for label, _, once, _ in record}
    assert [by["spatial_only"][k + "_kernel_ms"] for k in _qalib.SPATIAL_ONLY_KERNELS] == [1, 2, 3, 4, 5, 6]
    assert (by["em_mean_variance"]["em_rounds"], by["em_mean_variance"]["em_batches"]) == (1, 2)
    assert by["em_mean_variance"]["em_download_ms"] == 4 and by["infill_matrix"]["rounds"] == 1
    assert by["ppca_fit"] == dict(pp_prep_kernel_ms=1, pp_iter_kernel_ms=2, pp_upload_ms=3, pp_download_ms=4, pp_rounds=1,
                                  pp_batches=2, pp_calls=1)
    assert by["series_check"] == dict(sc_series_kernel_ms=1, sc_series_upload_ms=3, sc_series_download_ms=4,
                                      sc_series_batches=2, sc_series_calls=1)
    assert by["obs_cnt"] == dict(hm_cnt_kernel_ms=1, hm_upload_ms=3, hm_download_ms=4, hm_batches=2, hm_calls=1)
    assert by["homog_daily"]["hm_delta_kernel_ms"] == 1 and by["homog_daily"]["hm_apply_kernel_ms"] == 2
    assert by["col_count"] == dict(rv_colcount_kernel_ms=1, rv_upload_ms=2, rv_download_ms=3, rv_calls=1, rv_batches=2)
    assert by["tz_locate"]["tz_download_ms"] == 5 and by["tz_locate"]["tz_calls"] == 1


def test_a_failing_entry_raises_with_its_name(monkeypatch):
    lib = StandIn()
    monkeypatch.setattr(_qalib, "_LIB", lib)
    lib.fail = "twxhm_tobs_shift"
    with pytest.raises(_qalib.QaError, match="^twxhm_tobs_shift failed: $"):
        _qalib.tobs_shift(np.zeros((2, 31), np.float32), np.zeros((2, 31), np.float32), timing={})
    lib.fail = "twxmo_clear"
    with _qalib.Mosaic(1, 2, 2, 2, 2) as m:
        with pytest.raises(_qalib.QaError, match="^twxmo_clear failed: the object's message$"):
            m.clear(1)
    assert [n for n, _ in lib.calls][-3:] == ["twxmo_clear", "twxmo_last_error", "twxmo_destroy"]
    lib.fail = "twxmo_sizes"
    with pytest.raises(ValueError):
        _qalib.mosaic_sizes(1, 2, 2, 2, 2)
