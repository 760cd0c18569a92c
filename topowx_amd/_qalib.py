"""ctypes binding of libtwxqa.so (include/twx_qa.h): the station QA kernels that run before the interpolation stages.

Like ``_lib`` there is NO CPU fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtwxqa.so")

NTARGET = 13              # TWXQA_NTARGET: 12 monthly normals + the annual one
PT_STRIDE = 29            # TWXQA_PT_STRIDE: lon, lat, elev, lst[13], norm[13]
MAX_K = 159               # TWXQA_MAX_K
STATUS_OK, STATUS_FEW_STATIONS, STATUS_SINGULAR = 0, 1, 4     # TWX_CELL_* numbers (include/twx.h)
EXPORTS = ("twxqa_outlier_wls", "twxqa_spatial_nmonths", "twxqa_spatial_regress", "twxqa_doy_norms", "twxqa_spatial_only",
           "twxqa_non_spatial")
# the spatial regression check (TWXQA_SP_* / TWXQA_* of include/twx_qa.h)
MAX_RADIUS_NGH = 256      # TWXQA_MAX_RADIUS_NGH
SP_OK, SP_FEW_NGHS, SP_DEGENERATE, SP_NGH_CAP, SP_FEW_DAYS, SP_FEW_VALID = 0, 1, 4, 7, 16, 17
# the normals and the corroboration check
ANOMALY_CUTOFF = 10.0     # TWXQA_ANOMALY_CUTOFF
MIN_NORM_VALUES = 100     # TWXQA_MIN_NORM_VALUES
NORM_ROWS = 731           # TWXQA_NORM_ROWS: the 365-row table, then the 366-row table
MAX_NORM_VALUES = 2048    # TWXQA_MAX_NORM_VALUES
SPATIAL_ONLY_KERNELS = ("regress_radius", "regress_items", "radius_dist", "doy_norms", "corrob", "mega_final")
# the non-spatial checks
MAX_GAP_VALUES = 4096     # TWXQA_MAX_GAP_VALUES: 31 values per year of the series
NON_SPATIAL_KERNELS = ("init", "dups", "streak", "gap", "norms", "clim", "spike_lagrange", "mega")     # TWXQA_NS_NKERNELS

_LIB = None


class QaError(RuntimeError):
    pass


class TwxmoStreams(C.Structure):
    """twxmo_streams (include/twx_qa.h)."""
    _fields_ = [("data", C.c_void_p), ("offset", C.POINTER(C.c_int64)), ("nstreams", C.c_int64), ("slot_bytes", C.c_int64),
                ("nchunk", C.c_int32), ("chunk_y", C.c_int32), ("chunk_x", C.c_int32), ("reserved", C.c_int32)]


# Every export of include/twx_qa.h: name -> (restype, argtypes).  ``load`` applies the table once;
# tests/test_qalib_prototypes.py compares it with the header's prototypes.
_ERR = [C.c_char_p, C.c_int]          # errbuf, errlen
_PROTOTYPES = {
    "twxqa_outlier_wls": (C.c_int, [C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int32] +
                          [C.c_void_p] * 6 + _ERR),
    "twxqa_spatial_nmonths": (C.c_int, [C.c_int64, C.c_void_p]),
    "twxqa_spatial_regress": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64] +
                              [C.c_void_p] * 8 + _ERR),
    "twxqa_doy_norms": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + _ERR),
    "twxqa_spatial_only": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 6 + _ERR),
    "twxqa_non_spatial": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 7 + _ERR),
    "twxif_infill_matrix": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int32] +
                            [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 8 + _ERR),
    "twxem_mean_variance": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] +
                            [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 4 +
                            [C.c_double, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 9 + _ERR),
    "twxpp_ppca_fit": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] +
                       [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 7 + [C.c_double, C.c_int32, C.c_int32, C.c_int64] +
                       [C.c_void_p] * 9 + _ERR),
    "twxck_infill_check": (C.c_int, [C.c_int, C.c_int64] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_int64] +
                           [C.c_void_p] * 10 + _ERR),
    "twxxv_holdout": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32] +
                      [C.c_void_p] * 5 + _ERR),
    "twxxv_infill_matrix": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 5 +
                            [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4 +
                            [C.c_int64] + [C.c_void_p] * 8 + _ERR),
    "twxxv_score": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 10 + _ERR),
    "twxsc_serial_complete": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32, C.c_float, C.c_int32] +
                              [C.c_void_p] * 2 + [C.c_int32, C.c_int64] + [C.c_void_p] * 9 + _ERR),
    "twxsc_series_check": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_float] + [C.c_double] * 3 + [C.c_int64] +
                           [C.c_void_p] * 8 + _ERR),
    "twxnr_components": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 11 + [C.c_int64] +
                         [C.c_void_p] * 2 + _ERR),
    "twxhm_obs_cnt": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_int64] * 3 +
                      [C.c_void_p] * 3 + _ERR),
    "twxhm_monthly_means": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_void_p] * 2 + _ERR),
    "twxhm_tobs_shift": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p] + [C.c_void_p] * 2 + _ERR),
    "twxhm_homog_daily": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 10 +
                          [C.c_int64] + [C.c_void_p] * 4 + [C.c_void_p] * 2 + _ERR),
    "twxrv_sample": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                               C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] +
                     [C.c_void_p] * 5 + _ERR),
    "twxrv_nearest_data": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                     C.c_int64] + [C.c_void_p] * 9 + _ERR),
    "twxrv_dup_classes": (C.c_int, [C.c_int, C.c_int64] + [C.c_void_p] * 5 + _ERR),
    "twxrv_col_count": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_int64, C.c_void_p,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + _ERR),
    "twxpq_non_spatial": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32, C.c_int32] +
                          [C.c_void_p] * 3 + _ERR),
    "twxpq_percentiles": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + _ERR),
    "twxpc_spatial_corrob": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] +
                             [C.c_void_p] * 7 + _ERR),
    "twxpc_pors_counts": (C.c_int, [C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + _ERR),
    "twxgh_parse_dly": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p] + _ERR),
    "twxgh_parse_tobs": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_char_p,
                                   C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p] + _ERR),
    "twxgh_host_alloc": (C.c_void_p, [C.c_int64]),
    "twxgh_host_free": (None, [C.c_void_p]),
    "twxns_subset": (C.c_int, [C.c_int, C.c_int, C.c_void_p] + [C.c_int64] * 4 + [C.c_float, C.c_float] + [C.c_void_p] * 4 +
                     [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int] +
                     [C.c_void_p] * 3 + _ERR),
    "twxtz_locate": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] +
                     _ERR),
    "twxmo_sizes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p] + _ERR),
    "twxmo_create": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p] + _ERR),
    "twxmo_destroy": (None, [C.c_void_p]),
    "twxmo_last_error": (C.c_char_p, [C.c_void_p]),
    "twxmo_clear": (C.c_int, [C.c_void_p, C.c_int64]),
    "twxmo_place": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "twxmo_staging": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "twxmo_monthly": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "twxmo_deflate": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.POINTER(TwxmoStreams)]),
    "twxmo_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "twxmo_timing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def load():
    """Load libtwxqa.so and give every export its prototype; raises if the library has not been built or lacks an export
    (no fallback).  An entry that reports a missing build before it looks at its arguments calls this first; the others
    check their arguments first and load in ``_call``."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise QaError("%s not found: build it with ./build.sh (hipcc --offload-arch=gfx950); "
                          "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            if not hasattr(L, name):
                raise QaError("%s has no %s: it is older than this binding, run ./build.sh" % (LIB_PATH, name))
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def _call(name, args, ntimes, counts=None, ok=(0,)):
    """Call the entry ``name`` with ``args`` and the tail the timed entries end in -- ``counts`` (a numpy array, if the entry
    has one), kernel_ms [ntimes], errbuf, errlen.  Returns the times; a return value outside ``ok`` raises ``QaError``."""
    ms = (C.c_float * ntimes)()
    buf = C.create_string_buffer(512)
    tail = (C.addressof(ms), buf, 512)
    if counts is not None:
        tail = (counts.ctypes.data,) + tail
    if getattr(load(), name)(*(tuple(args) + tail)) not in ok:
        raise QaError("%s failed: %s" % (name, buf.value.decode(errors="replace")))
    return [float(v) for v in ms]


def _ms_keys(kernels, host=()):
    return tuple(k + "_kernel_ms" for k in kernels) + tuple(h + "_ms" for h in host)


def _put_times(timing, keys, ms, add=False, **ints):
    """Put the times ``ms`` into ``timing`` (a dict, or None: nothing happens) under ``keys`` (None skips a slot), then the
    integer counters ``ints``.  ``add`` False assigns: the dict describes the last call; True accumulates over calls."""
    if timing is None:
        return
    for key, v in list(zip(keys, ms)) + list(ints.items()):
        if key is not None:
            timing[key] = timing.get(key, 0) + v if add else v


def outlier_wls(lon, lat, elev, lst13, norm13, pt, idx, wgt, knn_status, device=0, timing=None):
    """``twxqa_outlier_wls``: leave-one-out WLS errors of ``XvalOutlier.run_xval_stn`` (optimize.py:113-153).

    lon, lat, elev [nstn], lst13 / norm13 [13, nstn]: the pool (row 12 = annual means); pt [npts, 29]: the left-out
    stations; idx / wgt [npts, k] and knn_status [npts]: their neighbours as ``_lib.Context.knn`` returns them.
    Returns (err [npts, 13], status [npts, 13]); ``timing`` (a dict) receives the kernel's device time as ``kernel_ms``."""
    load()
    lon, lat, elev = (_c(a, np.float64) for a in (lon, lat, elev))
    nstn = lon.size
    lst13, norm13 = _c(lst13, np.float64), _c(norm13, np.float64)
    pt = _c(pt, np.float64)
    idx, wgt = _c(idx, np.int32), _c(wgt, np.float64)
    knn_status = _c(knn_status, np.int32)
    if pt.ndim != 2 or pt.shape[1] != PT_STRIDE:
        raise ValueError("pt must be [npts, %d]" % PT_STRIDE)
    npts = pt.shape[0]
    if lat.size != nstn or elev.size != nstn or lst13.shape != (NTARGET, nstn) or norm13.shape != (NTARGET, nstn):
        raise ValueError("pool columns must be [nstn] and [13, nstn]")
    if idx.ndim != 2 or idx.shape[0] != npts or wgt.shape != idx.shape or knn_status.shape != (npts,):
        raise ValueError("idx / wgt must be [npts, k] and knn_status [npts]")
    k = idx.shape[1]
    err = np.empty((npts, NTARGET))
    status = np.empty((npts, NTARGET), np.int32)
    ms = _call("twxqa_outlier_wls", (int(device), nstn, lon.ctypes.data, lat.ctypes.data, elev.ctypes.data, lst13.ctypes.data,
                                     norm13.ctypes.data, npts, pt.ctypes.data, k, idx.ctypes.data, wgt.ctypes.data,
                                     knn_status.ctypes.data, err.ctypes.data, status.ctypes.data), 1)
    _put_times(timing, ("kernel_ms",), ms)
    return err, status


def spatial_nmonths(ymd):
    """``twxqa_spatial_nmonths``: the number of (year, month) items of a day axis."""
    ymd = _c(ymd, np.int32)
    n = load().twxqa_spatial_nmonths(ymd.size, ymd.ctypes.data)
    if n < 1:
        raise ValueError("ymd must hold at least one day, in ascending order")
    return int(n)


def _sp_inputs(lon, lat, tmin, tmax, ymd, target_idx):
    """The inputs of ``spatial_regress`` and ``spatial_only``, converted and checked."""
    lon, lat = _c(lon, np.float64), _c(lat, np.float64)
    tmin, tmax = _c(tmin, np.float32), _c(tmax, np.float32)
    ymd, target_idx = _c(ymd, np.int32), _c(target_idx, np.int32)
    nstn, ndays = lon.size, ymd.size
    if lon.ndim != 1 or lat.shape != lon.shape or tmin.shape != (nstn, ndays) or tmax.shape != (nstn, ndays):
        raise ValueError("lon / lat must be [nstn] and tmin / tmax [nstn, ndays]")
    if target_idx.ndim != 1:
        raise ValueError("target_idx must be [ntarget]")
    return lon, lat, tmin, tmax, ymd, target_idx


def spatial_regress(lon, lat, tmin, tmax, ymd, target_idx, device=0, details=False, timing=None):
    """``twxqa_spatial_regress``: step08's spatial regression check (qa_temp.py:688-738, 858-1015).

    lon, lat [nstn]; tmin, tmax [nstn, ndays] float32, station-major, NaN = missing; ymd [ndays] consecutive days;
    target_idx [ntarget].  Returns (flag_tmin, flag_tmax), each uint8 [ntarget, ndays] (1 = flagged); with ``details``
    also a dict of est [ntarget, 2, ndays] and r / nvalid / status [ntarget, 2, nmonths].  ``timing`` (a dict) receives
    ``radius_kernel_ms`` and ``regress_kernel_ms``."""
    load()
    lon, lat, tmin, tmax, ymd, target_idx = _sp_inputs(lon, lat, tmin, tmax, ymd, target_idx)
    nstn, ndays, nt = lon.size, ymd.size, target_idx.size
    fmin, fmax = np.zeros((nt, ndays), np.uint8), np.zeros((nt, ndays), np.uint8)
    det, ptr = {}, [None, None, None, None]
    if details:
        nm = spatial_nmonths(ymd) if ndays else 0
        det = dict(est=np.empty((nt, 2, ndays)), r=np.empty((nt, 2, nm)), nvalid=np.empty((nt, 2, nm), np.int32),
                   status=np.empty((nt, 2, nm), np.int32))
        ptr = [det[k].ctypes.data for k in ("est", "r", "nvalid", "status")]
    ms = _call("twxqa_spatial_regress", (int(device), nstn, ndays, lon.ctypes.data, lat.ctypes.data, tmin.ctypes.data,
                                         tmax.ctypes.data, ymd.ctypes.data, nt, target_idx.ctypes.data, fmin.ctypes.data,
                                         fmax.ctypes.data, ptr[0], ptr[1], ptr[2], ptr[3]), 2)
    _put_times(timing, ("radius_kernel_ms", "regress_kernel_ms"), ms)
    return (fmin, fmax, det) if details else (fmin, fmax)


def doy_norms(series, ymd, device=0, timing=None):
    """``twxqa_doy_norms``: the two day-of-year tables of biweight means of each series (qa_temp.py:1111-1130, 1171-1184,
    1215-1228).  series [nseries, ndays] float32 (NaN = missing), ymd [ndays] consecutive days.  Returns norms
    [nseries, 731]: rows 0..364 the 365-row table, rows 365..730 the 366-row table.  ``timing`` receives ``kernel_ms``."""
    load()
    series, ymd = _c(series, np.float32), _c(ymd, np.int32)
    if series.ndim != 2 or ymd.ndim != 1 or series.shape[1] != ymd.size:
        raise ValueError("series must be [nseries, ndays] and ymd [ndays]")
    out = np.empty((series.shape[0], NORM_ROWS))
    ms = _call("twxqa_doy_norms", (int(device), series.shape[0], ymd.size, series.ctypes.data, ymd.ctypes.data,
                                   out.ctypes.data), 1)
    _put_times(timing, ("kernel_ms",), ms)
    return out


def spatial_only(lon, lat, tmin, tmax, ymd, target_idx, device=0, timing=None):
    """``twxqa_spatial_only``: regression check -> normals -> corroboration check -> mega-inconsistency check
    (``run_qa_spatial_only``, qa_temp.py:218-258), inputs as ``spatial_regress``.  Returns (flag_tmin, flag_tmax), each
    uint8 [ntarget, ndays] in the reference's numbering (1, 2, 16, 17, 18), norms [ntarget, 2, 731] (the target tables)
    and status [ntarget] (SP_OK / SP_FEW_NGHS / SP_NGH_CAP).  ``timing`` receives ``<kernel>_kernel_ms`` for the names in
    ``SPATIAL_ONLY_KERNELS``."""
    load()
    lon, lat, tmin, tmax, ymd, target_idx = _sp_inputs(lon, lat, tmin, tmax, ymd, target_idx)
    nstn, ndays, nt = lon.size, ymd.size, target_idx.size
    fmin, fmax = np.zeros((nt, ndays), np.uint8), np.zeros((nt, ndays), np.uint8)
    norms, status = np.empty((nt, 2, NORM_ROWS)), np.empty(nt, np.int32)
    ms = _call("twxqa_spatial_only", (int(device), nstn, ndays, lon.ctypes.data, lat.ctypes.data, tmin.ctypes.data,
                                      tmax.ctypes.data, ymd.ctypes.data, nt, target_idx.ctypes.data, fmin.ctypes.data,
                                      fmax.ctypes.data, norms.ctypes.data, status.ctypes.data), len(SPATIAL_ONLY_KERNELS))
    _put_times(timing, _ms_keys(SPATIAL_ONLY_KERNELS), ms)
    return fmin, fmax, norms, status


def non_spatial(tmin, tmax, ymd, device=0, details=False, timing=None):
    """``twxqa_non_spatial``: ``run_qa_non_spatial`` (qa_temp.py:172-216) of every station on its own.  tmin, tmax
    [nstn, ndays] float32, station-major, NaN = missing; ymd [ndays] consecutive days.  Returns (flag_tmin, flag_tmax),
    each uint8 [nstn, ndays] in the reference's numbering (1 .. 13, 15, 18); with ``details`` also norms
    [nstn, 2, 731, 2]: mean and standard deviation of the day-of-year rows as the outlier check used them.  ``timing``
    receives ``<kernel>_kernel_ms`` for the names in ``NON_SPATIAL_KERNELS``."""
    load()
    tmin, tmax, ymd = _c(tmin, np.float32), _c(tmax, np.float32), _c(ymd, np.int32)
    if tmin.ndim != 2 or tmax.shape != tmin.shape or ymd.ndim != 1 or tmin.shape[1] != ymd.size:
        raise ValueError("tmin / tmax must be [nstn, ndays] and ymd [ndays]")
    nstn, ndays = tmin.shape
    fmin, fmax = np.zeros((nstn, ndays), np.uint8), np.zeros((nstn, ndays), np.uint8)
    norms = np.empty((nstn, 2, NORM_ROWS, 2)) if details else None
    ms = _call("twxqa_non_spatial", (int(device), nstn, ndays, tmin.ctypes.data, tmax.ctypes.data, ymd.ctypes.data,
                                     fmin.ctypes.data, fmax.ctypes.data, norms.ctypes.data if details else None),
               len(NON_SPATIAL_KERNELS))
    _put_times(timing, _ms_keys(NON_SPATIAL_KERNELS), ms)
    return (fmin, fmax, norms) if details else (fmin, fmax)


# ---- the neighbour matrices of the infill family (twxif_infill_matrix; TWXIF_* of include/twx_qa.h) ----
IF_EXPORTS = ("twxif_infill_matrix",)
IF_OK, IF_NUMERIC, IF_NGH_CAP, IF_NO_TARGET_OBS, IF_UNSATISFIED = 0, 4, 7, 18, 19
IF_MAX_GROUPS = 12        # TWXIF_MAX_GROUPS
IF_MAX_MIN_NNGHS = 16     # TWXIF_MAX_MIN_NNGHS
IF_MAX_COLS_NORM_IMPUTE = 31    # TWXIF_MAX_COLS_NORM_IMPUTE
INFILL_MATRIX_KERNELS = ("ring", "pair", "item", "compact")     # TWXIF_NKERNELS
INFILL_MATRIX_HOST_TIMES = ("upload", "download")               # the rest of TWXIF_NTIMES: host-clock milliseconds


def infill_matrix(lon, lat, obs, ymd, eligible, target_idx, group, nthres_all, nthres_target_por, min_daily_nnghs=3,
                  device=0, timing=None, exclude_idx=None):
    """``twxif_infill_matrix``: the ranked, widened and shrunk neighbour lists of ``_InfillMatrix``
    (infill_normals.py:52-237, 324-343, 391-420) of every (target, day group) item.

    lon, lat [nstn]; obs [nstn, ndays] float32, station-major, NaN = missing; ymd [ndays] consecutive days; eligible
    [nstn] bool; target_idx [ntarget]; group [ndays] int8, -1 or 0 .. G - 1; nthres_all [G], nthres_target_por
    [ntarget, G].  Returns a dict of status, nnghs, max_dist [ntarget, G], off [ntarget * G + 1] and the CSR columns idx,
    ioa, dist, nlap, nlap_stn, keep, and ``rounds``.  ``timing`` receives ``<kernel>_kernel_ms`` for the names in
    ``INFILL_MATRIX_KERNELS``, the host-clock ``upload_ms`` / ``download_ms`` and ``rounds``.

    ``exclude_idx`` [ntarget] (-1 or a pool row that is never a neighbour of that target) picks ``twxxv_infill_matrix``, the
    same driver and kernels with that one comparison more (step15)."""
    load()
    if exclude_idx is not None:
        exclude_idx = _c(exclude_idx, np.int32)
    lon, lat, obs = _c(lon, np.float64), _c(lat, np.float64), _c(obs, np.float32)
    ymd, target_idx = _c(ymd, np.int32), _c(target_idx, np.int32)
    eligible, group = _c(eligible, np.uint8), _c(group, np.int8)
    nthres_all, nthres_target_por = _c(nthres_all, np.int32), _c(nthres_target_por, np.int32)
    nstn, ndays, nt = lon.size, ymd.size, target_idx.size
    if lon.ndim != 1 or lat.shape != lon.shape or obs.shape != (nstn, ndays) or eligible.shape != (nstn,):
        raise ValueError("lon / lat / eligible must be [nstn] and obs [nstn, ndays]")
    if target_idx.ndim != 1 or group.shape != (ndays,) or nthres_all.ndim != 1:
        raise ValueError("target_idx must be [ntarget], group [ndays] and nthres_all [ngroups]")
    ng = nthres_all.size
    if nthres_target_por.shape != (nt, ng):
        raise ValueError("nthres_target_por must be [ntarget, ngroups]")
    if exclude_idx is not None and exclude_idx.shape != (nt,):
        raise ValueError("exclude_idx must be [ntarget]")
    ni = nt * ng
    cap = ni * MAX_RADIUS_NGH                      # always enough; the pages of an empty array are not touched
    out = dict(status=np.empty((nt, ng), np.int32), nnghs=np.empty((nt, ng), np.int32), max_dist=np.empty((nt, ng)),
               off=np.zeros(ni + 1, np.int64))
    col = dict(idx=np.empty(cap, np.int32), ioa=np.empty(cap), dist=np.empty(cap), nlap=np.empty(cap, np.int32),
               nlap_stn=np.empty(cap, np.int32), keep=np.empty(cap, np.uint8))
    rounds = np.zeros(1, np.int32)
    head = (int(device), nstn, ndays, lon.ctypes.data, lat.ctypes.data, obs.ctypes.data, ymd.ctypes.data,
            eligible.ctypes.data, nt, target_idx.ctypes.data)
    rest = (ng, group.ctypes.data, nthres_all.ctypes.data, nthres_target_por.ctypes.data, int(min_daily_nnghs),
            out["status"].ctypes.data, out["nnghs"].ctypes.data, out["max_dist"].ctypes.data, out["off"].ctypes.data, cap,
            col["idx"].ctypes.data, col["ioa"].ctypes.data, col["dist"].ctypes.data, col["nlap"].ctypes.data,
            col["nlap_stn"].ctypes.data, col["keep"].ctypes.data)
    ntimes = len(INFILL_MATRIX_KERNELS) + len(INFILL_MATRIX_HOST_TIMES)
    if exclude_idx is None:
        ms = _call("twxif_infill_matrix", head + rest, ntimes, rounds)
    else:
        ms = _call("twxxv_infill_matrix", head + (exclude_idx.ctypes.data,) + rest, ntimes, rounds)
    total = int(out["off"][-1])
    for k, a in col.items():
        out[k] = a[:total].copy()
    out["rounds"] = int(rounds[0])
    # the host times: allocations + copies in, copies out
    _put_times(timing, _ms_keys(INFILL_MATRIX_KERNELS, INFILL_MATRIX_HOST_TIMES), ms, rounds=out["rounds"])
    return out


# ---- the mean / variance estimator of step14 (twxem_mean_variance; TWXEM_* of include/twx_qa.h) ----
EM_EXPORTS = ("twxem_mean_variance",)
EM_OK, EM_NUMERIC, EM_MAXITS, EM_NO_MATRIX, EM_EMPTY_COLUMN, EM_ROW_CAP = 0, 4, 20, 21, 22, 23
EM_MAX_COLS = 31          # TWXEM_MAX_COLS
EM_MAX_ROWS = 8192        # TWXEM_MAX_ROWS
EM_KERNELS = ("em_prep", "em_iter")                     # TWXEM_NKERNELS
EM_HOST_TIMES = ("em_upload", "em_download")            # the rest of TWXEM_NTIMES: host-clock milliseconds


def _pack_sets(sets, ng, nrows):
    """(set_group, set_ncol, set_vals) of ``twxem_mean_variance`` / ``twxpp_ppca_fit`` for ``sets``, a sequence of (group,
    values [days of the group, ncol]); ``nrows`` [ng]: the days of every group."""
    sets = list(sets)
    set_group, set_ncol = np.zeros(len(sets), np.int32), np.zeros(len(sets), np.int32)
    vals = []
    for s, (g, v) in enumerate(sets):
        v = np.asarray(v, np.float64)
        if v.ndim != 2 or not 0 <= int(g) < ng or v.shape[0] != nrows[int(g)]:
            raise ValueError("extra-column set %d must be [days of its group, ncol]" % s)
        set_group[s], set_ncol[s] = int(g), v.shape[1]
        vals.append(np.ascontiguousarray(v.T).ravel())              # column after column
    return set_group, set_ncol, np.concatenate(vals) if vals else np.zeros(0)


def em_mean_variance(obs, group, item_target, item_group, col_off, col_idx, sets=(), item_set=None, matrix_status=None,
                     criterion=1e-4, maxits=1000, iters_per_launch=0, workspace_bytes=0, full=False, device=0, timing=None):
    """``twxem_mean_variance``: the EM estimate of mean and variance of every item's target column (norm's ``em.norm`` as
    include/twx_qa.h restates it).

    obs [nstn, ndays] float32, station-major, NaN = missing; group [ndays] int8, -1 or 0 .. G - 1; item_target, item_group
    [nitem]; col_off [nitem + 1] / col_idx: the CSR of each item's station columns (rows of obs) in order; ``sets``: a
    sequence of (group, values [ndays of the group, ncol] float64), ``item_set`` [nitem] the set of each item or -1;
    ``matrix_status`` [nitem]: the items' ``twxif_infill_matrix`` status (not 0: EM_NO_MATRIX).  ``iters_per_launch`` and
    ``workspace_bytes`` of 0 take the library's defaults.  Returns a dict of mean, variance, iters, delta, status [nitem],
    ``rounds`` and ``batches``, and with ``full`` mu [nitem, 31] and sigma [nitem, 31, 31].  ``timing`` receives
    ``em_prep_kernel_ms`` / ``em_iter_kernel_ms``, the host-clock ``em_upload_ms`` / ``em_download_ms``, ``em_rounds`` and
    ``em_batches``."""
    load()
    obs, group = _c(obs, np.float32), _c(group, np.int8)
    item_target, item_group = _c(item_target, np.int32), _c(item_group, np.int32)
    col_off, col_idx = _c(col_off, np.int64), _c(col_idx, np.int32)
    if obs.ndim != 2 or group.shape != (obs.shape[1],):
        raise ValueError("obs must be [nstn, ndays] and group [ndays]")
    ni = item_target.size
    if item_target.ndim != 1 or item_group.shape != (ni,) or col_off.shape != (ni + 1,) or col_idx.ndim != 1 or \
            (ni and (col_off[0] != 0 or col_off[-1] != col_idx.size)):
        raise ValueError("item_target / item_group must be [nitem] and col_off [nitem + 1] the CSR offsets of col_idx")
    ng = int(group.max()) + 1 if group.size and group.max() >= 0 else 1
    ng = max(ng, int(item_group.max()) + 1 if ni else 1)
    nrows = np.bincount(group[group >= 0].astype(np.int64), minlength=ng)
    set_group, set_ncol, set_vals = _pack_sets(sets, ng, nrows)
    item_set = np.full(ni, -1, np.int32) if item_set is None else _c(item_set, np.int32)
    if item_set.shape != (ni,):
        raise ValueError("item_set must be [nitem]")
    if matrix_status is not None:
        matrix_status = _c(matrix_status, np.int32)
        if matrix_status.shape != (ni,):
            raise ValueError("matrix_status must be [nitem]")
    out = dict(mean=np.empty(ni), variance=np.empty(ni), iters=np.empty(ni, np.int32), delta=np.empty(ni),
               status=np.empty(ni, np.int32))
    if full:
        out["mu"], out["sigma"] = np.empty((ni, EM_MAX_COLS)), np.empty((ni, EM_MAX_COLS, EM_MAX_COLS))
    counts = np.zeros(2, np.int32)
    ms = _call("twxem_mean_variance",
               (int(device), obs.shape[0], obs.shape[1], obs.ctypes.data, ng, group.ctypes.data, ni,
                item_target.ctypes.data, item_group.ctypes.data,
                matrix_status.ctypes.data if matrix_status is not None else None, col_off.ctypes.data,
                col_idx.ctypes.data, set_group.size, set_group.ctypes.data, set_ncol.ctypes.data,
                set_vals.ctypes.data, item_set.ctypes.data, float(criterion), int(maxits),
                int(iters_per_launch), int(workspace_bytes), out["mean"].ctypes.data,
                out["variance"].ctypes.data, out["iters"].ctypes.data, out["delta"].ctypes.data,
                out["status"].ctypes.data, out["mu"].ctypes.data if full else None,
                out["sigma"].ctypes.data if full else None), len(EM_KERNELS) + len(EM_HOST_TIMES), counts)
    out["rounds"], out["batches"] = int(counts[0]), int(counts[1])
    _put_times(timing, _ms_keys(EM_KERNELS, EM_HOST_TIMES), ms, em_rounds=out["rounds"], em_batches=out["batches"])
    return out


# ---- the estimator of step16 (twxpp_ppca_fit; TWXPP_* of include/twx_qa.h) ----
PP_EXPORTS = ("twxpp_ppca_fit",)
PP_OK, PP_NUMERIC, PP_MAXITS, PP_NO_MATRIX, PP_EMPTY_COLUMN, PP_ROW_CAP, PP_COL_CAP, PP_PCS_CAP = 0, 4, 20, 21, 22, 23, 24, 25
PP_MAX_COLS = 64          # TWXPP_MAX_COLS
PP_MAX_PCS = 32           # TWXPP_MAX_PCS
PP_MAX_ROWS = 8192        # TWXPP_MAX_ROWS
PP_SEED = 4324            # pca_infill.R: SEED
PP_KERNELS = ("pp_prep", "pp_iter")                     # TWXPP_NKERNELS
PP_HOST_TIMES = ("pp_upload", "pp_download")            # the rest of TWXPP_NTIMES: host-clock milliseconds


def ppca_default_c0(ncols, npcs, seed=PP_SEED):
    """The start of a fit, flat and column-major [D, d]: ``np.random.RandomState(seed).standard_normal(D * d)`` (R's
    ``rnorm`` stream under ``set.seed(4324)`` cannot be reproduced; this generator is frozen across numpy versions)."""
    return np.random.RandomState(seed).standard_normal(int(ncols) * int(npcs))


def ppca_pack(obs, group, item_target, item_group, item_npcs, col_off, col_idx, norms, stds, c0=None, sets=(),
              item_set=None, matrix_status=None):
    """The arrays ``twxpp_ppca_fit`` takes, checked: a dict.  See ``ppca_fit``."""
    obs, group = _c(obs, np.float32), _c(group, np.int8)
    item_target, item_group, item_npcs = _c(item_target, np.int32), _c(item_group, np.int32), _c(item_npcs, np.int32)
    col_off, col_idx = _c(col_off, np.int64), _c(col_idx, np.int32)
    if obs.ndim != 2 or group.shape != (obs.shape[1],):
        raise ValueError("obs must be [nstn, ndays] and group [ndays]")
    ni = item_target.size
    if item_target.ndim != 1 or ni < 1 or item_group.shape != (ni,) or item_npcs.shape != (ni,) or \
            col_off.shape != (ni + 1,) or col_idx.ndim != 1 or col_off[0] != 0 or col_off[-1] != col_idx.size:
        raise ValueError("item_target / item_group / item_npcs must be [nitem >= 1] and col_off [nitem + 1] the CSR "
                         "offsets of col_idx")
    ng = int(group.max()) + 1 if group.size and group.max() >= 0 else 1
    ng = max(ng, int(item_group.max()) + 1)
    if item_group.min() < 0:
        raise ValueError("item_group must be >= 0")
    nrows = np.bincount(group[group >= 0].astype(np.int64), minlength=ng)
    set_group, set_ncol, set_vals = _pack_sets(sets, ng, nrows)
    item_set = np.full(ni, -1, np.int32) if item_set is None else _c(item_set, np.int32)
    if item_set.shape != (ni,) or (ni and (item_set.min() < -1 or item_set.max() >= set_group.size)):
        raise ValueError("item_set must be [nitem] of -1 or a set index")
    if matrix_status is None:
        matrix_status = np.zeros(ni, np.int32)
    matrix_status = _c(matrix_status, np.int32)
    if matrix_status.shape != (ni,):
        raise ValueError("matrix_status must be [nitem]")
    ncols = (1 + np.diff(col_off) + np.where(item_set >= 0, set_ncol[np.maximum(item_set, 0)] if set_group.size else 0, 0)
             ).astype(np.int64)
    norms, stds = _c(norms, np.float64), _c(stds, np.float64)
    if norms.shape != (int(ncols.sum()),) or stds.shape != norms.shape:
        raise ValueError("norms / stds must hold the columns of every item, the items one after the other")
    nc0 = np.where(matrix_status == IF_OK, ncols * item_npcs, 0)
    if c0 is None:
        c0 = np.concatenate([ppca_default_c0(ncols[i], item_npcs[i]) if nc0[i] else np.zeros(0) for i in range(ni)])
    c0 = _c(c0, np.float64)
    if c0.shape != (int(nc0.sum()),):
        raise ValueError("c0 must hold D * d values per item with a matrix, column-major, the items one after the other")
    fit_off = np.concatenate([[0], np.cumsum(nrows[item_group])]).astype(np.int64)
    return dict(obs=obs, group=group, ng=ng, item_target=item_target, item_group=item_group, matrix_status=matrix_status,
                item_npcs=item_npcs, col_off=col_off, col_idx=col_idx, set_group=set_group, set_ncol=set_ncol,
                set_vals=set_vals, item_set=item_set, norms=norms, stds=stds, c0=c0, fit_off=fit_off, ncols=ncols)


def ppca_fit(obs, group, item_target, item_group, item_npcs, col_off, col_idx, norms, stds, c0=None, sets=(),
             item_set=None, matrix_status=None, threshold=1e-5, maxits=1000, iters_per_launch=0, workspace_bytes=0,
             full=False, device=0, timing=None):
    """``twxpp_ppca_fit``: one PPCA fit (pcaMethods' ``ppca`` as include/twx_qa.h restates it) per item.

    obs [nstn, ndays] float32, station-major, NaN = missing; group [ndays] int8, -1 or 0 .. G - 1; item_target,
    item_group, item_npcs [nitem]; col_off [nitem + 1] / col_idx: the CSR of each item's station columns; ``sets`` /
    ``item_set`` / ``matrix_status`` as ``em_mean_variance`` takes them; norms / stds: the D values of every item, flat;
    ``c0``: the starts, flat, D * d values per item column-major (default ``ppca_default_c0``).  Returns a dict of ``fit``
    (flat) with ``fit_off`` [nitem + 1], r2cum [nitem, 32], iters, rel, status [nitem], ``rounds``, ``batches``, and with
    ``full`` C [nitem, 64, 32] and M [nitem, 64].  ``timing`` receives ``pp_prep_kernel_ms`` / ``pp_iter_kernel_ms``, the
    host-clock ``pp_upload_ms`` / ``pp_download_ms`` (accumulated over calls when present), ``pp_rounds``, ``pp_batches``."""
    load()
    p = ppca_pack(obs, group, item_target, item_group, item_npcs, col_off, col_idx, norms, stds, c0, sets, item_set,
                  matrix_status)
    ni = p["item_target"].size
    out = dict(fit=np.empty(int(p["fit_off"][-1])), fit_off=p["fit_off"], r2cum=np.empty((ni, PP_MAX_PCS)),
               iters=np.empty(ni, np.int32), rel=np.empty(ni), status=np.empty(ni, np.int32))
    if full:
        out["C"], out["M"] = np.empty((ni, PP_MAX_COLS, PP_MAX_PCS)), np.empty((ni, PP_MAX_COLS))
    counts = np.zeros(2, np.int32)
    ms = _call("twxpp_ppca_fit",
               (int(device), p["obs"].shape[0], p["obs"].shape[1], p["obs"].ctypes.data, p["ng"],
                p["group"].ctypes.data, ni, p["item_target"].ctypes.data, p["item_group"].ctypes.data,
                p["matrix_status"].ctypes.data, p["item_npcs"].ctypes.data, p["col_off"].ctypes.data,
                p["col_idx"].ctypes.data, p["set_group"].size, p["set_group"].ctypes.data,
                p["set_ncol"].ctypes.data, p["set_vals"].ctypes.data, p["item_set"].ctypes.data,
                p["norms"].ctypes.data, p["stds"].ctypes.data, p["c0"].ctypes.data, float(threshold), int(maxits),
                int(iters_per_launch), int(workspace_bytes), out["fit"].ctypes.data, out["r2cum"].ctypes.data,
                out["iters"].ctypes.data, out["rel"].ctypes.data, out["status"].ctypes.data,
                out["C"].ctypes.data if full else None, out["M"].ctypes.data if full else None),
               len(PP_KERNELS) + len(PP_HOST_TIMES), counts)
    out["rounds"], out["batches"] = int(counts[0]), int(counts[1])
    _put_times(timing, _ms_keys(PP_KERNELS, PP_HOST_TIMES), ms, add=True, pp_rounds=out["rounds"],
               pp_batches=out["batches"], pp_calls=1)
    return out


# ---- the check of step16's fits (twxck_infill_check; TWXCK_* of include/twx_qa.h) ----
CK_EXPORTS = ("twxck_infill_check",)
CK_OK, CK_NOT_FITTED, CK_FEW_ROWS, CK_ROW_CAP = 0, 26, 27, 28
CK_LOW_PERF, CK_IMPOSSIBLE, CK_VAR_CHGPT, CK_UNFITTED = 1, 2, 4, 8      # bits of reasons
CK_MAX_ROWS = 8192        # TWXCK_MAX_ROWS
CK_MAE_MAX, CK_R2_MIN = 2.0, 0.7                          # infill_daily.py:578
CK_IMPOSSIBLE_HIGH, CK_IMPOSSIBLE_LOW = 57.7, -89.4       # infill_daily.py:584
CK_SIG = 1e-10            # pca_infill.R: hasVarChgPt's default sig
CK_KERNELS = ("ck_check",)
CK_HOST_TIMES = ("ck_upload", "ck_download")              # the rest of TWXCK_NTIMES: host-clock milliseconds


def cpt_penalty(n, sig=CK_SIG):
    """The "Asymptotic" penalty of ``cpt.var`` for a series of ``n`` values at the level ``sig`` (changepoint's formula for
    a change in variance, restated): NaN where a logarithm or root has a negative argument (n < 63 at sig = 1e-10), which
    the check reads as "no change point" and where R stops with an error."""
    import math
    try:
        ll = math.log(math.log(n))
        a = math.sqrt(2.0 * ll)
        b = 2.0 * ll + math.log(ll) / 2.0 - math.log(math.gamma(0.5))
        return (-(math.log(math.log((1.0 - sig + math.exp(-2.0 * math.exp(b))) ** -0.5)) / a) + b / a) ** 2
    except (ValueError, ZeroDivisionError, OverflowError):
        return float("nan")


def infill_check(off, fit, obs, pen=None, sig=CK_SIG, mae_max=CK_MAE_MAX, r2_min=CK_R2_MIN,
                 impossible_high=CK_IMPOSSIBLE_HIGH, impossible_low=CK_IMPOSSIBLE_LOW, workspace_bytes=0, device=0,
                 timing=None):
    """``twxck_infill_check``: ``_is_nonoptimal_infill`` with ``hasVarChgPt`` (as include/twx_qa.h restates them) of every
    item.

    off [nitem + 1] non-decreasing from 0; fit, obs [off[-1]] float64, the items one after the other, obs NaN = missing;
    ``pen`` [nitem] or a scalar: the change-point penalty (default ``cpt_penalty(N, sig)`` per item; NaN: no change point).
    Returns a dict of nobs, mae, r2, nimpossible, cpt_stat, cpt_tau, reasons (``CK_*`` bits), status and pen [nitem], and
    ``batches``.  ``timing`` receives ``ck_check_kernel_ms``, the host-clock ``ck_upload_ms`` / ``ck_download_ms``
    (accumulated over calls when present), ``ck_batches`` and ``ck_calls``."""
    load()
    off, fit, obs = _c(off, np.int64), _c(fit, np.float64), _c(obs, np.float64)
    if off.ndim != 1 or off.size < 2 or fit.ndim != 1 or obs.shape != fit.shape:
        raise ValueError("off must be [nitem + 1 >= 2] and fit / obs flat arrays of one length")
    ni = off.size - 1
    if (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] != fit.size:
        raise ValueError("off[-1] must be the length of fit / obs")
    if pen is None:
        cache = {}
        pen = np.array([cache.setdefault(int(n), cpt_penalty(int(n), sig)) for n in np.diff(off)], np.float64)
    pen = _c(np.broadcast_to(np.asarray(pen, np.float64), (ni,)), np.float64)
    out = dict(nobs=np.empty(ni, np.int32), mae=np.empty(ni), r2=np.empty(ni), nimpossible=np.empty(ni, np.int32),
               cpt_stat=np.empty(ni), cpt_tau=np.empty(ni, np.int32), reasons=np.empty(ni, np.int32),
               status=np.empty(ni, np.int32))
    counts = np.zeros(2, np.int32)
    ms = _call("twxck_infill_check",
               (int(device), ni, off.ctypes.data, fit.ctypes.data, obs.ctypes.data, pen.ctypes.data,
                float(mae_max), float(r2_min), float(impossible_high), float(impossible_low),
                int(workspace_bytes), out["nobs"].ctypes.data, out["mae"].ctypes.data, out["r2"].ctypes.data,
                out["nimpossible"].ctypes.data, out["cpt_stat"].ctypes.data, out["cpt_tau"].ctypes.data,
                out["reasons"].ctypes.data, out["status"].ctypes.data), len(CK_KERNELS) + len(CK_HOST_TIMES), counts)
    out["pen"], out["batches"] = pen, int(counts[1])
    _put_times(timing, _ms_keys(CK_KERNELS, CK_HOST_TIMES), ms, add=True, ck_batches=out["batches"], ck_calls=1)
    return out


# ---- step15, the cross-validation of the infill (twxxv_*; TWXXV_* of include/twx_qa.h) ----
XV_EXPORTS = ("twxxv_holdout", "twxxv_infill_matrix", "twxxv_score")
XV_NGROUPS = 12           # TWXXV_NGROUPS
XV_NSCORES = 13           # TWXXV_NSCORES: the groups, then the whole series


def xval_nkeep(ntrain_yrs):
    """The observations kept for training (xval_infill.py:73): ``int(np.round(ntrain_yrs * 365.25))``, half to even."""
    return int(np.round(ntrain_yrs * 365.25))


def holdout(obs, target_idx, nkeep, device=0, timing=None):
    """``twxxv_holdout``: the held-out observations of ``XvalInfill.__init__`` (xval_infill.py:73-86) for the rows
    ``target_idx`` of obs [nstn, ndays] float32 (station-major).  A finite day is held iff ``nkeep > 0`` and at least
    ``nkeep`` finite days of the row lie after it.  Returns a dict of ``held`` [ntarget, ndays] bool, ``train_obs``
    [ntarget, ndays] float32 (held days NaN, the rest bit for bit), ``nheld`` and ``nfinite`` [ntarget]."""
    load()
    obs, target_idx = _c(obs, np.float32), _c(target_idx, np.int32)
    if obs.ndim != 2 or target_idx.ndim != 1:
        raise ValueError("obs must be [nstn, ndays] and target_idx [ntarget]")
    if not isinstance(nkeep, (int, np.integer)):
        raise ValueError("nkeep must be an integer (xval_nkeep(ntrain_yrs))")
    nstn, ndays = obs.shape
    nt = target_idx.size
    held, train = np.zeros((nt, ndays), np.uint8), np.empty((nt, ndays), np.float32)
    nheld, nfin = np.zeros(nt, np.int32), np.zeros(nt, np.int32)
    ms = _call("twxxv_holdout", (int(device), nstn, ndays, obs.ctypes.data, nt, target_idx.ctypes.data, int(nkeep),
                                 held.ctypes.data, train.ctypes.data, nheld.ctypes.data, nfin.ctypes.data), 1)
    _put_times(timing, ("xv_holdout_kernel_ms",), ms)
    return dict(held=held.view(np.bool_), train_obs=train, nheld=nheld, nfinite=nfin)


def xval_score(infill, obs, held, group, device=0, timing=None):
    """``twxxv_score``: bias and MAE of the infilled series against the held-out observations (run_xval:153-154 and the
    writer's arithmetic, step15:127-134).  infill [ns, ndays] float64; obs [ns, ndays] float32; held [ns, ndays] bool; group
    [ndays] int8, -1 or 0 .. 11.  Returns a dict of ``n``, ``bias``, ``mae`` [ns] over the whole series, ``group_n``,
    ``group_bias``, ``group_mae`` [ns, 12], and ``obs_out`` / ``infill_out`` [ns, ndays] float32 (NaN off the scored days)."""
    load()
    infill, obs = _c(infill, np.float64), _c(obs, np.float32)
    held, group = _c(np.asarray(held) != 0, np.uint8), _c(group, np.int8)
    if infill.ndim != 2 or obs.shape != infill.shape or held.shape != infill.shape or group.shape != infill.shape[1:]:
        raise ValueError("infill / obs / held must be [nseries, ndays] and group [ndays]")
    ns, ndays = infill.shape
    n = np.zeros((ns, XV_NSCORES), np.int32)
    bias, mae = np.empty((ns, XV_NSCORES)), np.empty((ns, XV_NSCORES))
    oo, io = np.empty((ns, ndays), np.float32), np.empty((ns, ndays), np.float32)
    ms = _call("twxxv_score", (int(device), ns, ndays, infill.ctypes.data, obs.ctypes.data, held.ctypes.data,
                               group.ctypes.data, n.ctypes.data, bias.ctypes.data, mae.ctypes.data, oo.ctypes.data,
                               io.ctypes.data), 1)
    _put_times(timing, ("xv_score_kernel_ms",), ms)
    return dict(n=n[:, XV_NGROUPS].copy(), bias=bias[:, XV_NGROUPS].copy(), mae=mae[:, XV_NGROUPS].copy(),
                group_n=n[:, :XV_NGROUPS].copy(), group_bias=bias[:, :XV_NGROUPS].copy(),
                group_mae=mae[:, :XV_NGROUPS].copy(), obs_out=oo, infill_out=io)


# ---- step17 / step18, the serially-complete database (twxsc_*; TWXSC_* of include/twx_qa.h) ----
SC_EXPORTS = ("twxsc_serial_complete", "twxsc_series_check")
SC_MAX_DAYS = 1048576     # TWXSC_MAX_DAYS
SC_MAX_GROUPS = 1536      # TWXSC_MAX_GROUPS
SC_RUN_THRESHOLD = 1826   # TWXSC_DEFAULT_RUN_THRESHOLD: int(np.round(365.25 * 5.0)), post_infill.py:39
SC_MAX_MISS = 9           # TWXSC_DEFAULT_MAX_MISS
SC_FILL_F4 = 9.969209968386869e36       # netCDF4.default_fillvals['f4']
SC_KERNELS = ("sc_select", "sc_norms")                  # the first entries of TWXSC_NTIMES
SC_HOST_TIMES = ("sc_upload", "sc_download")            # the rest: host-clock milliseconds
SC_CHECK_TIMES = ("sc_series_kernel_ms", None, "sc_series_upload_ms", "sc_series_download_ms")


def run_threshold(years=5.0):
    """``USE_ALL_INFILL_THRESHOLD`` (post_infill.py:39): ``int(np.round(365.25 * years))``."""
    return int(np.round(365.25 * years))


def norm_groups(year, month, start_norm_yr, end_norm_yr, day=None):
    """(group_first, group_ndays) [12 * nyears] of ``twxsc_serial_complete`` for the day axis ``year`` / ``month`` [ndays]:
    group 12 (y - start_norm_yr) + m - 1 owns the days of month m of year y.  Raises ``ValueError`` for an axis that is not
    ascending and gap-free (in (year, month); with ``day`` [ndays] day by day), or a period of more than ``SC_MAX_GROUPS``
    months."""
    year, month = np.asarray(year, np.int64), np.asarray(month, np.int64)
    if year.ndim != 1 or month.shape != year.shape or year.size < 1:
        raise ValueError("year / month must be [ndays >= 1]")
    start_norm_yr, end_norm_yr = int(start_norm_yr), int(end_norm_yr)
    if end_norm_yr < start_norm_yr or 12 * (end_norm_yr - start_norm_yr + 1) > SC_MAX_GROUPS:
        raise ValueError("the normals cover 1 .. %d years" % (SC_MAX_GROUPS // 12))
    ym = year * 12 + month - 1
    if month.min() < 1 or month.max() > 12 or ((np.diff(ym) != 0) & (np.diff(ym) != 1)).any():
        raise ValueError("the day axis must be ascending and gap-free (no skipped month or year)")
    if day is not None:
        day = np.asarray(day, np.int64)
        if day.shape != year.shape or day.min() < 1 or day.max() > 31:
            raise ValueError("day must be [ndays] of 1 .. 31")
        d64 = ((year - 1970) * 12 + month - 1).astype("datetime64[M]").astype("datetime64[D]") + (day - 1)
        if (np.diff(d64).astype(np.int64) != 1).any():
            raise ValueError("the day axis must be ascending and gap-free (consecutive days)")
    ng = 12 * (end_norm_yr - start_norm_yr + 1)
    g = ym - 12 * start_norm_yr
    first, nd = np.zeros(ng, np.int32), np.zeros(ng, np.int32)
    inside = np.nonzero((g >= 0) & (g < ng))[0]
    if inside.size:
        u, i0, cnt = np.unique(g[inside], return_index=True, return_counts=True)
        first[u], nd[u] = inside[i0], cnt
    return first, nd


def serial_complete(tair, tair_infilled=None, flag=None, run_threshold=SC_RUN_THRESHOLD, fill=SC_FILL_F4, group_first=None,
                    group_ndays=None, max_miss=SC_MAX_MISS, workspace_bytes=0, device=0, timing=None):
    """``twxsc_serial_complete``: ``create_serially_complete_db``'s choice and scrub (post_infill.py:106-149) and the monthly
    normals of ``add_monthly_normals`` for every series of one call.

    tair [nseries, ndays] float32, station-major; tair_infilled the same and flag [nseries, ndays] int8, or both None
    ("take tair as it is": no serial / flag_infilled output); group_first / group_ndays [ngroups] (``norm_groups``) or both
    None (no normals); ``max_miss`` None or negative: no threshold.  Returns a dict of max_run, nmissing [nseries] int32,
    all_infill [nseries] bool, ``batches``, with flags ``serial`` [nseries, ndays] float32 and ``flag_infilled`` int8, with
    groups ``norm`` [nseries, 12] float64 and ``norm_nmths`` int32.  ``timing`` receives ``sc_select_kernel_ms`` /
    ``sc_norms_kernel_ms``, the host-clock ``sc_upload_ms`` / ``sc_download_ms`` (accumulated over calls), ``sc_batches``
    and ``sc_calls``."""
    load()
    tair = _c(tair, np.float32)
    if tair.ndim != 2:
        raise ValueError("tair must be [nseries, ndays]")
    ns, nd = tair.shape
    if (tair_infilled is None) != (flag is None):
        raise ValueError("tair_infilled and flag are given together or not at all")
    full = flag is not None
    if full:
        tair_infilled, flag = _c(tair_infilled, np.float32), _c(flag, np.int8)
        if tair_infilled.shape != tair.shape or flag.shape != tair.shape:
            raise ValueError("tair_infilled / flag must be [nseries, ndays] like tair")
    if (group_first is None) != (group_ndays is None):
        raise ValueError("group_first and group_ndays are given together or not at all")
    norms = group_first is not None
    ng = 0
    if norms:
        group_first, group_ndays = _c(group_first, np.int32), _c(group_ndays, np.int32)
        if group_first.ndim != 1 or group_ndays.shape != group_first.shape:
            raise ValueError("group_first / group_ndays must be [ngroups]")
        ng = group_first.size
    out = dict(max_run=np.zeros(ns, np.int32), nmissing=np.zeros(ns, np.int32), all_infill=np.zeros(ns, np.uint8))
    if full:
        out["serial"], out["flag_infilled"] = np.empty((ns, nd), np.float32), np.empty((ns, nd), np.int8)
    if norms:
        out["norm"], out["norm_nmths"] = np.empty((ns, 12)), np.empty((ns, 12), np.int32)
    counts = np.zeros(2, np.int32)
    ms = _call("twxsc_serial_complete",
               (int(device), ns, nd, tair.ctypes.data, tair_infilled.ctypes.data if full else None,
                flag.ctypes.data if full else None, int(run_threshold), float(fill), ng,
                group_first.ctypes.data if norms else None, group_ndays.ctypes.data if norms else None,
                -1 if max_miss is None else int(max_miss), int(workspace_bytes),
                out["serial"].ctypes.data if full else None, out["flag_infilled"].ctypes.data if full else None,
                out["max_run"].ctypes.data, out["nmissing"].ctypes.data, out["all_infill"].ctypes.data,
                out["norm"].ctypes.data if norms else None, out["norm_nmths"].ctypes.data if norms else None),
               len(SC_KERNELS) + len(SC_HOST_TIMES), counts)
    out["all_infill"] = out["all_infill"].view(np.bool_)
    out["batches"] = int(counts[1])
    _put_times(timing, _ms_keys(SC_KERNELS, SC_HOST_TIMES), ms, add=True, sc_batches=out["batches"], sc_calls=1)
    return out


def series_check(series, pen=None, sig=CK_SIG, fill=SC_FILL_F4, impossible_high=CK_IMPOSSIBLE_HIGH,
                 impossible_low=CK_IMPOSSIBLE_LOW, workspace_bytes=0, device=0, timing=None):
    """``twxsc_series_check``: step17's ``has_bad_infill`` of every WHOLE series (no cap of ``CK_MAX_ROWS`` rows).

    series [nseries, ndays] float32; ``pen``: the change-point penalty (default ``cpt_penalty(ndays, sig)``; NaN: no change
    point).  Returns a dict of nimpossible, nmissing, cpt_stat, cpt_tau, reasons (``CK_*`` bits), status [nseries], ``pen``
    and ``batches``.  ``timing`` receives ``sc_series_kernel_ms``, the host-clock ``sc_series_upload_ms`` /
    ``sc_series_download_ms`` (accumulated over calls), ``sc_series_batches`` and ``sc_series_calls``."""
    load()
    series = _c(series, np.float32)
    if series.ndim != 2:
        raise ValueError("series must be [nseries, ndays]")
    ns, nd = series.shape
    pen = cpt_penalty(nd, sig) if pen is None else float(pen)
    out = dict(nimpossible=np.empty(ns, np.int32), nmissing=np.empty(ns, np.int32), cpt_stat=np.empty(ns),
               cpt_tau=np.empty(ns, np.int32), reasons=np.empty(ns, np.int32), status=np.empty(ns, np.int32))
    counts = np.zeros(2, np.int32)
    ms = _call("twxsc_series_check",
               (int(device), ns, nd, series.ctypes.data, float(fill), pen, float(impossible_high),
                float(impossible_low), int(workspace_bytes), out["nimpossible"].ctypes.data,
                out["nmissing"].ctypes.data, out["cpt_stat"].ctypes.data, out["cpt_tau"].ctypes.data,
                out["reasons"].ctypes.data, out["status"].ctypes.data), len(SC_CHECK_TIMES), counts)
    out["pen"], out["batches"] = pen, int(counts[1])
    _put_times(timing, SC_CHECK_TIMES, ms, add=True, sc_series_batches=out["batches"], sc_series_calls=1)
    return out


# ---- the reanalysis columns of the infill family (twxnr_components; TWXNR_* of include/twx_qa.h) ----
NR_EXPORTS = ("twxnr_components",)
NR_OK, NR_NOCONV, NR_NONFINITE, NR_CONSTANT, NR_FEW_ROWS = 0, 29, 30, 31, 32
NR_MAX_COLS = 64          # TWXNR_MAX_COLS
NR_MAX_CUTS = 4           # TWXNR_MAX_CUTS
NR_MAX_SWEEPS = 30        # TWXNR_MAX_SWEEPS
NR_KERNELS = ("nr_gram", "nr_eig", "nr_scores")         # TWXNR_NKERNELS
NR_HOST_TIMES = ("nr_upload", "nr_download")            # the rest of TWXNR_NTIMES: host-clock milliseconds


class NrComponents(object):
    """The result of ``nnr_components_batched``, item = set * ngroups + group.  ``status``, ``bad_col``, ``sweeps``
    [nset, G]; ``ncomp`` [nset, G, nthr]; ``nrows`` [G]; ``ncols`` [nset]; and per item through ``var_explain(s, g)``,
    ``eigval(s, g)``, ``mean(s, g)``, ``sd(s, g)`` [P], ``loadings(s, g)`` [P, P] (component k is row k) and
    ``scores(s, g, k=None)`` [n, k] (the first k components, default all that were formed: those of the item's largest
    cut; an item that was not decomposed has none)."""

    def __init__(self, set_off, nrows, max_var, out):
        self.set_off, self.nrows, self.max_var = set_off, nrows, tuple(float(v) for v in max_var)
        self.ncols = np.diff(set_off).astype(np.int64)
        self.nset, self.ngroups = self.ncols.size, nrows.size
        self._sq = np.concatenate([[0], np.cumsum(self.ncols ** 2)])
        self.status, self.bad_col, self.sweeps, self.ncomp = out["status"], out["bad_col"], out["sweeps"], out["ncomp"]
        self._out = out

    def _p(self, s, g, name):
        P = int(self.ncols[s])
        a = self.ngroups * int(self.set_off[s]) + g * P
        return self._out[name][a:a + P]

    def var_explain(self, s, g):
        return self._p(s, g, "var_explain")

    def eigval(self, s, g):
        return self._p(s, g, "eigval")

    def mean(self, s, g):
        return self._p(s, g, "mean")

    def sd(self, s, g):
        return self._p(s, g, "sd")

    def loadings(self, s, g):
        P = int(self.ncols[s])
        a = self.ngroups * int(self._sq[s]) + g * P * P
        return self._out["loadings"][a:a + P * P].reshape(P, P)

    def scores(self, s, g, k=None):
        i, n = s * self.ngroups + g, int(self.nrows[g])
        a, b = int(self._out["score_off"][i]), int(self._out["score_off"][i + 1])
        have = (b - a) // n if n else 0
        if k is None:
            k = have
        if k > have:
            raise ValueError("item (%d, %d) has %d score columns, %d asked for" % (s, g, have, k))
        return self._out["scores"][a:a + k * n].reshape(k, n).T


def nnr_components_batched(cols, set_off, set_col, group, max_var=(0.99,), ngroups=None, device=0, timing=None):
    """``twxnr_components``: the principal components of every (column set, day group) item in one call.

    cols [ncol, ndays] float32 (a column's days contiguous); set_off [nset + 1] / set_col: the CSR of the sets' columns;
    group [ndays] int8, -1 or 0 .. G - 1; ``max_var``: the cuts, each in (0, 1).  Returns an ``NrComponents``.  ``timing``
    receives ``nr_gram_kernel_ms`` / ``nr_eig_kernel_ms`` / ``nr_scores_kernel_ms`` and the host-clock ``nr_upload_ms`` /
    ``nr_download_ms``."""
    load()
    cols, group = _c(cols, np.float32), _c(group, np.int8)
    set_off, set_col = _c(set_off, np.int64), _c(set_col, np.int32)
    max_var = _c(np.atleast_1d(np.asarray(max_var, np.float64)), np.float64)
    if cols.ndim != 2 or group.shape != (cols.shape[1],):
        raise ValueError("cols must be [ncol, ndays] and group [ndays]")
    if set_off.ndim != 1 or set_off.size < 2 or set_col.ndim != 1 or max_var.ndim != 1:
        raise ValueError("set_off must be [nset + 1 >= 2], set_col and max_var flat")
    nset = set_off.size - 1
    if ngroups is None:
        ngroups = int(group.max()) + 1 if group.size and group.max() >= 0 else 1
    ng, nthr = int(ngroups), max_var.size
    ok = set_off[0] == 0 and (np.diff(set_off) >= 0).all() and set_off[-1] == set_col.size and 0 < ng <= IF_MAX_GROUPS
    nrows = np.bincount(group[(group >= 0) & (group < ng)].astype(np.int64), minlength=ng)[:ng] if ok else np.zeros(max(ng, 0), np.int64)
    ni = nset * max(ng, 0)
    ncols = np.diff(set_off) if ok else np.zeros(nset, np.int64)
    ntot, sq = int(ncols.sum()) * max(ng, 0), int((ncols ** 2).sum()) * max(ng, 0)
    cap = int((np.minimum(ncols, NR_MAX_COLS)[:, None] * nrows[None, :]).sum()) if ok else 0     # always enough; pages of an empty array are not touched
    out = dict(status=np.empty((nset, max(ng, 0)), np.int32), bad_col=np.empty((nset, max(ng, 0)), np.int32),
               sweeps=np.empty((nset, max(ng, 0)), np.int32), ncomp=np.empty((nset, max(ng, 0), nthr), np.int32),
               mean=np.empty(ntot), sd=np.empty(ntot), var_explain=np.empty(ntot), eigval=np.empty(ntot),
               loadings=np.empty(sq), score_off=np.zeros(ni + 1, np.int64), scores=np.empty(cap))
    ms = _call("twxnr_components",
               (int(device), cols.shape[1], cols.shape[0], cols.ctypes.data, nset, set_off.ctypes.data,
                set_col.ctypes.data, ng, group.ctypes.data, nthr, max_var.ctypes.data,
                out["status"].ctypes.data, out["bad_col"].ctypes.data, out["ncomp"].ctypes.data,
                out["sweeps"].ctypes.data, out["mean"].ctypes.data, out["sd"].ctypes.data,
                out["var_explain"].ctypes.data, out["eigval"].ctypes.data, out["loadings"].ctypes.data,
                out["score_off"].ctypes.data, cap, out["scores"].ctypes.data), len(NR_KERNELS) + len(NR_HOST_TIMES))
    out["scores"] = out["scores"][:int(out["score_off"][-1])]
    _put_times(timing, _ms_keys(NR_KERNELS, NR_HOST_TIMES), ms, add=True, nr_calls=1)
    return NrComponents(set_off, nrows, max_var, out)


# ---- step05 / step09-11, counts, monthly means, TOB shift, daily homogenisation (twxhm_*; TWXHM_* of include/twx_qa.h) ----
HM_EXPORTS = ("twxhm_obs_cnt", "twxhm_monthly_means", "twxhm_tobs_shift", "twxhm_homog_daily")
HM_OK, HM_NO_ADJ, HM_OVERLAP = 0, 33, 34
HM_MAX_MONTHS = 16384     # TWXHM_MAX_MONTHS
HM_MAX_MISS = 9           # TWXHM_DEFAULT_MAX_MISS
HM_PHA_MISSING = -9999    # TWXHM_PHA_MISSING
HM_KERNELS = ("hm_cnt", "hm_means", "hm_tobs", "hm_delta", "hm_apply")


def month_groups(year, month):
    """(mth_first, mth_ndays, mth_ymd) [nmth] int32 of the ``twxhm_*`` entries for the day axis ``year`` / ``month``
    [ndays]: one entry per year-month present on the axis, ``mth_ymd`` = yyyymm01.  Raises ``ValueError`` for an axis that
    skips a month or runs backwards."""
    year, month = np.asarray(year, np.int64), np.asarray(month, np.int64)
    if year.ndim != 1 or month.shape != year.shape or year.size < 1:
        raise ValueError("year / month must be [ndays >= 1]")
    ym = year * 12 + month - 1
    if month.min() < 1 or month.max() > 12 or ((np.diff(ym) != 0) & (np.diff(ym) != 1)).any():
        raise ValueError("the day axis must be ascending and gap-free (no skipped month or year)")
    u, first, cnt = np.unique(ym, return_index=True, return_counts=True)
    return first.astype(np.int32), cnt.astype(np.int32), ((u // 12) * 10000 + (u % 12 + 1) * 100 + 1).astype(np.int32)


def _hm_rows(name, a, shape=None):
    a = _c(a, np.float32)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("%s must be [nstn >= 1, ndays >= 1]" % name)
    if shape is not None and a.shape != shape:
        raise ValueError("%s must be %s like the record" % (name, list(shape)))
    return a


def _hm_months(ndays, mth_first, mth_ndays):
    mth_first, mth_ndays = _c(mth_first, np.int32), _c(mth_ndays, np.int32)
    if mth_first.ndim != 1 or mth_first.size < 1 or mth_ndays.shape != mth_first.shape:
        raise ValueError("mth_first / mth_ndays must be [nmth >= 1]")
    if mth_first.size > HM_MAX_MONTHS:
        raise ValueError("at most %d months" % HM_MAX_MONTHS)
    f, n = mth_first.astype(np.int64), mth_ndays.astype(np.int64)
    if (f < 0).any() or (n < 1).any() or (n > 31).any() or (f + n > ndays).any():
        raise ValueError("a month lies outside the day axis (mth_first) or has not 1 .. 31 days")
    if (f[1:] != f[:-1] + n[:-1]).any():
        raise ValueError("the months must be consecutive runs of days")
    return mth_first, mth_ndays


def _hm_call(name, args, timing, kernels):
    """A ``twxhm_*`` entry: its one or two kernels' times, then upload and download; returns the number of batches."""
    counts = np.zeros(2, np.int32)
    ms = _call(name, args, 4, counts)
    keys = _ms_keys(kernels) + (None,) * (2 - len(kernels)) + ("hm_upload_ms", "hm_download_ms")
    _put_times(timing, keys, ms, add=True, hm_batches=int(counts[1]), hm_calls=1)
    return int(counts[1])


def obs_cnt(obs, day_month, first_day, last_day, workspace_bytes=0, device=0, timing=None):
    """``twxhm_obs_cnt``: [nstn, 12] int32 counts of the finite days of ``obs`` [nstn, ndays] per calendar month
    (``day_month`` [ndays], 1 .. 12) inside the inclusive day-index window.  Quality flags are not applied."""
    obs = _hm_rows("obs", obs)
    ns, nd = obs.shape
    day_month = _c(day_month, np.int8)
    if day_month.shape != (nd,):
        raise ValueError("day_month must be [ndays]")
    if day_month.min() < 1 or day_month.max() > 12:
        raise ValueError("day_month must hold 1 .. 12")
    first_day, last_day = int(first_day), int(last_day)
    if not 0 <= first_day <= last_day < nd:
        raise ValueError("need 0 <= first_day <= last_day < ndays")
    cnt = np.empty((ns, 12), np.int32)
    _hm_call("twxhm_obs_cnt", (int(device), ns, nd, obs.ctypes.data, day_month.ctypes.data, first_day, last_day,
                               int(workspace_bytes), cnt.ctypes.data), timing, HM_KERNELS[0:1])
    return cnt


def monthly_means(obs, mth_first, mth_ndays, max_miss=HM_MAX_MISS, workspace_bytes=0, device=0, timing=None):
    """``twxhm_monthly_means``: (mth_mean [nstn, nmth] float32 with NaN where masked, mth_miss [nstn, nmth] int16) of
    ``obs`` [nstn, ndays] (NaN on flagged and missing days); ``max_miss`` None or negative: no threshold."""
    obs = _hm_rows("obs", obs)
    ns, nd = obs.shape
    mth_first, mth_ndays = _hm_months(nd, mth_first, mth_ndays)
    nm = mth_first.size
    mean, miss = np.empty((ns, nm), np.float32), np.empty((ns, nm), np.int16)
    _hm_call("twxhm_monthly_means",
             (int(device), ns, nd, obs.ctypes.data, nm, mth_first.ctypes.data, mth_ndays.ctypes.data,
              -1 if max_miss is None else int(max_miss), int(workspace_bytes), mean.ctypes.data, miss.ctypes.data),
             timing, HM_KERNELS[1:2])
    return mean, miss


def tobs_shift(tmax, tobs, workspace_bytes=0, device=0, timing=None):
    """``twxhm_tobs_shift``: (out [nstn, ndays] float32, nshift [nstn] int32), ``_tobs_shift_tmax`` of every station."""
    tmax = _hm_rows("tmax", tmax)
    tobs = _hm_rows("tobs", tobs, tmax.shape)
    ns, nd = tmax.shape
    out, nshift = np.empty((ns, nd), np.float32), np.empty(ns, np.int32)
    _hm_call("twxhm_tobs_shift", (int(device), ns, nd, tmax.ctypes.data, tobs.ctypes.data, int(workspace_bytes),
                                  out.ctypes.data, nshift.ctypes.data), timing, HM_KERNELS[2:3])
    return out, nshift


def homog_daily(obs, mth_mean, mth_miss, pha, mth_ymd, mth_first, mth_ndays, adj_off, adj_ymd_start, adj_ymd_end, adj,
                workspace_bytes=0, device=0, timing=None):
    """``twxhm_homog_daily``: ``HomogDaily.homog_stn`` of every station.  Returns a dict of ``delta`` [nstn, nmth] float64
    (NaN: month untouched), ``out`` [nstn, ndays] float32, ``status`` (``HM_*``) and ``nchanged`` [nstn] int32.  The
    adjustment list is CSR (``adj_off`` [nstn + 1]), each station's entries sorted by ``adj_ymd_start``; an unsorted list,
    a month outside the day axis or a wrong shape raises ``ValueError`` before any launch."""
    obs = _hm_rows("obs", obs)
    ns, nd = obs.shape
    mth_first, mth_ndays = _hm_months(nd, mth_first, mth_ndays)
    nm = mth_first.size
    mth_mean, mth_miss, pha = _c(mth_mean, np.float32), _c(mth_miss, np.int16), _c(pha, np.int32)
    for name, a in (("mth_mean", mth_mean), ("mth_miss", mth_miss), ("pha", pha)):
        if a.shape != (ns, nm):
            raise ValueError("%s must be [nstn, nmth]" % name)
    mth_ymd = _c(mth_ymd, np.int32)
    if mth_ymd.shape != (nm,):
        raise ValueError("mth_ymd must be [nmth]")
    adj_off = _c(adj_off, np.int64)
    if adj_off.shape != (ns + 1,) or adj_off[0] != 0 or (np.diff(adj_off) < 0).any():
        raise ValueError("adj_off must be [nstn + 1], ascending from 0")
    na = int(adj_off[-1])
    adj_ymd_start, adj_ymd_end, adj = _c(adj_ymd_start, np.int32), _c(adj_ymd_end, np.int32), _c(adj, np.float64)
    for name, a in (("adj_ymd_start", adj_ymd_start), ("adj_ymd_end", adj_ymd_end), ("adj", adj)):
        if a.shape != (na,):
            raise ValueError("%s must be [adj_off[-1]]" % name)
    if na > 1:
        inner = np.ones(na, bool)
        inner[adj_off[:-1][adj_off[:-1] < na]] = False           # the first entry of a station has no predecessor
        if (inner[1:] & (np.diff(adj_ymd_start) < 0)).any():
            raise ValueError("a station's adjustments must be sorted by adj_ymd_start")
    out = dict(delta=np.empty((ns, nm)), out=np.empty((ns, nd), np.float32), status=np.empty(ns, np.int32),
               nchanged=np.empty(ns, np.int32))
    out["batches"] = _hm_call(
        "twxhm_homog_daily",
        (int(device), ns, nd, obs.ctypes.data, nm, mth_mean.ctypes.data, mth_miss.ctypes.data, pha.ctypes.data,
         mth_ymd.ctypes.data, mth_first.ctypes.data, mth_ndays.ctypes.data, adj_off.ctypes.data,
         adj_ymd_start.ctypes.data if na else None, adj_ymd_end.ctypes.data if na else None, adj.ctypes.data if na else None,
         int(workspace_bytes), out["delta"].ctypes.data, out["out"].ctypes.data, out["status"].ctypes.data,
         out["nchanged"].ctypes.data), timing, HM_KERNELS[3:5])
    return out


# ---- step19 and the front of step20: raster values at stations, duplicate stations, column counts (twxrv_*; TWXRV_* of
# include/twx_qa.h) ----
RV_EXPORTS = ("twxrv_sample", "twxrv_nearest_data", "twxrv_dup_classes", "twxrv_col_count")
RV_OK, RV_NEAREST, RV_NODATA, RV_NEEDS_FORCE, RV_NO_DATA_ANYWHERE = 0, 35, 36, 37, 38
RV_F32, RV_F64 = 0, 1                 # TWXRV_F32, TWXRV_F64
RV_MAX_EXTENT = 134217727             # TWXRV_MAX_EXTENT
RV_MAX_DUP_STNS = 1048576             # TWXRV_MAX_DUP_STNS
RV_COUNT_I8_SUM, RV_COUNT_F32_MISSING = 0, 1
RV_NTIMES = 3                         # TWXRV_NTIMES
RV_TIE_REL = 1e-9                     # TWXRV_TIE_REL
RV_KERNELS = ("rv_sample", "rv_ring", "rv_dup", "rv_colcount")
RV_RADIAN = 0.017453292519943295      # RADIAN_CONVERSION_FACTOR (twx/utils/util_geo.py:21)
RV_EARTH_KM = 6371.009                # AVG_EARTH_RADIUS_KM


def _rv_raster(data, geo_t):
    """The raster as the ``twxrv_*`` entries take it: (array float32 or float64, dtype code, geo_t [6] float64).  An integer
    raster becomes float32 if every value survives the round trip, float64 otherwise (exact up to 2^53)."""
    data = np.asarray(data)
    if data.ndim != 2 or data.shape[0] < 2 or data.shape[1] < 2:
        raise ValueError("the raster must be [rows >= 2, cols >= 2]")
    if data.dtype == np.float32 or data.dtype == np.float64:
        a = np.ascontiguousarray(data)
    elif data.dtype.kind in "iub":
        a = np.ascontiguousarray(data, np.float32)
        if data.dtype.itemsize > 2 and not np.array_equal(a.astype(data.dtype), data):
            a = np.ascontiguousarray(data, np.float64)
    else:
        a = np.ascontiguousarray(data, np.float64)
    geo_t = _c(geo_t, np.float64)
    if geo_t.shape != (6,) or not np.isfinite(geo_t).all():
        raise ValueError("geo_t must be 6 finite numbers")
    if geo_t[2] != 0.0 or geo_t[4] != 0.0:
        raise ValueError("a rotated raster is refused (geo_t[2] and geo_t[4] must be 0)")
    if not (geo_t[1] > 0.0 and geo_t[5] < 0.0):
        raise ValueError("the raster must be north-up (geo_t[1] > 0, geo_t[5] < 0)")
    return a, (RV_F32 if a.dtype == np.float32 else RV_F64), geo_t


def _rv_call(name, args, timing, kernel, counts=None):
    """A ``twxrv_*`` entry: its kernel's time, then upload and download; ``counts`` [2] int32 where the entry has batches."""
    ms = _call(name, args, RV_NTIMES, counts)
    batches = {} if counts is None else {"rv_batches": int(counts[1])}
    _put_times(timing, (kernel + "_kernel_ms", "rv_upload_ms", "rv_download_ms"), ms, add=True, rv_calls=1, **batches)


def raster_sample(data, geo_t, ndata, lon, lat, band_ndata=None, extract_method=1, revert_nn=False, force_data_value=False,
                  device=0, timing=None):
    """``twxrv_sample``: the decision of ``add_stn_raster_values`` (post_infill.py:305-339) up to the ring search, for all
    stations in one call.  Returns a dict of ``value`` [nstn] float64, ``status`` (``RV_OK`` the value of the method,
    ``RV_NEAREST`` the clipped nearest cell, ``RV_NODATA`` with ``value = ndata``, ``RV_NEEDS_FORCE``), ``row`` and ``col``
    [nstn] int32 (``get_row_col(check_bounds=False)``).  ``band_ndata`` None: the band masks nothing."""
    a, code, geo_t = _rv_raster(data, geo_t)
    lon, lat = _c(lon, np.float64), _c(lat, np.float64)
    if lon.ndim != 1 or lon.size < 1 or lat.shape != lon.shape:
        raise ValueError("lon / lat must be [nstn >= 1]")
    if not (np.isfinite(lon).all() and np.isfinite(lat).all()):
        raise ValueError("a station has a non-finite coordinate")
    if extract_method not in (0, 1):
        raise ValueError("extract_method must be 0 (nearest) or 1 (bilinear); 3 (cubic spline) is not supported")
    n = lon.size
    out = dict(value=np.empty(n), status=np.empty(n, np.int32), row=np.empty(n, np.int32), col=np.empty(n, np.int32))
    _rv_call("twxrv_sample",
             (int(device), a.shape[0], a.shape[1], code, a.ctypes.data, geo_t.ctypes.data, 0 if band_ndata is None else 1,
              0.0 if band_ndata is None else float(band_ndata), float(ndata), n, lon.ctypes.data, lat.ctypes.data,
              int(extract_method), 1 if revert_nn else 0, 1 if force_data_value else 0, out["value"].ctypes.data,
              out["status"].ctypes.data, out["row"].ctypes.data, out["col"].ctypes.data), timing, RV_KERNELS[0])
    return out


def grt_circle_dist(lon1, lat1, lon2, lat2):
    """``grt_circle_dist`` (twx/utils/util_geo.py:24-40) in numpy, operation for operation."""
    lat1rad, lat2rad = lat1 * RV_RADIAN, lat2 * RV_RADIAN
    lon1rad, lon2rad = lon1 * RV_RADIAN, lon2 * RV_RADIAN
    dlat, dlon = lat1rad - lat2rad, lon1rad - lon2rad
    ca = 2 * np.arcsin(np.sqrt(np.square(np.sin(dlat / 2)) + np.cos(lat1rad) * np.cos(lat2rad) * np.square(np.sin(dlon / 2))))
    return RV_EARTH_KM * ca


def ring_cells(rows, cols, y, x, r):
    """The slots of ring ``r`` around (``y``, ``x``) that ``_find_nn_data``'s tests admit, in its order: (slot, row, col)
    int64 arrays.  Slots are numbered over the whole ring, 0 .. 8 r + 1, as ``twxrv_nearest_data`` numbers them."""
    lcol, rcol, trow, brow = x - r, x + r, y - r, y + r
    rr = np.concatenate([np.full(2 * r + 1, trow), np.arange(trow, brow + 1), np.full(2 * r, brow), np.arange(brow, trow, -1)])
    cc = np.concatenate([np.arange(lcol, rcol + 1), np.full(2 * r + 1, lcol), np.arange(rcol, lcol, -1), np.full(2 * r, rcol)])
    ok = (rr > 0) & (rr < rows) & (cc > 0) & (cc < cols)
    return np.nonzero(ok)[0], rr[ok].astype(np.int64), cc[ok].astype(np.int64)


def _rv_ring_host(a, geo_t, ndata, y, x, r):
    """Ring ``r`` decided with numpy's transcendentals: (value, dist, slot) -- the tie guard of ``raster_nearest_data``."""
    slot, rr, cc = ring_cells(a.shape[0], a.shape[1], y, x, r)
    keep = a[rr, cc].astype(np.float64) != ndata
    slot, rr, cc = slot[keep], rr[keep], cc[keep]
    lons = (geo_t[0] + cc * geo_t[1] + rr * geo_t[2]) + geo_t[1] / 2.0
    lats = (geo_t[3] + cc * geo_t[4] + rr * geo_t[5]) + geo_t[5] / 2.0
    pt_lon = (geo_t[0] + x * geo_t[1] + y * geo_t[2]) + geo_t[1] / 2.0
    pt_lat = (geo_t[3] + x * geo_t[4] + y * geo_t[5]) + geo_t[5] / 2.0
    d = grt_circle_dist(pt_lon, pt_lat, lons, lats)
    j = int(np.argsort(d, kind="stable")[0])                      # an exact tie: the earlier slot
    return float(a[rr[j], cc[j]]), float(d[j]), int(slot[j])


def raster_nearest_data(data, geo_t, ndata, row, col, device=0, timing=None):
    """``twxrv_nearest_data``: ``_find_nn_data`` (post_infill.py:443-510) for every start (``row``, ``col``).  Returns a dict
    of ``value``, ``dist``, ``runner_up`` [npts] float64, ``ring``, ``winner`` (the slot in the ring), ``status`` [npts] int32
    (``RV_OK`` / ``RV_NO_DATA_ANYWHERE``) and ``redecided``: the number of points whose winner and runner-up lay within a
    relative ``RV_TIE_REL`` and were decided again on the host with numpy's sin / cos / arcsin on the same ring."""
    a, code, geo_t = _rv_raster(data, geo_t)
    row, col = _c(row, np.int32), _c(col, np.int32)
    if row.ndim != 1 or row.size < 1 or col.shape != row.shape:
        raise ValueError("row / col must be [npts >= 1]")
    if row.min() < 0 or row.max() >= a.shape[0] or col.min() < 0 or col.max() >= a.shape[1]:
        raise ValueError("a start lies outside the raster")
    n = row.size
    out = dict(value=np.empty(n), dist=np.empty(n), runner_up=np.empty(n), ring=np.empty(n, np.int32),
               winner=np.empty(n, np.int32), status=np.empty(n, np.int32))
    _rv_call("twxrv_nearest_data",
             (int(device), a.shape[0], a.shape[1], code, a.ctypes.data, geo_t.ctypes.data, float(ndata), n, row.ctypes.data,
              col.ctypes.data, out["value"].ctypes.data, out["dist"].ctypes.data, out["ring"].ctypes.data,
              out["winner"].ctypes.data, out["runner_up"].ctypes.data, out["status"].ctypes.data), timing, RV_KERNELS[1])
    ok = out["status"] == RV_OK
    with np.errstate(invalid="ignore"):
        close = ok & np.isfinite(out["runner_up"]) & (out["runner_up"] - out["dist"] <= RV_TIE_REL * out["runner_up"])
    for p in np.nonzero(close)[0]:
        out["value"][p], out["dist"][p], out["winner"][p] = _rv_ring_host(a, geo_t, float(ndata), int(row[p]), int(col[p]),
                                                                          int(out["ring"][p]))
    out["redecided"] = int(close.sum())
    return out


def dup_classes(lon, lat, device=0, timing=None):
    """``twxrv_dup_classes``: (cls, size) [nstn] int32 -- the smallest index at the same location (``grt_circle_dist`` == 0)
    and the number of stations there.  A NaN coordinate is a class of its own."""
    lon, lat = _c(lon, np.float64), _c(lat, np.float64)
    if lon.ndim != 1 or lon.size < 1 or lat.shape != lon.shape:
        raise ValueError("lon / lat must be [nstn >= 1]")
    n = lon.size
    cls, size = np.empty(n, np.int32), np.empty(n, np.int32)
    _rv_call("twxrv_dup_classes", (int(device), n, lon.ctypes.data, lat.ctypes.data, cls.ctypes.data, size.ctypes.data),
             timing, RV_KERNELS[2])
    return cls, size


def col_count(data, cols=None, fill=None, workspace_bytes=0, device=0, timing=None):
    """``twxrv_col_count`` on ``data`` [ndays, nstn] in the file's layout.  int8: the sum of every listed column
    (``flag_infilled``) without the days that equal ``fill`` (None: every day counts); float32: the number of days of every
    listed column that are non-finite or equal ``fill`` (None: the f4 fill value).  ``cols`` None: every column; a list may
    be empty, unsorted and may repeat.  Returns [ncol] int32."""
    data = np.asarray(data)
    if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] < 1:
        raise ValueError("data must be [ndays >= 1, nstn >= 1]")
    if data.dtype == np.int8:
        kind, fill = RV_COUNT_I8_SUM, float("nan") if fill is None else float(fill)
        if fill == fill and not (-128 <= fill <= 127 and fill == int(fill)):
            raise ValueError("the fill of an int8 variable must be None or an integer in -128 .. 127")
    elif data.dtype == np.float32:
        kind, fill = RV_COUNT_F32_MISSING, SC_FILL_F4 if fill is None else float(fill)
    else:
        raise ValueError("data must be int8 (a sum) or float32 (a count of missing days)")
    data = np.ascontiguousarray(data)
    nd, ns = data.shape
    if cols is not None:
        cols = _c(cols, np.int32)
        if cols.ndim != 1:
            raise ValueError("cols must be a list of columns")
        if cols.size and (cols.min() < 0 or cols.max() >= ns):
            raise ValueError("a column of the list is outside 0 .. nstn - 1")
        if cols.size == 0:
            return np.zeros(0, np.int32)
    ncol = ns if cols is None else cols.size
    out = np.empty(ncol, np.int32)
    _rv_call("twxrv_col_count",
             (int(device), nd, ns, kind, data.ctypes.data, float(fill), ncol, None if cols is None else cols.ctypes.data,
              int(workspace_bytes), out.ctypes.data), timing, RV_KERNELS[3], np.zeros(2, np.int32))
    return out


# ---- the precipitation QA: the non-spatial chain and the percentile table (twxpq_*; TWXPQ_* of include/twx_qa.h) ----
PQ_EXPORTS = ("twxpq_non_spatial", "twxpq_percentiles")
PQ_PCTILE_ROWS = 366                  # TWXPQ_PCTILE_ROWS: the dates of 2004
PQ_PCTILE_COLS = 5                    # TWXPQ_PCTILE_COLS: 30th, 50th, 70th, 90th, 95th
PQ_MIN_PERCENTILE_VALUES = 20         # TWXPQ_MIN_PERCENTILE_VALUES
PQ_MAX_WINDOW_VALUES = 4096           # TWXPQ_MAX_WINDOW_VALUES: 29 values per year of the series
PQ_KERNELS = ("pq_init", "pq_dups", "pq_streak", "pq_frequent", "pq_gap", "pq_pctiles", "pq_clim")     # TWXPQ_NKERNELS


def _pq_series(name, a, ymd):
    a = _c(a, np.float32)
    if a.ndim != 2 or ymd.ndim != 1 or a.shape[1] != ymd.size or a.shape[0] < 1 or ymd.size < 1:
        raise ValueError("%s must be [nstn >= 1, ndays >= 1] and ymd [ndays]" % name)
    return a


def prcp_non_spatial(prcp, tavg, ymd, streak=False, frequent=False, device=0, details=False, timing=None):
    """``twxpq_non_spatial``: ``run_qa_non_spatial`` (qa_prcp.py:135-176) of every station on its own, with ``_qa_streak`` /
    ``_qa_frequent`` in their places if asked for.  prcp, tavg [nstn, ndays] float32, station-major, NaN = missing; ymd
    [ndays] consecutive days.  Returns flag uint8 [nstn, ndays] (1, 2, 4, 5, 6, 8, 9, 10, 15, 19); with ``details``
    ``(flag, pctiles [nstn, 366, 5])``, the table as the outlier check used it.  ``timing`` receives
    ``<kernel>_kernel_ms`` for the names in ``PQ_KERNELS``.  Arguments are checked before anything touches the device."""
    ymd = _c(ymd, np.int32)
    prcp, tavg = _pq_series("prcp", prcp, ymd), _pq_series("tavg", tavg, ymd)
    if tavg.shape != prcp.shape:
        raise ValueError("prcp and tavg must have one shape")
    nstn, ndays = prcp.shape
    flag = np.zeros((nstn, ndays), np.uint8)
    pct = np.empty((nstn, PQ_PCTILE_ROWS, PQ_PCTILE_COLS)) if details else None
    ms = _call("twxpq_non_spatial", (int(device), nstn, ndays, prcp.ctypes.data, tavg.ctypes.data, ymd.ctypes.data,
                                     int(bool(streak)), int(bool(frequent)), flag.ctypes.data,
                                     pct.ctypes.data if details else None), len(PQ_KERNELS))
    _put_times(timing, _ms_keys(PQ_KERNELS), ms)
    return (flag, pct) if details else flag


def prcp_percentiles(vals, ymd, device=0, timing=None):
    """``twxpq_percentiles``: ``_build_percentiles(vals, days, DATES_366)`` (qa_prcp.py:790-812) of every row of vals
    [nstn, ndays] float32 (NaN = missing).  Returns [nstn, 366, 5] float64; a row with fewer than 20 values > 0 is NaN."""
    ymd = _c(ymd, np.int32)
    vals = _pq_series("vals", vals, ymd)
    pct = np.empty((vals.shape[0], PQ_PCTILE_ROWS, PQ_PCTILE_COLS))
    ms = _call("twxpq_percentiles", (int(device), vals.shape[0], vals.shape[1], vals.ctypes.data, ymd.ctypes.data,
                                     pct.ctypes.data), 1)
    _put_times(timing, ("pq_pctiles_kernel_ms",), ms)
    return pct


# ---- the precipitation QA's spatial corroboration check (twxpc_*; TWXPC_* of include/twx_qa.h) ----
PC_EXPORTS = ("twxpc_spatial_corrob", "twxpc_pors_counts")
PC_KERNELS = ("pc_radius", "pc_rowcounts", "pc_walk", "pc_rank")     # TWXPC_NKERNELS


def prcp_spatial_corrob(lon, lat, prcp, ymd, target_idx, flags, device=0, details=False, timing=None):
    """``twxpc_spatial_corrob``: ``_qa_spatial_corrob`` (qa_prcp.py:614-664) of the targets ``target_idx`` (rows of the pool)
    in one call.  lon, lat [nstn]; prcp [nstn, ndays] float32, station-major, NaN = missing; ymd [ndays] consecutive days;
    flags [ntarget, ndays] uint8, the working copy: a target's series is the pool value where its flag is 1.  Returns
    ``(flags, status)``: a copy of the flags with 17 where a day is flagged and the flag was 1, and status [ntarget] int32
    (``SP_OK``, ``SP_FEW_NGHS``, ``SP_NGH_CAP``); with ``details`` also ``abs_dif``, ``pctile``, ``thres`` [ntarget, ndays]
    float64, NaN where the day did not reach that step.  ``timing`` receives ``<kernel>_kernel_ms`` for the names in
    ``PC_KERNELS``.  Arguments are checked before anything touches the device."""
    ymd = _c(ymd, np.int32)
    prcp = _pq_series("prcp", prcp, ymd)
    lon, lat = _c(lon, np.float64), _c(lat, np.float64)
    nstn, ndays = prcp.shape
    if lon.shape != (nstn,) or lat.shape != (nstn,):
        raise ValueError("lon / lat must be [nstn]")
    tgt = np.asarray(target_idx)
    if tgt.ndim != 1 or tgt.size < 1 or not np.issubdtype(tgt.dtype, np.integer):
        raise ValueError("target_idx must be a 1-d integer array with at least one entry")
    if tgt.min() < 0 or tgt.max() >= nstn:
        raise ValueError("target_idx outside 0 .. nstn - 1")
    tgt = _c(tgt, np.int32)
    fl = np.array(flags, np.uint8, order="C")                    # a copy: the input is not modified
    if fl.shape != (tgt.size, ndays):
        raise ValueError("flags must be [ntarget, ndays]")
    status = np.zeros(tgt.size, np.int32)
    det = [np.empty((tgt.size, ndays)) for _ in range(3)] if details else [None] * 3
    ms = _call("twxpc_spatial_corrob",
               (int(device), nstn, ndays, lon.ctypes.data, lat.ctypes.data, prcp.ctypes.data, ymd.ctypes.data, tgt.size,
                tgt.ctypes.data, fl.ctypes.data, status.ctypes.data, *[d.ctypes.data if details else None for d in det]),
               len(PC_KERNELS))
    _put_times(timing, _ms_keys(PC_KERNELS), ms)
    return (fl, status) + tuple(det) if details else (fl, status)


def prcp_pors_counts(vals, ymd, device=0, timing=None):
    """``twxpc_pors_counts``: the sizes of ``_build_pors``' rows (qa_prcp.py:675-681) of every row of vals [nstn, ndays]
    float32 (NaN = missing).  Returns [nstn, 366] uint16."""
    ymd = _c(ymd, np.int32)
    vals = _pq_series("vals", vals, ymd)
    cnt = np.empty((vals.shape[0], PQ_PCTILE_ROWS), np.uint16)
    ms = _call("twxpc_pors_counts", (int(device), vals.shape[0], vals.shape[1], vals.ctypes.data, ymd.ctypes.data,
                                     cnt.ctypes.data), 1)
    _put_times(timing, ("pc_rowcounts_kernel_ms",), ms)
    return cnt


# ---- the GHCN-Daily ingest of step04 (twxgh_*; TWXGH_* of include/twx_qa.h) ----
GH_EXPORTS = ("twxgh_parse_dly", "twxgh_parse_tobs", "twxgh_host_alloc", "twxgh_host_free")
GH_KERNELS = ("gh_fill", "gh_index", "gh_claim", "gh_write")     # TWXGH_NKERNELS
GH_MAX_BYTES = 2147483584             # TWXGH_MAX_BYTES
GH_FB_WORDS = 8                       # TWXGH_FB_WORDS
GH_NO_BAD_HEADER = 0xffffffff         # TWXGH_NO_BAD_HEADER
GH_ELEMENTS = ("TMIN", "TMAX", "PRCP")
GH_MISSING = -9999.0


def _gh_buffer(buf, file_off):
    """(address, nbytes, file_off int64) of a byte buffer and its file offsets, checked."""
    off = _c(file_off, np.int64)
    if off.ndim != 1 or off.size < 2 or off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("file_off must be [nfiles + 1] int64, from 0, not decreasing")
    mv = memoryview(buf).cast("B")
    if mv.nbytes < int(off[-1]):
        raise ValueError("the buffer holds %d bytes, file_off ends at %d" % (mv.nbytes, int(off[-1])))
    if int(off[-1]) > GH_MAX_BYTES:
        raise ValueError("a call takes at most TWXGH_MAX_BYTES = %d bytes" % GH_MAX_BYTES)
    a = np.frombuffer(mv, np.uint8)
    return a, int(off[-1]), off


def ghcn_parse_dly(buf, file_off, file_col, nrows, min_ymd, max_ymd, ndays, fallback_cap=4096, device=0, timing=None):
    """``twxgh_parse_dly``: ``InsertGhcn.parse_stn_obs`` (create_db_all_stations.py:1042-1103) of the .dly files laid end to
    end in ``buf`` (any object with the buffer protocol) at ``file_off`` [nfiles + 1]; file f fills row ``file_col[f]``.
    Returns ``(val [3, nrows, ndays] float32, qflag [3, nrows, ndays] uint8, bad_header [nfiles] uint32, fallback [n, 8]
    uint32, counts [3] int64)`` as include/twx_qa.h describes them; the call is repeated once with room for every
    fallback entry if ``fallback_cap`` was too small.  Arguments are checked before anything touches the device."""
    a, nbytes, off = _gh_buffer(buf, file_off)
    col = _c(file_col, np.int32)
    nfiles = off.size - 1
    nrows, ndays = int(nrows), int(ndays)
    if col.shape != (nfiles,) or nrows < 1 or (nfiles and (col.min() < 0 or col.max() >= nrows)) or np.unique(col).size != nfiles:
        raise ValueError("file_col must be [nfiles] distinct rows in 0 .. nrows - 1")
    if ndays < 1:
        raise ValueError("ndays must be the number of days from min_ymd to max_ymd")
    cap = int(fallback_cap)
    while True:
        val = np.empty((3, nrows, ndays), np.float32)
        qf = np.empty((3, nrows, ndays), np.uint8)
        bad = np.empty(nfiles, np.uint32)
        fb = np.zeros((max(cap, 1), GH_FB_WORDS), np.uint32)
        counts = np.zeros(3, np.int64)
        ms = _call("twxgh_parse_dly",
                   (int(device), a.ctypes.data if nbytes else None, nbytes, nfiles, off.ctypes.data, col.ctypes.data, nrows,
                    int(min_ymd), int(max_ymd), ndays, val.ctypes.data, qf.ctypes.data, bad.ctypes.data, fb.ctypes.data, cap),
                   len(GH_KERNELS), counts)
        _put_times(timing, _ms_keys(GH_KERNELS), ms, add=True)
        if counts[2] <= cap:
            return val, qf, bad, fb[:int(counts[2])].copy(), counts
        cap = int(counts[2])


def ghcn_parse_tobs(buf, file_off, ids11, element, min_ymd, max_ymd, win0, tobs, bad_cap=4096, device=0, timing=None):
    """``twxgh_parse_tobs``: ``create_tobs_db`` (tobs.py:121-157) on the by-year CSV files laid end to end in ``buf``.
    ``ids11``: the sorted station ids without ``GHCN_`` (``"S11"``); ``tobs`` [nstn, nwin] int16, the days ``win0 .. win0 +
    nwin - 1`` of the period, updated IN PLACE.  Returns ``(bad [n, 2] uint32, counts [5] int64)``: counts are values,
    dates outside the period, dates outside the window, bad lines, lines."""
    a, nbytes, off = _gh_buffer(buf, file_off)
    ids = np.ascontiguousarray(ids11, "S11")
    if ids.ndim != 1 or ids.size < 1 or np.any(ids[1:] <= ids[:-1]):
        raise ValueError("ids11 must be a sorted 1-d array of distinct ids")
    if not (isinstance(tobs, np.ndarray) and tobs.dtype == np.int16 and tobs.flags.c_contiguous and tobs.flags.writeable and
            tobs.ndim == 2 and tobs.shape[0] == ids.size and tobs.shape[1] >= 1):
        raise ValueError("tobs must be a C-contiguous writeable int16 array [nstn, nwin]")
    elem = str(element).encode()
    if len(elem) != 4:
        raise ValueError("the element is four characters")
    table = np.zeros((ids.size, 11), np.uint8)
    for k, s in enumerate(ids):
        table[k, :len(s)] = np.frombuffer(s, np.uint8)
    cap = int(bad_cap)
    keep = tobs.copy()
    while True:
        bad = np.zeros((max(cap, 1), 2), np.uint32)
        counts = np.zeros(5, np.int64)
        ms = _call("twxgh_parse_tobs",
                   (int(device), a.ctypes.data if nbytes else None, nbytes, off.size - 1, off.ctypes.data, ids.size,
                    table.ctypes.data, elem, int(min_ymd), int(max_ymd), int(win0), tobs.shape[1], tobs.ctypes.data,
                    bad.ctypes.data, cap), len(GH_KERNELS), counts)
        _put_times(timing, _ms_keys(GH_KERNELS), ms, add=True)
        if counts[3] <= cap:
            return bad[:int(counts[3])].copy(), counts
        cap = int(counts[3])
        tobs[:] = keep


class PinnedBuffer(object):
    """``nbytes`` of page-locked host memory (``twxgh_host_alloc``) with the buffer protocol: ``view`` is a writable
    memoryview, ``close()`` releases it."""

    def __init__(self, nbytes):
        lib = load()
        self._lib, self.nbytes = lib, int(nbytes)
        self._p = lib.twxgh_host_alloc(self.nbytes)
        if not self._p:
            raise QaError("twxgh_host_alloc(%d) failed" % self.nbytes)
        self.view = memoryview((C.c_ubyte * self.nbytes).from_address(self._p)).cast("B")

    def close(self):
        if self._p:
            try:
                self.view.release()
            except BufferError:                                    # still exported somewhere: keep the memory, try again later
                return
            self._lib.twxgh_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the reanalysis subsets of step12 (twxns_subset; TWXNS_* of include/twx_qa.h) ----
NS_EXPORTS = ("twxns_subset",)
NS_KERNELS = ("nsub_upload", "nsub_kernels", "nsub_download")          # TWXNS_NKERNELS
NS_I16, NS_F32 = 0, 1                 # TWXNS_I16, TWXNS_F32
NS_TILED, NS_PLAIN = 0, 1             # TWXNS_TILED, TWXNS_PLAIN
NS_CONV = {"none": 0, "k_to_c": 1}    # TWXNS_CONV_*
NS_KIND_LEVELS, NS_KIND_THICK = 0, 1  # TWXNS_KIND_*
NS_MAX_LEV = 32                       # TWXNS_MAX_LEV
NS_MAX_PROD = 64                      # TWXNS_MAX_PROD
NS_MAX_DAYS = 1 << 20                 # TWXNS_MAX_DAYS
NS_MAX_SIDE = 4096                    # TWXNS_MAX_SIDE
NS_PD_WORDS = 4 + NS_MAX_LEV          # TWXNS_PD_WORDS
NS_C_DAYS, NS_C_MARKED, NS_C_UNWRITTEN = 0, 1, 2                 # TWXNS_C_*
NS_FILL = np.float32(9.969209968386869e36)                       # TWXNS_FILL


def ns_out_shape(layout, ndays, nlev, nlat_out, nlon_out):
    """The shape of one product of ``ns_subset`` in a layout."""
    if layout == NS_TILED:
        return ((nlat_out + 3) // 4, (nlon_out + 3) // 4, ndays, nlev, 4, 4)
    return (ndays, nlev, nlat_out, nlon_out)


def ns_subset(raw, scale, offset, marks, rec_slot, rec_day, ndays, lat_idx, lon_idx, products, layout=NS_TILED, dtype=None,
              device=0, timing=None):
    """``twxns_subset``: every product of one raw reanalysis variable from one upload of its records.

    ``raw`` [nrec, nl, ny, nx] (or [nrec, ny, nx]) int16 or float32, the STORED values; ``scale`` / ``offset``: the packing
    (1 and 0 for none); ``marks``: ``(missing_value, _FillValue)``, ``None`` for an absent one; ``rec_slot`` / ``rec_day``
    [nrec]: 0 / 1 / 2 (12z, 18z, 24z) or -1, and the output day or -1; ``lat_idx`` / ``lon_idx``: raw rows / columns of the
    output; ``products``: dicts with ``slot``, either ``levels`` (level indices) or ``thick`` = (idx_up, idx_low), and
    ``conv`` ("none" / "k_to_c").  Returns ``(outs, counts)``: per product a float32 array of ``ns_out_shape`` and
    ``counts`` [nprod, 3] int64 (days with a record, values filled for a mark, days unwritten).  What the library refuses
    (include/twx_qa.h) raises ``QaError`` before anything touches the device."""
    raw = np.asarray(raw)
    if dtype is None:
        if raw.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
            raise ValueError("raw must be int16 or float32, not %s" % raw.dtype)
        dtype = NS_I16 if raw.dtype == np.int16 else NS_F32
    if raw.ndim == 3:
        raw = raw[:, None]
    if raw.ndim != 4 or not raw.flags.c_contiguous or raw.dtype.byteorder not in "=|":
        raise ValueError("raw must be a C-contiguous native [nrec, nl, ny, nx] array")
    nrec, nl, ny, nx = raw.shape
    slot, day = _c(rec_slot, np.int32), _c(rec_day, np.int32)
    lat, lon = _c(lat_idx, np.int32), _c(lon_idx, np.int32)
    if slot.shape != (nrec,) or day.shape != (nrec,) or lat.ndim != 1 or lon.ndim != 1:
        raise ValueError("rec_slot / rec_day must be [nrec], lat_idx / lon_idx 1-d")
    mk = np.zeros(2, raw.dtype if raw.dtype.itemsize in (2, 4) else np.float32)
    has = np.zeros(2, np.int32)
    for k, m in enumerate(tuple(marks) + (None,) * (2 - len(tuple(marks)))):
        if m is not None:
            mk[k], has[k] = m, 1
    nprod = len(products)
    pd = np.zeros((max(nprod, 1), NS_PD_WORDS), np.int32)
    nlevs = []
    for p, d in enumerate(products):
        if d.get("conv", "none") not in NS_CONV:
            raise ValueError("conv must be 'none' or 'k_to_c'")
        pd[p, 0], pd[p, 2] = int(d["slot"]), NS_CONV[d.get("conv", "none")]
        if d.get("thick") is not None:
            pd[p, 1], pd[p, 3] = NS_KIND_THICK, 1
            pd[p, 4:6] = d["thick"]
            nlevs.append(1)
        else:
            lv = np.asarray(d["levels"], np.int32).ravel()
            pd[p, 1], pd[p, 3] = NS_KIND_LEVELS, lv.size
            pd[p, 4:4 + min(lv.size, NS_MAX_LEV)] = lv[:NS_MAX_LEV]
            nlevs.append(max(1, min(int(lv.size), NS_MAX_LEV)))
    ndays = int(ndays)
    big = not (1 <= ndays <= NS_MAX_DAYS and 1 <= lat.size <= NS_MAX_SIDE and 1 <= lon.size <= NS_MAX_SIDE and
               1 <= nprod <= NS_MAX_PROD)                      # the library refuses these: no buffer of such a size is made
    shapes = [(1,) if big else ns_out_shape(layout, ndays, n, lat.size, lon.size) if layout in (NS_TILED, NS_PLAIN) else (1,)
              for n in nlevs]
    outs = [np.empty(s, np.float32) for s in shapes] or [np.empty(1, np.float32)]
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    counts = np.zeros((max(nprod, 1), 3), np.int64)
    ms = _call("twxns_subset",
               (int(device), int(dtype), raw.ctypes.data, nrec, nl, ny, nx, float(np.float32(scale)), float(np.float32(offset)),
                mk.ctypes.data, has.ctypes.data, slot.ctypes.data, day.ctypes.data, ndays, lat.size, lat.ctypes.data, lon.size,
                lon.ctypes.data, nprod, pd.ctypes.data, int(layout), C.addressof(ptrs)), len(NS_KERNELS), counts)
    _put_times(timing, _ms_keys((), NS_KERNELS), ms, add=True)
    return outs, counts[:nprod]


# ---- step13's time-zone lookup (twxtz_locate; TWXTZ_* of include/twx_qa.h) ----
TZ_EXPORTS = ("twxtz_locate",)
TZ_PHASES = ("tz_upload", "tz_candidates", "tz_contain", "tz_forced", "tz_download")          # TWXTZ_NPHASES
TZ_INSIDE, TZ_FORCED, TZ_NONE, TZ_BAD_POINT, TZ_UNCERTAIN, TZ_PENDING = 0, 1, 2, 3, 4, 5     # TWXTZ_* statuses
TZ_OVERFLOW = 1                       # TWXTZ_OVERFLOW
TZ_CHUNK_EDGES = 2048                 # TWXTZ_CHUNK_EDGES
TZ_C_PAIRS, TZ_C_ITEMS, TZ_C_PENDING, TZ_C_UNCERTAIN = 0, 1, 2, 3                            # TWXTZ_C_*


def tz_locate(lon, lat, edge_off, bbox, edges, max_force_deg=1.0, uncertain_cap=4096, device=0, timing=None):
    """``twxtz_locate``: for every point the first polygon that contains it (even-odd rule over the polygon's edges),
    otherwise the nearest within ``max_force_deg`` degrees (``None``: any distance).

    ``lon`` / ``lat`` [npt] float64; ``edge_off`` [npoly + 1] int64, ``bbox`` [npoly, 4], ``edges`` [nedge, 4] float64 as
    ``utc_offsets.load_tz_polygons`` returns them.  Returns ``(poly, status, dist2, uncertain [n, 2], counts [4])`` as
    include/twx_qa.h describes them: points with status ``TZ_UNCERTAIN`` are NOT decided, ``uncertain`` lists what the
    caller has to decide exactly (``utc_offsets.UtcOffset`` does).  The call is repeated with room for every entry if
    ``uncertain_cap`` was too small.  Arguments are checked before anything touches the device."""
    lon, lat = _c(lon, np.float64).ravel(), _c(lat, np.float64).ravel()
    off, bb, ed = _c(edge_off, np.int64), _c(bbox, np.float64), _c(edges, np.float64)
    if lat.shape != lon.shape:
        raise ValueError("lon / lat must be [npt]")
    if off.ndim != 1 or off.size < 1 or bb.shape != (off.size - 1, 4) or ed.ndim != 2 or ed.shape[1:] != (4,) or \
            (off.size and int(off[-1]) != ed.shape[0]):
        raise ValueError("need edge_off [npoly + 1] ending at nedge, bbox [npoly, 4] and edges [nedge, 4]")
    mf = float("inf") if max_force_deg is None else float(max_force_deg)
    npt, cap = lon.size, int(uncertain_cap)
    while True:
        poly, status, d2 = np.empty(npt, np.int32), np.empty(npt, np.int32), np.empty(npt, np.float64)
        unc = np.zeros((max(cap, 1), 2), np.int32)
        counts = np.zeros(4, np.int64)
        ms = _call("twxtz_locate",
                   (int(device), npt, lon.ctypes.data, lat.ctypes.data, off.size - 1, off.ctypes.data, bb.ctypes.data,
                    ed.ctypes.data if ed.size else None, mf, poly.ctypes.data, status.ctypes.data, d2.ctypes.data,
                    unc.ctypes.data, cap), len(TZ_PHASES), counts, ok=(0, TZ_OVERFLOW))
        _put_times(timing, _ms_keys((), TZ_PHASES), ms, add=True, tz_calls=1)
        if counts[TZ_C_UNCERTAIN] <= cap:                          # otherwise the entry returned TZ_OVERFLOW: the list was too small
            return poly, status, d2, unc[:int(counts[TZ_C_UNCERTAIN])].copy(), counts
        cap = int(counts[TZ_C_UNCERTAIN])


# ---- step26 / step27: mosaics deflated on the device (twxmo_*; TWXMO_* of include/twx_qa.h) ----
MO_EXPORTS = ("twxmo_sizes", "twxmo_create", "twxmo_destroy", "twxmo_last_error", "twxmo_clear", "twxmo_place", "twxmo_staging",
              "twxmo_monthly", "twxmo_deflate", "twxmo_download", "twxmo_timing")
MO_DAILY, MO_MONTHLY = 0, 1                                                                        # TWXMO_DAILY / TWXMO_MONTHLY
MO_GROUPS = ("clear", "place", "hist_table", "count_scan", "emit", "compact", "aggregate")         # TWXMO_NGROUPS
MO_SIZES = ("Yp", "Xp", "nchunk", "nseg", "slot_bytes", "device_bytes", "pinned_bytes", "vec")     # TWXMO_S_*
MO_FILL_I2 = np.int16(-32767)


def mosaic_sizes(max_days, Y, X, chunk_y, chunk_x):
    """``twxmo_sizes``: dict of ``MO_SIZES`` for an object with these arguments (no device needed); ValueError when the library
    refuses them."""
    sz = np.zeros(len(MO_SIZES), np.int64)
    buf = C.create_string_buffer(512)
    if load().twxmo_sizes(int(max_days), int(Y), int(X), int(chunk_y), int(chunk_x), sz.ctypes.data, buf, 512) != 0:
        raise ValueError(buf.value.decode(errors="replace"))
    return {k: int(v) for k, v in zip(MO_SIZES, sz)}


class Mosaic(object):
    """A mosaic resident on the GPU (twxmo_create / twxmo_destroy): an int16 image ``[max_days, Yp, Xp]`` -- ``Y``, ``X``
    rounded up to whole ``(chunk_y, chunk_x)`` chunks, the padding at the fill value --, a monthly image ``[12, Yp, Xp]`` and the
    workspace of the deflate coder.  ``clear``, then ``place`` tile slabs, then ``deflate`` gives the HDF5 chunk bytes of the
    days in file order; ``monthly`` forms the twelve monthly means of the resident days, ``deflate(monthly=True)`` their chunks.
    QaError with the library's message when the object does not fit the device: ask for fewer days."""

    def __init__(self, max_days, Y, X, chunk_y, chunk_x, device=0):
        self.sizes = mosaic_sizes(max_days, Y, X, chunk_y, chunk_x)
        self.max_days, self.Y, self.X, self.cy, self.cx = int(max_days), int(Y), int(X), int(chunk_y), int(chunk_x)
        self.Yp, self.Xp, self.nchunk = self.sizes["Yp"], self.sizes["Xp"], self.sizes["nchunk"]
        self.lib = load()
        h = C.c_void_p()
        buf = C.create_string_buffer(512)
        self.h = None
        if self.lib.twxmo_create(int(device), self.max_days, self.Y, self.X, self.cy, self.cx, C.byref(h), buf, 512) != 0:
            raise QaError(buf.value.decode(errors="replace"))
        self.h = h
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.twxmo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise QaError("%s failed: %s" % (what, self.lib.twxmo_last_error(self.h).decode(errors="replace")))

    def chunk_origins(self, nlayers):
        """[(layer, row, column)] of the streams ``deflate`` returns for ``nlayers`` layers: the ``write_chunk_raw`` offsets."""
        return [(d, r0, c0) for d in range(nlayers) for r0 in range(0, self.Yp, self.cy) for c0 in range(0, self.Xp, self.cx)]

    def clear(self, ndays):
        self._chk(self.lib.twxmo_clear(self.h, int(ndays)), "twxmo_clear")

    def staging(self, shape):
        """An int16 array of ``shape`` over the pinned buffer the next ``place`` uploads from: fill it, then pass it to ``place``."""
        n = int(np.prod(shape, dtype=np.int64))
        p = C.c_void_p()
        self._chk(self.lib.twxmo_staging(self.h, n * 2, C.byref(p)), "twxmo_staging")
        return np.frombuffer((C.c_char * (n * 2)).from_address(p.value), np.int16, n).reshape(shape)

    def place(self, slab, y0, x0):
        """``slab`` int16 [nd, ty, tx] at row ``y0``, column ``x0`` of layers 0 .. nd - 1; a slab that leaves Y x X is refused."""
        a = np.asarray(slab)
        if a.dtype != np.int16 or a.ndim != 3:
            raise TypeError("place takes an int16 slab [nd, ty, tx]")
        a = np.ascontiguousarray(a)
        if not (-2 ** 31 <= int(y0) < 2 ** 31 and -2 ** 31 <= int(x0) < 2 ** 31):
            raise QaError("twxmo_place failed: the slab lies outside the mosaic")
        self._chk(self.lib.twxmo_place(self.h, a.ctypes.data, a.shape[0], a.shape[1], a.shape[2], int(y0), int(x0)),
                  "twxmo_place")

    def monthly(self, ndays, day_month):
        dm = _c(day_month, np.int32)
        if dm.shape != (int(ndays),):
            raise ValueError("day_month must be [ndays]")
        self._chk(self.lib.twxmo_monthly(self.h, int(ndays), dm.ctypes.data), "twxmo_monthly")

    def deflate(self, nlayers, monthly=False, with_offset=False):
        """List of uint8 views, one zlib stream per (layer, chunk row, chunk column) in that order -- views of the object's pinned
        block, valid until the next ``deflate``.  ``with_offset``: also the int64 offsets [n + 1] of the streams in that block."""
        s = TwxmoStreams()
        self._chk(self.lib.twxmo_deflate(self.h, MO_MONTHLY if monthly else MO_DAILY, int(nlayers), C.byref(s)), "twxmo_deflate")
        n = int(s.nstreams)
        off = np.ctypeslib.as_array(s.offset, shape=(n + 1,)).copy()
        whole = np.frombuffer((C.c_char * int(off[-1])).from_address(s.data), np.uint8)
        if int(np.diff(off).max()) > int(s.slot_bytes):
            raise QaError("twxmo_deflate: a stream is longer than its slot")
        out = [whole[off[k]:off[k + 1]] for k in range(n)]
        return (out, off) if with_offset else out

    def download(self, nlayers, monthly=False):
        """The padded image int16 [nlayers, Yp, Xp] (debug / tests)."""
        out = np.empty((int(nlayers), self.Yp, self.Xp), np.int16)
        self._chk(self.lib.twxmo_download(self.h, MO_MONTHLY if monthly else MO_DAILY, int(nlayers), out.ctypes.data),
                  "twxmo_download")
        return out

    def timing(self):
        """{group + '_ms': device time since the last ``clear``} plus ``device_bytes`` / ``pinned_bytes`` held now."""
        ms = (C.c_float * len(MO_GROUPS))()
        db, pb = C.c_int64(), C.c_int64()
        self._chk(self.lib.twxmo_timing(self.h, C.addressof(ms), C.addressof(db), C.addressof(pb)), "twxmo_timing")
        out = {g + "_ms": float(ms[k]) for k, g in enumerate(MO_GROUPS)}
        out["device_bytes"], out["pinned_bytes"] = db.value, pb.value
        return out


def mosaic_max_days(Y, X, chunk_y, chunk_x, free_bytes, want_days, margin=1 << 30):
    """Largest ``max_days <= want_days`` whose object (``mosaic_sizes``: images, slots, workspace) plus a packed block as large as
    the slots fits ``free_bytes`` less ``margin``; 0 when not even one day does."""
    def fits(nd):
        s = mosaic_sizes(nd, Y, X, chunk_y, chunk_x)
        return s["device_bytes"] + nd * s["nchunk"] * s["slot_bytes"] + margin <= free_bytes
    lo, hi = 0, int(want_days)
    if fits(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def device_free_bytes(device=0):
    """Free device memory as hipMemGetInfo reports it (``twx_device_memory`` of libtwxhip, on a context of its own)."""
    from . import _lib
    ctx = _lib.Context(device)
    try:
        return int(ctx.device_memory()[0])
    finally:
        ctx.close()
