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
EXPORTS = ("twxqa_outlier_wls",)

_LIB = None


class QaError(RuntimeError):
    pass


def load():
    """Load libtwxqa.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise QaError("%s not found: build it with ./build.sh (hipcc --offload-arch=gfx950); "
                          "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.twxqa_outlier_wls.restype = C.c_int
        L.twxqa_outlier_wls.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int32] + \
            [C.c_void_p] * 6 + [C.c_char_p, C.c_int]
        _LIB = L
    return _LIB


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def outlier_wls(lon, lat, elev, lst13, norm13, pt, idx, wgt, knn_status, device=0, timing=None):
    """``twxqa_outlier_wls``: leave-one-out WLS errors of ``XvalOutlier.run_xval_stn`` (optimize.py:113-153).

    lon, lat, elev [nstn], lst13 / norm13 [13, nstn]: the pool (row 12 = annual means); pt [npts, 29]: the left-out
    stations; idx / wgt [npts, k] and knn_status [npts]: their neighbours as ``_lib.Context.knn`` returns them.
    Returns (err [npts, 13], status [npts, 13]); ``timing`` (a dict) receives the kernel's device time as ``kernel_ms``."""
    L = load()
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
    ms = C.c_float(0.0)
    buf = C.create_string_buffer(512)
    rc = L.twxqa_outlier_wls(int(device), nstn, lon.ctypes.data, lat.ctypes.data, elev.ctypes.data, lst13.ctypes.data,
                             norm13.ctypes.data, npts, pt.ctypes.data, k, idx.ctypes.data, wgt.ctypes.data,
                             knn_status.ctypes.data, err.ctypes.data, status.ctypes.data, C.addressof(ms), buf, 512)
    if rc != 0:
        raise QaError("twxqa_outlier_wls failed: %s" % buf.value.decode(errors="replace"))
    if timing is not None:
        timing["kernel_ms"] = float(ms.value)
    return err, status
