"""The stored bytes of the ``(ndays, 1)`` chunks of a station database, formed on the GPU.

The reference stores every ``(time, station_id)`` variable of its station databases with ``zlib=True, chunksizes=(ndays,
1)`` (twx/db/create_db_all_stations.py:307-311, 399-435): a chunk is the shuffled and deflated series of one station, and
libhdf5 deflates it on one core.  ``deflate_series`` turns station-major rows into those chunk bytes with the kernels of
``topowx_amd/qa/twxsd_serdeflate.hip`` (``twxsd_deflate``, include/twx_series_deflate.h): one zlib stream per row, any
inflate reads it; ``ncio.write_series_chunks`` appends them with ``write_chunk_raw``.  There is no CPU fallback.

One Huffman code per (call, byte plane): a batch is a call, so the streams depend on ``batch_bytes`` (and on nothing
else: two runs give the same bytes).
"""
import ctypes as C

import numpy as np

from . import _qalib

__all__ = ["deflate_series", "deflate_rows", "bound", "shuffled", "SeriesDeflateCap", "SD_KERNELS", "SD_COUNTS", "BATCH_BYTES"]

# ---- the unit's entries (twxsd_*; TWXSD_* of include/twx_series_deflate.h), bound here: the unit has a header of its own ----
SD_BOUND, SD_ENTRY = "twxsd_bound", "twxsd_deflate"
SD_PROTOTYPES = {
    SD_BOUND: (C.c_int64, [C.c_int64, C.c_int32]),
    SD_ENTRY: (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                         C.c_void_p, C.c_char_p, C.c_int]),
}
SD_KERNELS = ("sd_hist", "sd_count", "sd_scan", "sd_emit")            # TWXSD_NKERNELS
SD_HOST_TIMES = ("sd_upload", "sd_download")                           # the rest of TWXSD_NTIMES: host-clock milliseconds
SD_OK, SD_E_CAP = 0, 2                                                 # TWXSD_OK, TWXSD_E_CAP
SD_COUNTS = ("blocks", "stored", "halvings0", "halvings1", "halvings2", "halvings3", "bytes_in", "bytes_out")      # TWXSD_C_*
SD_SEG = 16384                                                         # TWXSD_SEG
BATCH_BYTES = 256 << 20


class SeriesDeflateCap(_qalib.QaError):
    """The packed streams need ``needed`` bytes, more than the buffer given (``TWXSD_E_CAP``)."""

    def __init__(self, msg, needed):
        _qalib.QaError.__init__(self, msg)
        self.needed = needed


def _bind():
    """Give the entries their prototypes in the loaded library; raises if the library lacks one (no fallback)."""
    lib = _qalib.load()
    for name, (restype, argtypes) in SD_PROTOTYPES.items():
        if not hasattr(lib, name):
            raise _qalib.QaError("%s has no %s: it is older than this binding, run ./build.sh" % (_qalib.LIB_PATH, name))
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bound(n, es):
    """``twxsd_bound``: the longest stream of a row of ``n`` elements of ``es`` bytes, ``2 + es (n + 5 ceil(n / 16384)) +
    9``; ``ValueError`` for arguments the entry refuses."""
    n, es = int(n), int(es)
    if es not in (1, 2, 4) or n < 1 or es * n >= 1 << 31:
        raise ValueError("a row has n >= 1 elements of 1, 2 or 4 bytes, es * n < 2^31")
    return 2 + es * (n + 5 * ((n + SD_SEG - 1) // SD_SEG)) + 9


def shuffled(row):
    """HDF5's shuffle of one row (the test helper): uint8 [es * n], plane p = byte p of every element."""
    a = np.ascontiguousarray(row).reshape(-1)
    return np.ascontiguousarray(a.view(np.uint8).reshape(a.size, a.dtype.itemsize).T).reshape(-1)


def _check_rows(rows):
    if not isinstance(rows, np.ndarray) or rows.ndim != 2 or not rows.flags.c_contiguous or rows.dtype.itemsize not in (1, 2, 4):
        raise ValueError("rows must be a C-contiguous 2-D array [nrows, n] of itemsize 1, 2 or 4")
    if rows.shape[1] < 1:
        raise ValueError("a row has n >= 1 elements")
    bound(rows.shape[1], rows.dtype.itemsize)
    return rows


def deflate_rows(rows, out=None, device=0, timing=None):
    """ONE ``twxsd_deflate`` call: ``rows`` [nrows, n] -> ``(out, offsets [nrows + 1] int64, counts [8] int64)``; row r's
    stream is ``out[offsets[r]:offsets[r + 1]]``.  ``out``: a writable buffer (a ``_qalib.PinnedBuffer``'s ``view``, a uint8
    array) that receives the packed streams -- ``SeriesDeflateCap`` (with ``needed``) if it is too small, nothing is written
    then; by default an array of ``nrows * bound`` bytes, which always suffices.  ``timing`` (a dict) accumulates
    ``<kernel>_kernel_ms`` for ``SD_KERNELS``, ``sd_upload_ms`` / ``sd_download_ms`` and the counts as ``sd_<name>``.
    Arguments are checked before the library is loaded."""
    rows = _check_rows(rows)
    if int(device) < 0:
        raise ValueError("device must not be negative")
    nrows, n = rows.shape
    es = rows.dtype.itemsize
    if out is None:
        out = np.empty(nrows * bound(n, es), np.uint8)
    mv = memoryview(out).cast("B")
    if mv.readonly:
        raise ValueError("out must be writable")
    o = np.frombuffer(mv, np.uint8)
    offsets, counts = np.zeros(nrows + 1, np.int64), np.zeros(len(SD_COUNTS), np.int64)
    lib = _bind()
    ms = (C.c_float * (len(SD_KERNELS) + len(SD_HOST_TIMES)))()
    buf = C.create_string_buffer(512)
    rc = getattr(lib, SD_ENTRY)(int(device), rows.ctypes.data if nrows else None, nrows, n, es, o.ctypes.data if o.size else None,
                                o.size, offsets.ctypes.data, counts.ctypes.data, C.addressof(ms), buf, 512)
    if rc == SD_E_CAP:
        raise SeriesDeflateCap("%s: %s" % (SD_ENTRY, buf.value.decode(errors="replace")), int(counts[7]))
    if rc != SD_OK:
        raise _qalib.QaError("%s failed: %s" % (SD_ENTRY, buf.value.decode(errors="replace")))
    _qalib._put_times(timing, _qalib._ms_keys(SD_KERNELS, SD_HOST_TIMES), [float(v) for v in ms], add=True,
                      **{"sd_" + k: int(v) for k, v in zip(SD_COUNTS, counts)})
    return o, offsets, counts


def deflate_series(rows, device=0, batch_bytes=BATCH_BYTES, timing=None, pinned=None):
    """The chunk bytes of station-major ``rows`` [nrows, n] (C-contiguous, itemsize 1, 2 or 4): ``(packed uint8, offsets
    [nrows + 1] int64)``, row r's zlib stream is ``packed[offsets[r]:offsets[r + 1]]``.  The rows go to the device in batches
    of at most ``batch_bytes`` of input (at least one row), a ``twxsd_deflate`` call and a Huffman code per plane each.
    ``pinned``: a ``_qalib.PinnedBuffer`` that every batch's streams come down into (it must hold a batch's streams:
    ``SeriesDeflateCap`` otherwise); by default ordinary memory.  ``timing`` as ``deflate_rows``, and ``sd_batches``."""
    rows = _check_rows(rows)
    if int(batch_bytes) < 1:
        raise ValueError("batch_bytes must be positive")
    nrows, n = rows.shape
    per = max(1, int(batch_bytes) // (n * rows.dtype.itemsize))
    pieces, offsets, at = [], np.zeros(nrows + 1, np.int64), 0
    for i0 in range(0, nrows, per):
        i1 = min(nrows, i0 + per)
        o, off, _ = deflate_rows(rows[i0:i1], out=None if pinned is None else pinned.view, device=device, timing=timing)
        pieces.append(o[:off[-1]].copy())
        offsets[i0 + 1:i1 + 1] = at + off[1:]
        at += int(off[-1])
        _qalib._put_times(timing, (), (), add=True, sd_batches=1)
    return (np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)), offsets
