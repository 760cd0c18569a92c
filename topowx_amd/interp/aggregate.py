"""Mosaicking and monthly / annual aggregation of the tile product.

Counterparts of ``twx/interp/tiling.py``: ``TileMosaic`` (:553-971), ``_TairAggregate`` (:1080-1166) and
``write_ds_mthly`` (:1169-1219, scripts/step27_create_monthly.py), at two levels: on arrays (tile stores in memory)
and on files with the reference's signatures (``TileMosaic(fpath_mask, ...).create_dly_ann_mosaics(tiles, varname,
path_in, path_out, start_yr, end_yr, ds_version_str, chunk_cache_size)``, ``create_normals_mosaic(tiles, varname,
path_in, fpath_out, ds_version_str)``, ``write_ds_mthly(ds_dly, fpath_out, varname, yr, ds_version_str)``; the
containers are ``topowx_amd.ncio``).  The arithmetic between the files -- the means over
(year, month) groups, the rounding and the int16 packing -- runs in libtwxhip (``twx_aggregate``, ``twx_pack_i16``).
"""
import os

import numpy as np

from .. import _lib
from ..dates import MONTH, YEAR, get_mth_metadata

__all__ = ["TairAggregate", "TileMosaic", "mthly_from_daily", "write_ds_mthly", "write_ds_mthly_gpu"]


class TairAggregate(object):
    """``_TairAggregate`` (tiling.py:1080-1166): first axis of every input is time."""

    def __init__(self, days, device=0):
        self.days = days
        u_yrs, u_mths = np.unique(days[YEAR]), np.unique(days[MONTH])
        self.u_yrs = u_yrs
        yr_mths = get_mth_metadata(int(u_yrs[0]), int(u_yrs[-1]))
        # tiling.py:1110-1111 keeps every year between the first and the last; the day groups only exist
        # for years that occur (tiling.py:1101), so the two agree only for a gap-free day axis
        if u_yrs.size != int(u_yrs[-1]) - int(u_yrs[0]) + 1:
            raise ValueError("day axis skips whole years")
        self.yr_mths = yr_mths[np.isin(yr_mths[MONTH], u_mths)]
        self._ctx = _lib.Context(device)
        self._ctx.set_days(days)
        self._ctx_mth = None
        self.nyr, self.nmth = self._ctx.aggregate_dims()

    def close(self):
        for c in (self._ctx, self._ctx_mth):
            if c is not None:
                c.close()
        self._ctx = self._ctx_mth = None

    @staticmethod
    def _dense(tair):
        """masked / plain array -> contiguous int16 / f4 / f8 with NaN at masked cells."""
        if np.ma.isMaskedArray(tair):
            a = np.ma.getdata(tair)
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            return np.where(np.ma.getmaskarray(tair), np.nan, a)
        a = np.asarray(tair)
        if a.dtype not in (np.int16, np.float32, np.float64):
            a = a.astype(np.float64)
        return a

    def daily_to_mthly(self, tair):
        out = self._ctx.aggregate(self._dense(tair), mthly=True)["mthly"]
        return np.ma.masked_invalid(out)

    def daily_to_ann(self, tair):
        out = self._ctx.aggregate(self._dense(tair), mthly=False, ann=True)["ann"]
        return np.ma.masked_invalid(out)

    def mthly_to_ann(self, tair_mthly):
        """Per year the mean of its monthly values (tiling.py:1151-1166): the same group-mean kernel on
        the month axis, one group per year."""
        if self._ctx_mth is None:
            self._ctx_mth = _lib.Context(self._ctx.device)
            self._ctx_mth.set_days({MONTH: np.ones(self.yr_mths.size, np.int32), YEAR: self.yr_mths[YEAR]})
        a = self._dense(tair_mthly)
        if a.dtype == np.int16:
            a = a.astype(np.float64)
        out = self._ctx_mth.aggregate(a, mthly=True)["mthly"]
        return np.ma.masked_invalid(out)

    def daily_i16_to_mthly_i16(self, daily_raw):
        """write_ds_mthly (tiling.py:1169-1219) on the raw 'i2' product: unpack (scale 0.01, fill
        -32767), group means, ``np.ma.round(., 2)``, pack with the same scale -> int16 [nyr*nmth, ...]."""
        daily_raw = np.ascontiguousarray(daily_raw)
        if daily_raw.dtype != np.int16:
            raise TypeError("daily_i16_to_mthly_i16 takes the raw int16 product")
        return self._ctx.aggregate(daily_raw, mthly=False, mthly_i16=True)["mthly_i16"]


def mthly_from_daily(daily_raw, days, device=0):
    """One-call form of write_ds_mthly's arithmetic for one year (or more) of the daily mosaic."""
    agg = TairAggregate(days, device=device)
    try:
        return agg.daily_i16_to_mthly_i16(daily_raw)
    finally:
        agg.close()


def write_ds_mthly(ds_dly, fpath_out, varname, yr, ds_version_str, format=None, device=0):
    """``write_ds_mthly`` (tiling.py:1169-1219, step27): the monthly file of one year's daily mosaic ``ds_dly`` (an open
    ``ncio.open_dataset`` / ``h5nc.Dataset``).  The daily variable is read in bands of its chunk rows, unpacked as
    netCDF4-python unpacks it, averaged per (year, month), rounded to 2 decimals and packed with the variable's scale
    on the GPU (``twx_aggregate``: bit-exact against the executed reference slice, tests/test_gpu_agg.py)."""
    from .. import ncio
    ds_out = ncio.create_ds_mthly(ds_dly, fpath_out, yr, varname, ds_version_str, format=format)
    try:
        days = ncio.days_of(ds_dly)
        var = ds_dly.variables[varname]
        chk = var.chunking()
        nrow, ncol = var.shape[1], var.shape[2]
        step = max(int(chk[1]) if chk != "contiguous" else nrow, 1)
        # bands of whole chunk rows, a few hundred MB of int16 at a time
        step *= max(1, (256 << 20) // max(1, 2 * var.shape[0] * ncol * step))
        agg = TairAggregate(days, device=device)
        try:
            out = np.empty((agg.nyr * agg.nmth, nrow, ncol), np.int16)
            for r in range(0, nrow, step):
                out[:, r:r + step, :] = agg.daily_i16_to_mthly_i16(np.ascontiguousarray(var[:, r:r + step, :], np.int16))
        finally:
            agg.close()
        if out.shape[0] != 12:
            raise ValueError("write_ds_mthly takes ONE year of daily data (tiling.py:1176-1178)")
        ds_out.variables[varname][:] = out
        ds_out.sync()
    finally:
        ds_out.close()
    return fpath_out


def write_ds_mthly_gpu(ds_dly, fpath_out, varname, yr, ds_version_str, format=None, device=0, timings=None):
    """``write_ds_mthly`` with the monthly file's chunks deflated on the device (step27 ``--deflate gpu``): the daily variable
    is read through libhdf5 in bands of its chunk rows and averaged on the GPU exactly as ``write_ds_mthly`` does; the twelve
    layers are then placed in a device mosaic, deflated there and appended with ``write_chunk_raw``.  Same file content."""
    import time
    from .. import _qalib, ncio
    fmt = format or ncio.default_format()
    if fmt != "NETCDF4":
        raise ValueError("deflate='gpu' appends HDF5 chunks: the monthly file must be NETCDF4, a %s file has no chunks "
                         "(use deflate='host')" % fmt)
    t = dict(year=int(yr), read_s=0.0, place_s=0.0, deflate_s=0.0, write_s=0.0)
    t0 = time.perf_counter()
    ds_out = ncio.create_ds_mthly(ds_dly, fpath_out, yr, varname, ds_version_str, format=fmt)
    try:
        days = ncio.days_of(ds_dly)
        var = ds_dly.variables[varname]
        chk = var.chunking()
        nrow, ncol = var.shape[1], var.shape[2]
        step = max(int(chk[1]) if chk != "contiguous" else nrow, 1)
        step *= max(1, (256 << 20) // max(1, 2 * var.shape[0] * ncol * step))
        _, cy, cx = ncio._mosaic_chunks(nrow, ncol)
        agg = TairAggregate(days, device=device)
        try:
            if agg.nyr * agg.nmth != 12:
                raise ValueError("write_ds_mthly takes ONE year of daily data (tiling.py:1176-1178)")
            with _qalib.Mosaic(12, nrow, ncol, cy, cx, device=device) as mo:
                mo.clear(12)
                for r in range(0, nrow, step):
                    ta = time.perf_counter()
                    band = np.ascontiguousarray(var[:, r:r + step, :], np.int16)
                    tb = time.perf_counter()
                    mo.place(agg.daily_i16_to_mthly_i16(band), r, 0)
                    t["read_s"] += tb - ta
                    t["place_s"] += time.perf_counter() - tb
                ta = time.perf_counter()
                streams = mo.deflate(12)
                tb = time.perf_counter()
                vm = ds_out.variables[varname]
                for (d, r0, c0), s in zip(mo.chunk_origins(12), streams):
                    vm.write_chunk_raw((d, r0, c0), s)
                t["deflate_s"] = tb - ta
                t.update(mo.timing())
        finally:
            agg.close()
        ta = time.perf_counter()
        ds_out.sync()
    finally:
        ds_out.close()
    t["write_s"] = time.perf_counter() - tb
    t["total_s"] = time.perf_counter() - t0
    if timings is not None:
        timings.append(t)
    return fpath_out


class TileMosaic(object):
    """Assemble tile results into mosaics (tiling.py:553-971).  The mosaic spans the tile rows / columns between the
    first and the last tile given (tiling.py:570-596); tiles that are missing stay at the fill value (:772-776).
    ``TileMosaic(tile_grid_info)`` works on ``step25.TileStore`` objects in memory; the reference's
    ``TileMosaic(fpath_mask, tile_size_y, tile_size_x, chk_size_y, chk_size_x)`` (tiling.py:557-565) reads the tile
    layout from the mask file and serves the file-level methods."""

    def __init__(self, tile_grid_info, tile_size_y=None, tile_size_x=None, chk_size_y=None, chk_size_x=None, device=0):
        if isinstance(tile_grid_info, (str, os.PathLike)):
            from .. import ncio
            from .tiling import Tiler
            ds_mask = ncio.open_dataset(os.fspath(tile_grid_info))
            try:
                self.atiler = Tiler(ds_mask, [], tile_size_y, tile_size_x, chk_size_y, chk_size_x, None)
            finally:
                ds_mask.close()
            tile_grid_info = self.atiler.build_tile_grid_info()
            self.lon, self.lat = self.atiler.lons, self.atiler.lats
        self.tinfo = tile_grid_info
        self.device = device

    # ---- file level (tiling.py:567-780, :782-971) -------------------------------------------------------------------
    def _mosaic_grid(self, tiles):
        """Tile names of the bounding tile rectangle, its first row / column in the grid, lon / lat of the mosaic."""
        tcols = [int(t[1:3]) for t in tiles]
        trows = [int(t[4:]) for t in tiles]
        tcols = list(range(min(tcols), max(tcols) + 1))
        trows = list(range(min(trows), max(trows) + 1))
        ty, tx = self.tinfo.tile_size_y, self.tinfo.tile_size_x
        rc = [self.tinfo.tile_rc[n] for n in ("h%02dv%02d" % (c, r) for c in tcols for r in trows) if n in self.tinfo.tile_rc]
        if not rc:
            raise ValueError("none of the tiles exists in the grid")
        min_row, min_col = min(r for r, _ in rc), min(c for _, c in rc)
        max_row, max_col = max(r for r, _ in rc), max(c for _, c in rc)
        lon = np.asarray(self.tinfo.lons)[min_col:max_col + tx]
        lat = np.asarray(self.tinfo.lats)[min_row:max_row + ty]
        return tcols, trows, lon, lat

    @staticmethod
    def _tile_path(path_in, name, varname):
        return os.path.join(path_in, name, "%s_%s.nc" % (name, varname))

    def create_dly_ann_mosaics(self, tiles, varname, path_in, path_out, start_yr, end_yr, ds_version_str,
                               chunk_cache_size=None, format=None, deflate="host", path_out_mthly=None, batch_days=None,
                               deflater=None, timings=None):
        """``create_dly_ann_mosaics`` (tiling.py:567-780): one ``<varname>_<year>.nc`` per year of ``start_yr..end_yr``
        under ``path_out`` holding the raw int16 daily values of every tile file found under ``path_in`` (a missing
        tile stays at the fill value).  Returns the paths.

        ``deflate="host"`` (the default): the values go through libhdf5, which deflates every chunk on the calling core.
        ``deflate="gpu"``: a year is assembled in device memory, deflated there into the chunk bytes and appended with
        ``write_chunk_raw`` (``_dly_ann_mosaics_gpu``); the files hold the same values, attributes and filters.
        ``path_out_mthly``: also ``<path_out_mthly>/<varname>_<year>.nc``, step27's monthly file of every year."""
        from .. import ncio
        if deflate == "gpu":
            return self._dly_ann_mosaics_gpu(tiles, varname, path_in, path_out, start_yr, end_yr, ds_version_str, chunk_cache_size,
                                             format, path_out_mthly, batch_days, deflater, timings)
        if deflate != "host":
            raise ValueError("deflate must be 'host' or 'gpu', not %r" % (deflate,))
        if path_out_mthly is not None:
            paths = self.create_dly_ann_mosaics(tiles, varname, path_in, path_out, start_yr, end_yr, ds_version_str,
                                                chunk_cache_size, format)
            os.makedirs(path_out_mthly, exist_ok=True)
            for p in paths:
                yr = int(os.path.basename(p)[len(varname) + 1:-3])
                with ncio.open_dataset(p) as ds_dly:
                    write_ds_mthly(ds_dly, os.path.join(path_out_mthly, os.path.basename(p)), varname, yr, ds_version_str,
                                   format=format, device=self.device)
            return paths
        tcols, trows, lon, lat = self._mosaic_grid(tiles)
        ty, tx = self.tinfo.tile_size_y, self.tinfo.tile_size_x
        names = [("h%02dv%02d" % (c, r), i, j) for i, c in enumerate(tcols) for j, r in enumerate(trows)]
        first = next((n for n, _, _ in names if os.path.exists(self._tile_path(path_in, n, varname))), None)
        if first is None:
            raise IOError("no tile file of %s under %s" % (varname, path_in))
        ds_tile = ncio.open_dataset(self._tile_path(path_in, first, varname))
        days_all = ncio.days_of(ds_tile)
        ds_tile.close()
        keep = np.nonzero((days_all[YEAR] >= start_yr) & (days_all[YEAR] <= end_yr))[0]
        yrs = np.unique(days_all[YEAR][keep])
        yr_rows = [keep[days_all[YEAR][keep] == yr] for yr in yrs]
        os.makedirs(path_out, exist_ok=True)
        paths = [os.path.join(path_out, "%s_%d.nc" % (varname, yr)) for yr in yrs]
        yr_ds = [ncio.create_dly_mosaic_ds(p, varname, days_all[rows], lon, lat, ds_version_str, format=format)
                 for p, rows in zip(paths, yr_rows)]
        try:
            for name, i, j in names:
                fp = self._tile_path(path_in, name, varname)
                if not os.path.exists(fp):
                    continue                               # "Tile does not exist. Values for tile will be fill values."
                ds_tile = ncio.open_dataset(fp, rdcc_nbytes=chunk_cache_size)
                try:
                    v = ds_tile.variables[varname]
                    for ds, rows in zip(yr_ds, yr_rows):   # a year's days are contiguous on a gap-free axis
                        ds.variables[varname][:, j * ty:(j + 1) * ty, i * tx:(i + 1) * tx] = v[rows[0]:rows[-1] + 1, :, :]
                finally:
                    ds_tile.close()
        finally:
            for ds in yr_ds:
                ds.close()
        return paths

    # ---- the same files with their chunks deflated on the device -----------------------------------------------------
    MAX_READERS = 16                                        # threads that pread tile chunks (ghcn.MAX_READERS is the precedent)

    @staticmethod
    def _tile_pieces(ds_tile, fp, varname, d0, nd, pool):
        """The days ``d0 .. d0 + nd - 1`` of a tile file's daily variable as ``[(row, column, int16 [nd, h, w])]``.

        A tile variable is int16 ``(ndays, ty, tx)`` in uncompressed chunks ``(ndays, cy, cx)``: the days of a chunk are ONE
        contiguous run of the file, read with ``pread`` on ``pool`` -- one piece per chunk, placed on its own.  Every other
        layout (the classic container, a deflated or shuffled variable as ``driver --deflate`` writes it -- libhdf5 inflates
        it on this core: slow --, chunks that do not divide the tile or do not span the day axis) goes through the ordinary
        slice read and is one piece."""
        v = ds_tile.variables[varname]
        ndays, ty, tx = v.shape
        chk = v.chunking() if hasattr(v, "chunk_info") else "contiguous"
        flt = v.filters() if hasattr(v, "filters") else {}
        raw = (chk != "contiguous" and int(chk[0]) == ndays and ty % int(chk[1]) == 0 and tx % int(chk[2]) == 0 and
               not flt.get("zlib") and not flt.get("shuffle") and np.dtype(v.dtype) == np.dtype("<i2"))
        info = None
        if raw:
            try:
                info = v.chunk_info()
            except IOError:
                info = None
            if info is not None and (len(info) != (ty // int(chk[1])) * (tx // int(chk[2])) or any(m for _, _, m in info.values())):
                info = None                                 # chunks never written, or written past a filter: the slice read
        if info is None:
            return [(0, 0, np.ascontiguousarray(v[d0:d0 + nd, :, :], np.int16))]
        cy, cx = int(chk[1]), int(chk[2])
        fd = os.open(fp, os.O_RDONLY)
        try:
            def read(item):
                (_, r0, c0), (addr, size, _) = item
                if size != ndays * cy * cx * 2:
                    raise IOError("%s: chunk (%d, %d) of %s holds %d bytes, not %d" % (fp, r0, c0, varname, size, ndays * cy * cx * 2))
                buf = np.empty((nd, cy, cx), np.int16)
                mv, got, want, pos = memoryview(buf).cast("B"), 0, nd * cy * cx * 2, addr + d0 * cy * cx * 2
                while got < want:
                    n = os.preadv(fd, [mv[got:]], pos + got)
                    if n <= 0:
                        raise IOError("%s: short read of chunk (%d, %d) of %s" % (fp, r0, c0, varname))
                    got += n
                return r0, c0, buf
            return list(pool.map(read, info.items()))
        finally:
            os.close(fd)

    def _dly_ann_mosaics_gpu(self, tiles, varname, path_in, path_out, start_yr, end_yr, ds_version_str, chunk_cache_size, format,
                             path_out_mthly, batch_days, deflater, timings):
        """``create_dly_ann_mosaics(..., deflate="gpu")``.  Per year: the file is created exactly as on the host route
        (``create_dly_mosaic_ds``, ``zlib=True``); the year -- or, where it does not fit the device or ``batch_days`` is
        given, a run of its days -- is cleared to the fill value in device memory, every tile found is placed, the image is
        deflated there (one Huffman code per run) and every ``(1, cy, cx)`` chunk is appended with ``write_chunk_raw``.  With
        ``path_out_mthly`` the twelve monthly means are formed from the resident year and their chunks deflated on the device
        too (a year done in several runs takes ``write_ds_mthly`` on the finished daily file instead).

        ``deflater`` (tests): a callable ``image [nd, Yp, Xp] -> list of streams`` used IN PLACE of the device object, so that
        the file layer runs on a machine without a GPU; the image is then assembled in host memory.
        ``timings`` (a list): one dict per year is appended -- seconds of read, place (upload + placement, host side),
        deflate (kernels + download), write, monthly, the device's kernel times by group, bytes in and out."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from .. import _qalib, ncio
        fmt = format or ncio.default_format()
        if fmt != "NETCDF4":
            raise ValueError("deflate='gpu' appends HDF5 chunks: the mosaics must be NETCDF4, a %s file has no chunks "
                             "(use deflate='host')" % fmt)
        if batch_days is not None and int(batch_days) < 1:
            raise ValueError("batch_days must be at least 1")
        tcols, trows, lon, lat = self._mosaic_grid(tiles)
        ty, tx = self.tinfo.tile_size_y, self.tinfo.tile_size_x
        names = [("h%02dv%02d" % (c, r), i, j) for i, c in enumerate(tcols) for j, r in enumerate(trows)]
        found = [(n, i, j) for n, i, j in names if os.path.exists(self._tile_path(path_in, n, varname))]
        if not found:
            raise IOError("no tile file of %s under %s" % (varname, path_in))
        with ncio.open_dataset(self._tile_path(path_in, found[0][0], varname)) as ds_tile:
            days_all = ncio.days_of(ds_tile)
        keep = np.nonzero((days_all[YEAR] >= start_yr) & (days_all[YEAR] <= end_yr))[0]
        yrs = np.unique(days_all[YEAR][keep])
        yr_rows = [keep[days_all[YEAR][keep] == yr] for yr in yrs]
        os.makedirs(path_out, exist_ok=True)
        if path_out_mthly is not None:
            os.makedirs(path_out_mthly, exist_ok=True)
        Y, X = int(np.size(lat)), int(np.size(lon))
        _, cy, cx = ncio._mosaic_chunks(Y, X)
        longest = max(r.size for r in yr_rows)
        want = min(longest, int(batch_days)) if batch_days is not None else longest
        mo = None
        if deflater is None:
            fit = _qalib.mosaic_max_days(Y, X, cy, cx, _qalib.device_free_bytes(self.device), want)
            if fit < 1:
                raise _qalib.QaError("not even one day of a %d x %d mosaic fits the device" % (Y, X))
            mo = _qalib.Mosaic(fit, Y, X, cy, cx, device=self.device)
            want, Yp, Xp = fit, mo.Yp, mo.Xp
        else:
            Yp, Xp = -(-Y // cy) * cy, -(-X // cx) * cx
        origins = [(r0, c0) for r0 in range(0, Yp, cy) for c0 in range(0, Xp, cx)]
        paths = []
        pool = ThreadPoolExecutor(self.MAX_READERS)
        try:
            for yr, rows in zip(yrs, yr_rows):
                yr = int(yr)
                t = dict(year=yr, ndays=int(rows.size), read_s=0.0, place_s=0.0, deflate_s=0.0, write_s=0.0, monthly_s=0.0,
                         bytes_in=int(rows.size) * Y * X * 2, bytes_out=0, runs=0)
                t0 = time.perf_counter()
                path = os.path.join(path_out, "%s_%d.nc" % (varname, yr))
                ds = ncio.create_dly_mosaic_ds(path, varname, days_all[rows], lon, lat, ds_version_str, format=fmt)
                mthly = None
                try:
                    v = ds.variables[varname]
                    if [int(c) for c in v.chunking()] != [1, cy, cx]:
                        raise ValueError("the daily mosaic's chunks are %r, not (1, %d, %d)" % (v.chunking(), cy, cx))
                    for b0 in range(0, rows.size, want):
                        nb = min(want, rows.size - b0)
                        d0 = int(rows[0]) + b0                 # (a year's days are contiguous on a gap-free axis)
                        img = None
                        if mo is not None:
                            mo.clear(nb)
                        else:
                            img = np.full((nb, Yp, Xp), _lib.FILL_I2, np.int16)
                        for name, i, j in found:
                            fp = self._tile_path(path_in, name, varname)
                            ta = time.perf_counter()
                            with ncio.open_dataset(fp, rdcc_nbytes=chunk_cache_size) as ds_tile:
                                shp = tuple(ds_tile.variables[varname].shape)
                                if shp[1:] != (ty, tx) or shp[0] != days_all.size:
                                    raise ValueError("%s: %s is %r, the tile grid of the mask says (%d, %d, %d)"
                                                     % (fp, varname, shp, days_all.size, ty, tx))
                                pieces = self._tile_pieces(ds_tile, fp, varname, d0, nb, pool)
                            tb = time.perf_counter()
                            for r0, c0, a in pieces:
                                if mo is not None:
                                    mo.place(a, j * ty + r0, i * tx + c0)
                                else:
                                    img[:, j * ty + r0:j * ty + r0 + a.shape[1], i * tx + c0:i * tx + c0 + a.shape[2]] = a
                            t["read_s"] += tb - ta
                            t["place_s"] += time.perf_counter() - tb
                        ta = time.perf_counter()
                        streams = mo.deflate(nb) if mo is not None else deflater(img)
                        if len(streams) != nb * len(origins):
                            raise ValueError("the deflater returned %d streams for %d chunks" % (len(streams), nb * len(origins)))
                        tb = time.perf_counter()
                        k = 0
                        for d in range(nb):
                            for r0, c0 in origins:
                                v.write_chunk_raw((b0 + d, r0, c0), streams[k])
                                t["bytes_out"] += len(streams[k])
                                k += 1
                        t["deflate_s"] += tb - ta
                        t["write_s"] += time.perf_counter() - tb
                        t["runs"] += 1
                    if mo is not None:
                        t.update(mo.timing())              # (the daily chunks alone; the monthly chunks' kernels: monthly_*_ms)
                    if path_out_mthly is not None and mo is not None and t["runs"] == 1:
                        ta = time.perf_counter()
                        dm = np.asarray(days_all[MONTH][rows])
                        if np.unique(dm).size != 12:
                            raise ValueError("write_ds_mthly takes ONE whole year of daily data (tiling.py:1176-1178): %d has %d months"
                                             % (yr, np.unique(dm).size))
                        mo.monthly(rows.size, dm)
                        mthly = [bytes(s) for s in mo.deflate(12, monthly=True)]
                        t["monthly_s"] += time.perf_counter() - ta
                        t.update({"monthly_" + k: v - t[k] for k, v in mo.timing().items() if k.endswith("_ms")})
                    ta = time.perf_counter()
                    ds.sync()
                finally:
                    ds.close()
                t["write_s"] += time.perf_counter() - ta
                if path_out_mthly is not None:
                    ta = time.perf_counter()
                    fp_m = os.path.join(path_out_mthly, "%s_%d.nc" % (varname, yr))
                    with ncio.open_dataset(path) as ds_dly:       # create_ds_mthly copies lon / lat / crs and the attributes from it
                        if mthly is None:
                            write_ds_mthly(ds_dly, fp_m, varname, yr, ds_version_str, format=fmt, device=self.device)
                        else:
                            ds_m = ncio.create_ds_mthly(ds_dly, fp_m, yr, varname, ds_version_str, format=fmt)
                            try:
                                vm = ds_m.variables[varname]
                                k = 0
                                for mth in range(12):
                                    for r0, c0 in origins:
                                        vm.write_chunk_raw((mth, r0, c0), mthly[k])
                                        k += 1
                                ds_m.sync()
                            finally:
                                ds_m.close()
                    t["monthly_s"] += time.perf_counter() - ta
                t["total_s"] = time.perf_counter() - t0
                if timings is not None:
                    timings.append(t)
                paths.append(path)
        finally:
            pool.shutdown()
            if mo is not None:
                mo.close()
        return paths

    def _normals_mosaic_file(self, tiles, varname, path_in, fpath_out, ds_version_str, format=None):
        """``create_normals_mosaic`` (tiling.py:782-971) on files: packed int16 normals / SE of every tile found."""
        from .. import ncio
        tcols, trows, lon, lat = self._mosaic_grid(tiles)
        ty, tx = self.tinfo.tile_size_y, self.tinfo.tile_size_x
        ds = ncio.create_normals_mosaic_ds(fpath_out, varname, lon, lat, ds_version_str, format=format)
        ctx = _lib.Context(self.device)
        try:
            for i, c in enumerate(tcols):
                for j, r in enumerate(trows):
                    fp = self._tile_path(path_in, "h%02dv%02d" % (c, r), varname)
                    if not os.path.exists(fp):
                        continue
                    t = ncio.read_tile(fp, varname)
                    for key, out in (("norm", varname + "_normal"), ("se", varname + "_se")):
                        a = t[key]
                        p = ctx.pack_i16(np.where(a == _lib.FILL_F4, 0.0, a.astype(np.float64)))   # :948-957
                        p[a == _lib.FILL_F4] = _lib.FILL_I2
                        ds.variables[out][:, j * ty:(j + 1) * ty, i * tx:(i + 1) * tx] = p
        finally:
            ctx.close()
            ds.close()
        return fpath_out

    def _extent(self, tiles):
        tcols = [int(t[1:3]) for t in tiles]
        trows = [int(t[4:]) for t in tiles]
        ty, tx = self.tinfo.tile_size_y, self.tinfo.tile_size_x
        c0, c1, r0, r1 = min(tcols), max(tcols), min(trows), max(trows)
        return r0, c0, (r1 - r0 + 1) * ty, (c1 - c0 + 1) * tx

    def _place(self, tiles, stores, key, fill, dtype, conv=None):
        r0, c0, ny, nx = self._extent(tiles)
        ty, tx = self.tinfo.tile_size_y, self.tinfo.tile_size_x
        out = None
        for t in tiles:
            if t not in stores:
                continue                                  # "Tile does not exist. Values ... fill values."
            a = stores[t].a[key]
            if conv is not None:
                a = conv(a)
            if out is None:
                out = np.full(a.shape[:-2] + (ny, nx), fill, dtype)
            i, j = (int(t[4:]) - r0) * ty, (int(t[1:3]) - c0) * tx
            out[..., i:i + ty, j:j + tx] = a
        return out

    def create_dly_mosaic(self, tiles, varname, stores):
        """Daily int16 mosaic [ndays, Y, X] (create_dly_ann_mosaics, tiling.py:567-780; the per-year
        split is a slice of the time axis)."""
        return self._place(tiles, stores, "daily_" + varname, _lib.FILL_I2, np.int16)

    def create_normals_mosaic(self, tiles, varname, stores, fpath_out=None, ds_version_str=None, format=None):
        """Monthly normals and kriging standard errors as packed int16 [12, Y, X]
        (tiling.py:948-957: ``np.ma.round(x.astype(float), 2) / SCALE_FACTOR`` cast to int16).  With the reference's
        argument list ``(tiles, varname, path_in, fpath_out, ds_version_str)`` the mosaic is read from / written to
        files (tiling.py:782-971)."""
        if isinstance(stores, (str, os.PathLike)):
            return self._normals_mosaic_file(tiles, varname, os.fspath(stores), fpath_out, ds_version_str, format)
        ctx = _lib.Context(self.device)
        try:
            def conv(a):
                p = ctx.pack_i16(np.where(a == _lib.FILL_F4, 0.0, a.astype(np.float64)))
                p[a == _lib.FILL_F4] = _lib.FILL_I2
                return p
            return (self._place(tiles, stores, "norm_" + varname, _lib.FILL_I2, np.int16, conv),
                    self._place(tiles, stores, "se_" + varname, _lib.FILL_I2, np.int16, conv))
        finally:
            ctx.close()
