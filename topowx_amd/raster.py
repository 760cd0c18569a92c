"""A 2-D raster with GDAL's geo-transform: what step19 needs of ``RasterDataset`` (twx/raster/raster_dataset.py), without GDAL.

``RasterGrid(data, geo_t, ndata, band_ndata=None)`` carries ``rows``, ``cols``, ``min_x .. max_y``, ``get_coord``,
``get_row_col``, ``is_inbounds``, ``get_coord_grid_1d`` and ``read_as_array`` with the reference's arithmetic.  ``ndata`` is
the attribute callers may reassign (step19 sets it to 0 on the mask raster); ``band_ndata`` is the band's own no-data value,
which ``read_as_array`` keeps masking.  The reference's osr transformation from WGS84 to the raster's projection is an
identity that is REQUIRED here and not performed: ``lon`` / ``lat`` are the raster's own coordinates, so a projected raster
(a GeoTIFF whose ``GTModelTypeGeoKey`` is not geographic) and a rotated one are refused.

Loaders: ``from_netcdf`` for grids in the containers ``ncio`` reads, and ``from_geotiff``, a small reader in numpy + zlib.
"""
import struct
import zlib

import numpy as np

__all__ = ["RasterGrid", "from_netcdf", "from_geotiff", "open_raster"]


class RasterGrid(object):
    def __init__(self, data, geo_t, ndata, band_ndata=None):
        data = np.asarray(data)
        if data.ndim != 2:
            raise ValueError("a raster is 2-D")
        geo_t = np.array(geo_t, dtype=np.float64)
        if geo_t.shape != (6,) or not np.isfinite(geo_t).all():
            raise ValueError("geo_t must be 6 finite numbers")
        if geo_t[2] != 0.0 or geo_t[4] != 0.0:
            raise ValueError("a rotated raster is refused (geo_t[2] and geo_t[4] must be 0)")
        if not (geo_t[1] > 0.0 and geo_t[5] < 0.0):
            raise ValueError("the raster must be north-up (geo_t[1] > 0, geo_t[5] < 0)")
        self.data = data
        self.geo_t = geo_t
        self.rows, self.cols = int(data.shape[0]), int(data.shape[1])
        self.ndata = ndata
        self.band_ndata = ndata if band_ndata is None else band_ndata
        self.min_x = self.geo_t[0]
        self.max_x = self.min_x + (self.cols * self.geo_t[1])
        self.max_y = self.geo_t[3]
        self.min_y = self.max_y - (-self.rows * self.geo_t[5])

    def get_coord(self, row, col):
        """(y, x) of the centre of a cell (raster_dataset.py:135-157)."""
        x = (self.geo_t[0] + col * self.geo_t[1] + row * self.geo_t[2]) + self.geo_t[1] / 2.0
        y = (self.geo_t[3] + col * self.geo_t[4] + row * self.geo_t[5]) + self.geo_t[5] / 2.0
        return y, x

    def get_coord_grid_1d(self):
        """(y [rows] north to south, x [cols]) of the cell centres (raster_dataset.py:108-133)."""
        ulx = self.geo_t[0] + (self.geo_t[1] / 2.0)
        urx = self.get_coord(0, self.cols - 1)[1]
        uly = self.geo_t[3] + (self.geo_t[5] / 2.0)
        lly = self.get_coord(self.rows - 1, 0)[0]
        return np.linspace(uly, lly, self.rows), np.linspace(ulx, urx, self.cols)

    def is_inbounds(self, x_geo, y_geo):
        return bool(x_geo >= self.min_x and x_geo <= self.max_x and y_geo >= self.min_y and y_geo <= self.max_y)

    def get_row_col(self, lon, lat, check_bounds=True):
        """raster_dataset.py:159-202, its ``abs(int())`` kept: a point west or north of the raster is mirrored into it."""
        if check_bounds and not self.is_inbounds(lon, lat):
            raise ValueError("lat/lon outside raster bounds: " + str(lat) + "," + str(lon))
        xoff = abs(int((lon - self.geo_t[0]) / self.geo_t[1]))
        yoff = abs(int((lat - self.geo_t[3]) / self.geo_t[5]))
        return min(max(yoff, 0), self.rows - 1), min(max(xoff, 0), self.cols - 1)

    def read_as_array(self):
        """The raster with the BAND's no-data value masked (raster_dataset.py:229-242)."""
        if self.band_ndata is None:
            return np.ma.masked_array(self.data)
        return np.ma.masked_equal(self.data, self.band_ndata)


def from_netcdf(path, varname=None):
    """A grid variable [lat, lon] of a netCDF file as ``ncio`` reads it: 1-D ``lon`` ascending and ``lat`` descending cell
    centres, evenly spaced; the no-data value is the variable's ``_FillValue`` / ``missing_value``."""
    from . import ncio
    ds = ncio.open_dataset(path, "r")
    try:
        names = [n for n, v in ds.variables.items() if len(getattr(v, "dimensions", ())) == 2]
        if varname is None:
            if len(names) != 1:
                raise ValueError("%s: name the variable (2-D variables: %s)" % (path, ", ".join(names)))
            varname = names[0]
        v = ds.variables[varname]
        ydim, xdim = v.dimensions
        lat = np.asarray(ds.variables[ydim][:], np.float64)
        lon = np.asarray(ds.variables[xdim][:], np.float64)
        a = v[:]
        ndata = None
        for att in ("_FillValue", "missing_value"):
            if att in v.ncattrs():
                ndata = np.asarray(v.getncattr(att)).ravel()[0].item()
                break
        data = np.ma.filled(a, ndata) if np.ma.isMaskedArray(a) and ndata is not None else np.asarray(a)
    finally:
        ds.close()
    if lat.size < 2 or lon.size < 2:
        raise ValueError("%s: the grid must be at least 2 x 2" % path)
    dx, dy = (lon[-1] - lon[0]) / (lon.size - 1), (lat[-1] - lat[0]) / (lat.size - 1)
    if not (dx > 0 and dy < 0):
        raise ValueError("%s: lon must ascend and lat descend (a north-up grid)" % path)
    if np.abs(np.diff(lon) - dx).max() > 1e-6 * dx or np.abs(np.diff(lat) - dy).max() > 1e-6 * -dy:
        raise ValueError("%s: the grid is not evenly spaced" % path)
    return RasterGrid(data, (lon[0] - dx / 2.0, dx, 0.0, lat[0] - dy / 2.0, 0.0, dy), ndata)


# ---- a small GeoTIFF reader ---------------------------------------------------------------------------------------------
_TYPES = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d", 16: "Q"}
_SAMPLES = {(1, 8): "u1", (2, 16): "i2", (1, 16): "u2", (2, 32): "i4", (3, 32): "f4", (3, 64): "f8"}
(_T_WIDTH, _T_LENGTH, _T_BITS, _T_COMPRESSION, _T_STRIP_OFF, _T_SPP, _T_ROWS_PER_STRIP, _T_STRIP_BYTES, _T_PLANAR,
 _T_PREDICTOR, _T_TILE_W, _T_TILE_L, _T_TILE_OFF, _T_TILE_BYTES, _T_SAMPLE_FORMAT, _T_PIXEL_SCALE, _T_TIEPOINT,
 _T_TRANSFORMATION, _T_GEOKEYS, _T_GDAL_NODATA) = (256, 257, 258, 259, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 339,
                                                  33550, 33922, 34264, 34735, 42113)


def _tiff_tags(buf):
    if buf[:2] == b"II":
        bo = "<"
    elif buf[:2] == b"MM":
        bo = ">"
    else:
        raise ValueError("not a TIFF file (byte-order mark %r)" % buf[:2])
    magic, off = struct.unpack(bo + "HI", buf[2:8])
    if magic == 43:
        raise NotImplementedError("BigTIFF (magic 43) is not supported")
    if magic != 42:
        raise ValueError("not a TIFF file (magic %d)" % magic)
    (n,) = struct.unpack(bo + "H", buf[off:off + 2])
    tags = {}
    for k in range(n):
        tag, typ, cnt, val = struct.unpack(bo + "HHI4s", buf[off + 2 + 12 * k:off + 14 + 12 * k])
        if typ not in _TYPES:
            continue
        code = _TYPES[typ]
        size = struct.calcsize(bo + code) * cnt
        raw = val[:size] if size <= 4 else buf[struct.unpack(bo + "I", val)[0]:struct.unpack(bo + "I", val)[0] + size]
        if len(raw) != size:
            raise ValueError("TIFF tag %d points outside the file" % tag)
        if typ == 2:
            tags[tag] = raw.split(b"\0")[0].decode("ascii", "replace")
        else:
            tags[tag] = struct.unpack(bo + code * cnt, raw)
    return bo, tags


def from_geotiff(path):
    """A one-band GeoTIFF as a ``RasterGrid``.  Reads classic TIFF of either byte order, strips or tiles, compression none
    (1) or deflate (8 / 32946), predictor 1, samples u8 / i16 / u16 / i32 / f32 / f64, the georeference from
    ``ModelPixelScale`` + ``ModelTiepoint`` or ``ModelTransformation``, and ``GDAL_NODATA``.  Anything else is a
    ``NotImplementedError`` that names the tag and its value."""
    with open(path, "rb") as fh:
        buf = fh.read()
    bo, t = _tiff_tags(buf)

    def one(tag, default=None):
        v = t.get(tag)
        return default if v is None else v[0]

    def refuse(name, tag, value):
        raise NotImplementedError("%s: %s (tag %d) = %r is not supported" % (path, name, tag, value))

    cols, rows = one(_T_WIDTH), one(_T_LENGTH)
    if cols is None or rows is None:
        raise ValueError("%s: no ImageWidth / ImageLength" % path)
    if one(_T_SPP, 1) != 1:
        refuse("SamplesPerPixel", _T_SPP, one(_T_SPP))
    if one(_T_PLANAR, 1) != 1:
        refuse("PlanarConfiguration", _T_PLANAR, one(_T_PLANAR))
    comp = one(_T_COMPRESSION, 1)
    if comp not in (1, 8, 32946):
        refuse("Compression", _T_COMPRESSION, comp)
    if one(_T_PREDICTOR, 1) != 1:
        refuse("Predictor", _T_PREDICTOR, one(_T_PREDICTOR))
    fmt = (one(_T_SAMPLE_FORMAT, 1), one(_T_BITS, 1))
    if fmt not in _SAMPLES:
        refuse("SampleFormat / BitsPerSample", _T_SAMPLE_FORMAT, fmt)
    dt = np.dtype(bo + _SAMPLES[fmt])

    def block(off, nbytes, shape):
        raw = buf[off:off + nbytes]
        if len(raw) != nbytes:
            raise ValueError("%s: a strip or tile lies outside the file" % path)
        if comp != 1:
            raw = zlib.decompress(raw)
        need = shape[0] * shape[1] * dt.itemsize
        if len(raw) < need:
            raise ValueError("%s: a strip or tile is shorter than its shape" % path)
        return np.frombuffer(raw, dt, shape[0] * shape[1]).reshape(shape)

    data = np.empty((rows, cols), dt.newbyteorder("="))
    if _T_TILE_OFF in t:
        tw, tl = one(_T_TILE_W), one(_T_TILE_L)
        across = (cols + tw - 1) // tw
        for k, (off, nb) in enumerate(zip(t[_T_TILE_OFF], t[_T_TILE_BYTES])):
            r0, c0 = (k // across) * tl, (k % across) * tw
            if r0 >= rows:
                break
            tile = block(off, nb, (tl, tw))
            data[r0:r0 + tl, c0:c0 + tw] = tile[:rows - r0, :cols - c0]
    elif _T_STRIP_OFF in t:
        rps = min(one(_T_ROWS_PER_STRIP, rows), rows)
        for k, (off, nb) in enumerate(zip(t[_T_STRIP_OFF], t[_T_STRIP_BYTES])):
            r0 = k * rps
            n = min(rps, rows - r0)
            data[r0:r0 + n] = block(off, nb, (n, cols))
    else:
        raise ValueError("%s: neither strips nor tiles" % path)

    keys = t.get(_T_GEOKEYS)
    if keys is not None:
        for k in range(keys[3]):
            kid, loc, _, val = keys[4 + 4 * k:8 + 4 * k]
            if kid == 1024 and loc == 0 and val != 2:
                refuse("GTModelTypeGeoKey", _T_GEOKEYS, val)          # 2: geographic.  A projected raster is refused
    if _T_TRANSFORMATION in t:
        m = t[_T_TRANSFORMATION]
        if m[1] != 0.0 or m[4] != 0.0:
            refuse("ModelTransformation (rotated)", _T_TRANSFORMATION, tuple(m[:8]))
        geo_t = (m[3], m[0], 0.0, m[7], 0.0, m[5])
    elif _T_PIXEL_SCALE in t and _T_TIEPOINT in t:
        sx, sy = t[_T_PIXEL_SCALE][:2]
        i, j, _, x, y = t[_T_TIEPOINT][:5]
        geo_t = (x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy)
    else:
        raise NotImplementedError("%s: no ModelPixelScale + ModelTiepoint and no ModelTransformation tag" % path)
    ndata = None
    if _T_GDAL_NODATA in t:
        ndata = float(t[_T_GDAL_NODATA].strip())
    return RasterGrid(data, geo_t, ndata)


def open_raster(path, varname=None):
    """``from_geotiff`` for ``.tif`` / ``.tiff``, ``from_netcdf`` otherwise."""
    return from_geotiff(path) if str(path).lower().endswith((".tif", ".tiff")) else from_netcdf(path, varname)
