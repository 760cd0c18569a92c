"""What tests/test_gpu_mosaic.py and tests/test_mosaic_host.py share: seeded mosaic images, the expected streams from
oracle/deflate_oracle.py, generated mask and tile files, and the comparison of two product files."""
import datetime as dt
import os

import numpy as np

FILL = np.int16(-32767)


def make_image(nd, Y, X, cy, cx, seed):
    """int16 [nd, Y, X]: a smooth field in 1/100 degC plus noise; a block of cells at the fill value; where the mosaic has
    them, one chunk entirely fill and one chunk constant."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Y, 0:X]
    base = 1500.0 + 900.0 * np.sin(yy / 37.0) * np.cos(xx / 53.0) - 2.5 * yy + 1.2 * xx
    img = np.empty((nd, Y, X), np.int16)
    for d in range(nd):
        img[d] = np.clip(np.rint(base + 300.0 * np.sin(d / 3.0) + rng.normal(0.0, 20.0, (Y, X))), -9000, 6000).astype(np.int16)
    img[:, Y // 3:Y // 3 + max(1, Y // 7), X // 4:X // 4 + max(1, X // 5)] = FILL
    ncy, ncx = -(-Y // cy), -(-X // cx)
    if ncy * ncx > 1:
        img[:, (ncy - 1) * cy:, (ncx - 1) * cx:] = FILL                       # the last chunk: all fill
        img[:, 0:cy, 0:cx] = 1234                                             # the first: constant
    else:
        img[:, :, :X // 3] = 1234                                             # one chunk only: a constant third of it
    return img


def padded(img, cy, cx):
    nd, Y, X = img.shape
    Yp, Xp = -(-Y // cy) * cy, -(-X // cx) * cx
    out = np.full((nd, Yp, Xp), FILL, np.int16)
    out[:, :Y, :X] = img
    return out


def oracle_streams(img_p, cy, cx):
    """The expected streams of a padded image [nd, Yp, Xp] in (day, chunk row, chunk column) order: ONE table from the summed
    histograms of the days, every (1, cy, cx) chunk deflated with it."""
    from oracle import deflate_oracle as dorc
    nd, Yp, Xp = img_p.shape
    hist = [0] * dorc.NSYM
    for d in range(nd):
        hist = [a + b for a, b in zip(hist, dorc.tile_hist(img_p[d:d + 1], cy, cx))]
    table = dorc.make_table(hist)
    return [dorc.deflate_chunk(img_p[d:d + 1, r0:r0 + cy, c0:c0 + cx], table)
            for d in range(nd) for r0 in range(0, Yp, cy) for c0 in range(0, Xp, cx)]


def oracle_deflater(cy, cx):
    return lambda img_p: oracle_streams(img_p, cy, cx)


def write_mask(path, Y, X):
    from topowx_amd import ncio
    ds = ncio.open_dataset(path, "w", "NETCDF4")
    ds.createDimension("lat", Y)
    ds.createDimension("lon", X)
    ds.createVariable("lat", "f8", ("lat",))[:] = 49.0 - np.arange(Y) / 120.0
    ds.createVariable("lon", "f8", ("lon",))[:] = -110.0 + np.arange(X) / 120.0
    ds.createVariable("mask", "i1", ("lat", "lon"))[:] = np.ones((Y, X), np.int8)
    ds.close()
    return path


def days_between(first, last):
    from topowx_amd.dates import get_days_metadata
    return get_days_metadata(dt.date(*first), dt.date(*last))


def write_tiles(fm, path_tiles, days, varname, seed, missing=(), fmt="NETCDF4", zlib=False):
    """One tile file per tile of ``fm`` (a file-level TileMosaic) but the ``missing`` ones; returns (tile names, the whole
    mosaic int16 [ndays, Y, X] with the missing tiles at the fill value)."""
    from topowx_amd import ncio
    info = fm.tinfo
    ty, tx = info.tile_size_y, info.tile_size_x
    Y, X = len(info.lats), len(info.lons)
    whole = make_image(days.size, Y, X, 50, 70, seed)
    w = ncio.TileWriter(info, path_tiles, format=fmt, zlib=zlib)
    names = []
    for name in info.tile_ids.values() if hasattr(info.tile_ids, "values") else info.tile_ids:
        r, c = info.tile_rc[name]
        if name in missing:
            whole[:, r:r + ty, c:c + tx] = FILL
            os.makedirs(os.path.join(path_tiles, name), exist_ok=True)      # the folder is there, the file is not
            names.append(name)
            continue
        z = np.zeros((12, ty, tx), np.float32)
        w.write_tile_chunk(name, varname, days, 0, 0, whole[:, r:r + ty, c:c + tx], z, z, np.zeros((ty, tx), np.int32))
        names.append(name)
    return sorted(names), whole


def assert_same_files(path_a, path_b, varname, skip_attrs=()):
    """Every variable, every attribute, chunking() and filters() of two NetCDF-4 product files, read through h5nc."""
    from topowx_amd import h5nc
    with h5nc.Dataset(path_a) as a, h5nc.Dataset(path_b) as b:
        assert sorted(a.variables) == sorted(b.variables)
        assert sorted(a.ncattrs()) == sorted(b.ncattrs())
        for k in a.ncattrs():
            if k not in skip_attrs:
                assert a.getncattr(k) == b.getncattr(k), k
        for name in a.variables:
            va, vb = a.variables[name], b.variables[name]
            assert va.shape == vb.shape and va.dtype == vb.dtype and va.dimensions == vb.dimensions, name
            assert sorted(va.ncattrs()) == sorted(vb.ncattrs()), name
            for k in va.ncattrs():
                x, y = va.getncattr(k), vb.getncattr(k)
                assert np.array_equal(np.asarray(x), np.asarray(y)), (name, k)
            assert va.chunking() == vb.chunking() and va.filters() == vb.filters(), name
            if va.shape:
                assert np.array_equal(np.asarray(va[:]), np.asarray(vb[:])), name
        return np.asarray(a.variables[varname][:])
