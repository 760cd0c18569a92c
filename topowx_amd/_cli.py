"""What the step14 / step15 / step16 command lines share: reading a file of station ids against a pool, and a step14
``--estimate`` report as the monthly mean / variance of every station of the pool, and ``--nnr-dir``: the reanalysis
reader over the database's days with the stations' ``utc_offset``."""
import zipfile

import numpy as np

__all__ = ["UnknownIds", "BadNormals", "NnrInputError", "NoUtcOffset", "BadNnrDir", "read_ids", "normals", "open_nnr",
           "NNR_DIR_HELP"]


class UnknownIds(Exception):
    pass


def read_ids(path, pool, what):
    with open(path) as fh:
        ids = [ln.strip() for ln in fh if ln.strip()]
    missing = [s for s in ids if s not in pool.idxs]
    if missing:
        raise UnknownIds("%s: %d %s ids are not in the database (first: %s)" % (path, len(missing), what, missing[0]))
    return ids


class BadNormals(Exception):
    pass


def normals(path, pool):
    """(mean, vari) [n, 12] in the pool's station order from a step14 report."""
    try:
        with np.load(path) as z:
            if not all(k in z.files for k in ("ids", "mean", "variance")):
                raise BadNormals("%s has no ids / mean / variance: write it with step14 --estimate" % path)
            ids, mean, vari = [str(s) for s in z["ids"]], np.asarray(z["mean"], np.float64), np.asarray(z["variance"], np.float64)
    except (IOError, OSError, ValueError, KeyError, zipfile.BadZipFile) as e:
        raise BadNormals("cannot read the normals %s: %s" % (path, e))
    if mean.shape != (len(ids), 12) or vari.shape != mean.shape:
        raise BadNormals("%s: mean / variance must be [%d, 12] over its ids" % (path, len(ids)))
    pos = {s: i for i, s in enumerate(ids)}
    missing = [s for s in pool.ids if str(s) not in pos]
    if missing:
        raise UnknownIds("%s: %d stations of the database have no normals (first: %s)" % (path, len(missing), missing[0]))
    order = [pos[str(s)] for s in pool.ids]
    return mean[order], vari[order]


class NnrInputError(Exception):
    """What ``--nnr-dir`` cannot work with; the command lines print it and exit with 1."""


class NoUtcOffset(NnrInputError):
    pass


class BadNnrDir(NnrInputError):
    pass


NNR_DIR_HELP = ("directory of the North American reanalysis subsets nnr_<var>_<time>.nc: the matrices get the "
                "reference's reanalysis score columns; the database must hold the station variable utc_offset")


def open_nnr(nnr_dir, db_path, pool):
    """(``NNRNghData`` over the days of the pool, utc_offset [n] in the pool's station order) for ``--nnr-dir``.
    ``NoUtcOffset`` if the database has no ``utc_offset`` (step13 writes it; i2) or a station has none; ``BadNnrDir`` if the
    subsets cannot be opened or do not cover the days of the database.  The caller closes the reader."""
    from . import ncio
    from .dates import YMD
    from .reanalysis import NNRNghData
    ds = ncio.open_dataset(db_path, "r")
    try:
        if "utc_offset" not in ds.variables:
            raise NoUtcOffset("%s has no station variable utc_offset, which --nnr-dir needs (step13 writes it)" % db_path)
        v = ds.variables["utc_offset"]
        raw = np.asarray(v[:])
        fills = [v.getncattr(a) for a in ("missing_value", "_FillValue") if a in v.ncattrs()] or [ncio.FILL_I2]
        ids = [str(s) for s in ncio._read_ids(ds.variables["station_id"])]
    finally:
        ds.close()
    if raw.shape != (len(ids),) or any((raw == f).any() for f in fills):
        raise NoUtcOffset("%s: utc_offset must hold a value for every station" % db_path)
    pos = {s: i for i, s in enumerate(ids)}
    utc = np.array([int(raw[pos[str(s)]]) for s in pool.ids], np.int16)
    ymd = pool.days[YMD]
    try:
        nnr = NNRNghData(nnr_dir, (int(ymd[0]), int(ymd[-1])))
    except (IOError, OSError, ValueError, KeyError) as e:
        raise BadNnrDir("cannot open the reanalysis subsets in %s: %s" % (nnr_dir, e))
    if nnr.days.size != pool.days.size or not np.array_equal(nnr.days[YMD], ymd):
        nnr.close()
        raise BadNnrDir("the reanalysis subsets in %s do not cover the days of the database" % nnr_dir)
    return nnr, utc
