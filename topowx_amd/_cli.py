"""What the step14 / step15 / step16 command lines share: reading a file of station ids against a pool, and a step14
``--estimate`` report as the monthly mean / variance of every station of the pool."""
import zipfile

import numpy as np

__all__ = ["UnknownIds", "BadNormals", "read_ids", "normals"]


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
