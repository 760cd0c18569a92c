"""The reanalysis reader of the infill family: ``NNRNghData`` (twx/db/reanalysis.py:308-432) on ``ncio.open_dataset``, and the
batched principal components of the columns it returns (``batched_components``: one call of libtwxqa's
``twxnr_components`` for every target and day group; include/twx_qa.h states the arithmetic).

The files are the North American subsets ``nnr_<var>_<time>.nc`` that step12's ``create_nnr_subset*`` write: one float32
variable on ``(time, level, lat, lon)`` or ``(time, lat, lon)``, a daily ``time`` axis, ``lat`` and ``lon``.  Writing them
from the raw yearly reanalysis files (step12) and the time-zone lookup that gives a station its ``utc_offset`` (step13)
are not ported.

Deviations.  The reference's ``np.argsort`` of the cell distances leaves the order of exactly equidistant cells to the
sort implementation; here the sort is stable: of equidistant cells the one of lower flat index (latitude-major, as
``meshgrid`` lays them out) comes first.  A non-finite or fill value in a returned column, or a column that is constant,
gives NaN scores or a division by zero in the reference; here ``get_nngh_matrix`` raises ``ValueError`` for a non-finite or
fill value, and the result of ``batched_components`` raises it for either when the scores of such an item are asked for
(``NnrBatch.scores``), naming the variable and the cell; an item nobody uses raises nothing, as on the host route.
"""
import os

import numpy as np

from . import _qalib, ncio
from .dates import YMD

__all__ = ["NNRNghData", "NnrBatch", "grt_circle_dist", "NNR_STATUS"]

RADIAN_CONVERSION_FACTOR = 0.017453292519943295         # util_geo.py:21
AVG_EARTH_RADIUS_KM = 6371.009                          # util_geo.py:22

NNR_STATUS = {_qalib.NR_OK: "ok", _qalib.NR_NOCONV: "the Jacobi sweeps did not converge",
              _qalib.NR_NONFINITE: "a non-finite or fill value", _qalib.NR_CONSTANT: "a column of zero variance",
              _qalib.NR_FEW_ROWS: "fewer than 2 days"}


def grt_circle_dist(lon1, lat1, lon2, lat2):
    """The haversine distance in km (util_geo.py:24-40), float64, the reference's order of operations."""
    lat1rad = lat1 * RADIAN_CONVERSION_FACTOR
    lat2rad = lat2 * RADIAN_CONVERSION_FACTOR
    lon1rad = lon1 * RADIAN_CONVERSION_FACTOR
    lon2rad = lon2 * RADIAN_CONVERSION_FACTOR
    dlat = lat1rad - lat2rad
    dlon = lon1rad - lon2rad
    angle = 2 * np.arcsin(np.sqrt((np.sin(dlat / 2)) ** 2 + np.cos(lat1rad) * np.cos(lat2rad) * (np.sin(dlon / 2)) ** 2))
    return AVG_EARTH_RADIUS_KM * angle


class NnrBatch(object):
    """The result of ``NNRNghData.batched_components``.  ``set_of`` [ntarget]: the set of each target (targets with the same
    cells and time slot share one); ``sets``: per set ``(cells, time slot)``; ``max_vars``; ``res``: the ``NrComponents`` of the
    call; ``labels``: per set the (variable, level index, cell) of its columns.  ``ncomp(t, g, max_var)``, ``scores(t, g,
    max_var)`` [days of the group, ncomp] (a view), ``var_explain(t, g)``, ``loadings(t, g)``, ``key(t)`` (hashable: what
    identifies the target's columns)."""

    def __init__(self, set_of, sets, labels, max_vars, res, grid_lons=None, grid_lats=None):
        self.set_of, self.sets, self.labels, self.max_vars, self.res = set_of, sets, labels, tuple(max_vars), res
        self.grid_lons, self.grid_lats = grid_lons, grid_lats

    def _v(self, max_var):
        for v, x in enumerate(self.max_vars):
            if x == float(max_var):
                return v
        raise KeyError("max_var %r is not one of the cuts of the call %r" % (max_var, self.max_vars))

    def key(self, t):
        return ("nnr-set",) + self.sets[int(self.set_of[t])]

    def status(self, t, g):
        return int(self.res.status[int(self.set_of[t]), g])

    def ncomp(self, t, g, max_var):
        return int(self.res.ncomp[int(self.set_of[t]), g, self._v(max_var)])

    def scores(self, t, g, max_var):
        s = int(self.set_of[t])
        st = int(self.res.status[s, g])
        if st == _qalib.NR_NOCONV:
            raise _qalib.QaError("twxnr_components: set %d, group %d: %s" % (s, g, NNR_STATUS[st]))
        if st in (_qalib.NR_NONFINITE, _qalib.NR_CONSTANT):
            name, lev, cell = self.labels[s][int(self.res.bad_col[s, g])]
            raise ValueError("reanalysis variable %s%s (level index %d) at cell (lon %g, lat %g): %s on the days of group %d"
                             % (name, self.sets[s][1], lev, self.grid_lons[cell], self.grid_lats[cell], NNR_STATUS[st], g))
        if st != _qalib.NR_OK:
            raise ValueError("the reanalysis columns of target %d, group %d have no components: %s"
                             % (t, g, NNR_STATUS.get(st, "?")))
        return self.res.scores(s, g, self.ncomp(t, g, max_var))

    def var_explain(self, t, g):
        return self.res.var_explain(int(self.set_of[t]), g)

    def loadings(self, t, g):
        return self.res.loadings(int(self.set_of[t]), g)


class _MemVar(object):
    """An array behind the few members of a netCDF variable the reader uses."""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, key):
        return self.a[key]

    def ncattrs(self):
        return []


class _MemDs(object):
    def __init__(self, variables, dimensions):
        self.variables, self.dimensions = variables, dimensions

    def close(self):
        pass


class NNRNghData(object):
    """NCEP/NCAR reanalysis data around a point (twx/db/reanalysis.py:308-432).  Attributes as the reference's: ``ds_nnr``,
    ``nnr_vars``, ``days``, ``day_mask``, ``nnr_lons``, ``nnr_lats``, ``grid_lons``, ``grid_lats``."""

    NNR_VARS = np.array(["tair", "hgt", "thick", "rhum", "uwnd", "vwnd", "slp"])
    NNR_TIMES = np.array(["24z", "18z", "12z"])
    TMIN = "tmin"
    TMAX = "tmax"
    # the reanalysis observation time nearest the local time of Tmin / Tmax, by UTC offset (reanalysis.py:320-321)
    UTC_OFFSET_TIMES = {TMIN: {-4: "12z", -5: "12z", -6: "12z", -7: "12z", -8: "12z"},
                        TMAX: {-4: "18z", -5: "18z", -6: "18z", -7: "24z", -8: "24z"}}

    def __init__(self, path_nnr_na, startend_ymd, nnr_vars=None):
        self.ds_nnr = {}
        self.nnr_vars = self.NNR_VARS if nnr_vars is None else np.asarray(nnr_vars)
        for nnr_var in self.nnr_vars:
            for nnr_time in self.NNR_TIMES:
                self.ds_nnr["".join([nnr_var, nnr_time])] = ncio.open_dataset(
                    os.path.join(path_nnr_na, "nnr_%s_%s.nc" % (nnr_var, nnr_time)))
        eg_ds = next(iter(self.ds_nnr.values()))
        self.days = ncio.days_of(eg_ds)
        self.day_mask = np.nonzero(np.logical_and(self.days[YMD] >= startend_ymd[0], self.days[YMD] <= startend_ymd[1]))[0]
        self.days = self.days[self.day_mask]
        self.nnr_lons = np.asarray(eg_ds.variables["lon"][:])
        self.nnr_lats = np.asarray(eg_ds.variables["lat"][:])
        llgrid = np.meshgrid(self.nnr_lons, self.nnr_lats)
        self.grid_lons = llgrid[0].ravel()
        self.grid_lats = llgrid[1].ravel()
        self._data = {}

    @classmethod
    def from_arrays(cls, days, lons, lats, data, nnr_vars=None):
        """A reader over arrays in memory instead of files: ``days`` (a days record array), ``lons`` / ``lats`` of the grid,
        ``data[(var, time)]``: float32 [ndays, nlevels, nlat, nlon] or [ndays, nlat, nlon]."""
        self = cls.__new__(cls)
        self.nnr_vars = cls.NNR_VARS if nnr_vars is None else np.asarray(nnr_vars)
        self.ds_nnr = {}
        for nnr_var in self.nnr_vars:
            for nnr_time in cls.NNR_TIMES:
                a = np.asarray(data[(str(nnr_var), str(nnr_time))], np.float32)
                dims = {"time": a.shape[0], "lat": a.shape[-2], "lon": a.shape[-1]}
                if a.ndim == 4:
                    dims["level"] = a.shape[1]
                if a.ndim not in (3, 4) or a.shape[0] != days.size or a.shape[-2:] != (len(lats), len(lons)):
                    raise ValueError("data[(%s, %s)] must be [ndays, (nlevels,) nlat, nlon]" % (nnr_var, nnr_time))
                self.ds_nnr["".join([str(nnr_var), str(nnr_time)])] = _MemDs({str(nnr_var): _MemVar(a)}, dims)
        self.days = days
        self.day_mask = np.arange(days.size)
        self.nnr_lons, self.nnr_lats = np.asarray(lons, np.float64), np.asarray(lats, np.float64)
        llgrid = np.meshgrid(self.nnr_lons, self.nnr_lats)
        self.grid_lons, self.grid_lats = llgrid[0].ravel(), llgrid[1].ravel()
        self._data = {}
        return self

    def close(self):
        for ds in self.ds_nnr.values():
            ds.close()
        self.ds_nnr = {}

    def nearest_cells(self, lon, lat, nngh=4):
        """The flat indices (latitude-major) of the ``nngh`` nearest cells in ascending ``grt_circle_dist``; equidistant
        cells by index."""
        dist = grt_circle_dist(lon, lat, self.grid_lons, self.grid_lats)
        return np.argsort(dist, kind="stable")[0:nngh]

    def _fills(self, v):
        marks = [float(v.getncattr(a)) for a in ("missing_value", "_FillValue") if a in v.ncattrs()]
        return marks or [float(ncio.FILL_F4)]

    def _cell_columns(self, nnr_var, nnr_time, cell):
        """float32 [days, levels] of a variable at a cell (a flat index), fill values as NaN; cached."""
        key = (nnr_var, nnr_time, int(cell))
        if key not in self._data:
            ds = self.ds_nnr["".join([nnr_var, nnr_time])]
            v = ds.variables[nnr_var]
            idx_lat, idx_lon = divmod(int(cell), self.nnr_lons.size)
            d0, d1 = (int(self.day_mask[0]), int(self.day_mask[-1]) + 1) if self.day_mask.size else (0, 0)
            if "level" in ds.dimensions:
                a = np.asarray(v[d0:d1, :, idx_lat, idx_lon], np.float32)
            else:
                a = np.asarray(v[d0:d1, idx_lat, idx_lon], np.float32)
            a = a.reshape(d1 - d0, -1).copy()
            for m in self._fills(v):
                a[a == np.float32(m)] = np.nan
            self._data[key] = a
        return self._data[key]

    def get_nngh_matrix(self, lon, lat, tair_var, utc_offset, nngh=4):
        """[ndays, P] float32: for each of the ``nngh`` nearest cells in order of distance, the variables in ``nnr_vars``
        order, each with its levels, at the time slot of ``tair_var`` and ``utc_offset`` (``KeyError`` outside -4 .. -8)."""
        cells = self.nearest_cells(lon, lat, nngh)
        nnr_time = self.UTC_OFFSET_TIMES[tair_var][utc_offset]
        parts = []
        for cell in cells:
            for nnr_var in self.nnr_vars:
                a = self._cell_columns(nnr_var, nnr_time, cell)
                if not np.isfinite(a).all():
                    raise ValueError("reanalysis variable %s%s has a non-finite or fill value at cell (lon %g, lat %g)"
                                     % (nnr_var, nnr_time, self.grid_lons[cell], self.grid_lats[cell]))
                parts.append(a)
        return np.hstack(parts)

    def batched_components(self, lons, lats, tair_var, utc_offsets, day_idx_per_group, max_vars=(0.99, 0.90), nngh=4,
                           device=0, timing=None):
        """The principal components of every target's matrix on every day group, in one library call: an ``NnrBatch``.
        ``lons`` / ``lats`` / ``utc_offsets`` [ntarget]; ``day_idx_per_group``: per group the indices of its days on
        ``self.days`` (disjoint; a group may be empty); ``max_vars``: the cuts.  The nearest cells are chosen here, in
        float64 with the reference's formula; targets with the same (cells, time slot) share one set, and only the
        columns of the cells in use are uploaded, one copy per time slot."""
        import time
        t0 = time.perf_counter()
        lons, lats = np.atleast_1d(np.asarray(lons, np.float64)), np.atleast_1d(np.asarray(lats, np.float64))
        if utc_offsets is None:
            raise KeyError("utc_offset is required with reanalysis columns (step13 writes it to the station database)")
        offs = np.atleast_1d(np.asarray(utc_offsets))
        if lons.shape != lats.shape or offs.shape != lons.shape or lons.ndim != 1:
            raise ValueError("lons / lats / utc_offsets must be [ntarget]")
        nd = self.days.size
        group = np.full(nd, -1, np.int8)
        for g, idx in enumerate(day_idx_per_group):
            idx = np.asarray(idx, np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= nd or (group[idx] != -1).any() or np.unique(idx).size != idx.size):
                raise ValueError("day_idx_per_group must hold disjoint day indices of the reader's axis")
            group[idx] = g
        ng = len(day_idx_per_group)
        set_id, sets, set_of = {}, [], np.zeros(lons.size, np.int64)
        for t in range(lons.size):
            slot = self.UTC_OFFSET_TIMES[tair_var][int(offs[t]) if float(offs[t]) == int(offs[t]) else offs[t]]
            k = (tuple(int(c) for c in self.nearest_cells(lons[t], lats[t], nngh)), str(slot))
            if k not in set_id:
                set_id[k] = len(sets)
                sets.append(k)
            set_of[t] = set_id[k]
        col_id, cols, set_off, set_col, labels = {}, [], [0], [], []
        for cells, slot in sets:
            lab = []
            for cell in cells:
                if (slot, cell) not in col_id:
                    ids = []
                    for nnr_var in self.nnr_vars:
                        a = self._cell_columns(nnr_var, slot, cell)
                        for lev in range(a.shape[1]):
                            ids.append((len(cols), str(nnr_var), lev))
                            cols.append(a[:, lev])
                    col_id[(slot, cell)] = ids
                for c, name, lev in col_id[(slot, cell)]:
                    set_col.append(c)
                    lab.append((name, lev, cell))
            set_off.append(len(set_col))
            labels.append(lab)
        cols = np.ascontiguousarray(np.stack(cols)) if cols else np.zeros((0, nd), np.float32)
        t1 = time.perf_counter()
        res = _qalib.nnr_components_batched(cols, np.array(set_off, np.int64), np.array(set_col, np.int32), group,
                                            max_vars, ngroups=ng, device=device, timing=timing)
        if timing is not None:
            timing["nr_select_s"] = timing.get("nr_select_s", 0.0) + (t1 - t0)
            timing["nr_library_s"] = timing.get("nr_library_s", 0.0) + (time.perf_counter() - t1)
            timing["nr_sets"] = len(sets)
        return NnrBatch(set_of, sets, labels, res.max_var, res, self.grid_lons, self.grid_lats)
