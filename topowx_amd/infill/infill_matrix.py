"""The neighbour matrices of the infill family (``scripts/step14_mpi_infill_stn_normals.py``, step15, step16) on the GPU:
what ``_InfillMatrix.__init__`` (twx/infill/infill_normals.py:52-237), the widening loop of ``_InfillMatrix.infill``
(:324-343) and ``_shrink_matrix`` (:391-420) do for one target station, variable and day mask, done for every target
and day group in ONE call of libtwxqa's ``twxif_infill_matrix``.  There is no CPU fallback: without the library the
call raises.

``build_infill_matrices`` returns the ranked neighbour lists and the ``keep`` marks; ``InfillMatrices.matrix`` gathers
the observation matrix of an item on the host (target first, then the kept stations in rank order, at most
``MAX_COLS_NORM_IMPUTE`` columns).  ``InfillMatrix`` is a facade with the reference's attribute names for one target.

The estimate of mean and variance from the matrices (``infill_mu_sigma`` / ``em.norm``, the PCA of the reanalysis columns)
is ``topowx_amd.infill.infill_normals``; the reanalysis reader is ``topowx_amd.NNRNghData``.  Out of scope: ``build_por_mask`` and
``InfillMatrixPPCA``; the reference's ``tair_mask`` is ``topowx_amd.infill.XvalInfill`` (step15), which hands the masked
series in as rows appended to the pool (``exclude_cols`` / ``never_neighbour`` below).
"""
import time

import numpy as np

from .. import _qalib
from ..dates import MONTH, YMD

__all__ = ["build_infill_matrices", "InfillMatrices", "InfillMatrix", "item_thresholds", "ITEM_STATUS", "MAX_DISTANCE",
           "MIN_POR_OVERLAP", "MIN_DAILY_NGHBRS", "MAX_COLS_NORM_IMPUTE"]

# infill_normals.py:31-37
MAX_DISTANCE = 75.0
MIN_POR_OVERLAP = 2.0 / 3.0
MIN_DAILY_NGHBRS = 3
MAX_COLS_NORM_IMPUTE = 31

ITEM_STATUS = {_qalib.IF_OK: "ok", _qalib.IF_NUMERIC: "a d1 denominator is 0",
               _qalib.IF_NGH_CAP: "more stations than TWXQA_MAX_RADIUS_NGH",
               _qalib.IF_NO_TARGET_OBS: "the target has no finite day in the item",
               _qalib.IF_UNSATISFIED: "unsatisfied: no eligible station left"}


def _groups(days, day_groups):
    if day_groups is None:                                          # step14:42: the twelve calendar months
        g = np.asarray(days[MONTH], np.int64) - 1
    elif isinstance(day_groups, str):
        if day_groups != "all":
            raise ValueError("day_groups must be None (calendar months), 'all' or an integer array [ndays]")
        g = np.zeros(days.size, np.int64)
    else:
        g = np.asarray(day_groups)
        if g.shape != (days.size,) or g.dtype.kind not in "iu":
            raise ValueError("day_groups must be an integer array [ndays]")
        g = g.astype(np.int64)
    if g.size == 0 or g.min() < -1 or g.max() >= _qalib.IF_MAX_GROUPS:
        raise ValueError("day groups must be -1 (not used) or 0 .. %d" % (_qalib.IF_MAX_GROUPS - 1))
    if g.max() < 0:
        raise ValueError("no day belongs to a group")
    return g.astype(np.int8), int(g.max()) + 1


def item_thresholds(target_obs, group, ngroups):
    """``(nthres_all [G], nthres_target_por [ntarget, G])`` as infill_normals.py:110-115 writes them:
    ``np.round(MIN_POR_OVERLAP * days of the item)`` and ``np.round(MIN_POR_OVERLAP * finite target days of the item)``.
    target_obs [ntarget, ndays]; group [ndays]."""
    used = group >= 0
    ndays_item = np.bincount(group[used].astype(np.int64), minlength=ngroups)
    nthres_all = np.round(MIN_POR_OVERLAP * ndays_item)
    fin = np.isfinite(target_obs)
    nvalid = np.stack([fin[:, group == g].sum(axis=1) for g in range(ngroups)], axis=1) if len(target_obs) else \
        np.zeros((0, ngroups), np.int64)
    nthres_por = np.round(MIN_POR_OVERLAP * nvalid)
    return nthres_all.astype(np.int32), nthres_por.astype(np.int32)


class InfillMatrices(object):
    """The result of ``build_infill_matrices``.  Per item [ntarget, G]: ``status`` (``ITEM_STATUS``), ``nnghs``,
    ``max_dist``, ``nthres_all`` [G], ``nthres_target_por``; the ranked lists as CSR columns over ``off`` [ntarget * G + 1]
    (item = target * G + group): ``idx`` (pool column), ``ioa``, ``dist``, ``nlap``, ``nlap_stn`` and ``keep`` (1: among the
    first ``nnghs`` and not dropped by the shrink).  ``rounds`` is the number of rings the call ran.
    ``obs_station_major``: the transposed copy of the observations the call made, kept for ``estimate_mean_variance``."""

    def __init__(self, pool, var, target_ids, target_cols, group, ngroups, res, nthres_all, nthres_por, min_daily_nnghs,
                 obs_station_major=None):
        self.pool, self.var = pool, var
        self.obs_station_major = obs_station_major                  # [n, ndays] float32: kept for the estimator's call
        self.target_ids, self.target_cols = target_ids, target_cols
        self.group, self.ngroups = group, ngroups
        self.min_daily_nnghs = min_daily_nnghs
        self.nthres_all, self.nthres_target_por = nthres_all, nthres_por
        for k in ("status", "nnghs", "max_dist", "off", "idx", "ioa", "dist", "nlap", "nlap_stn", "keep", "rounds"):
            setattr(self, k, res[k])
        self._tpos = {s: i for i, s in enumerate(target_ids)}

    def _item(self, target, group):
        t = self._tpos[str(target)] if not isinstance(target, (int, np.integer)) else int(target)
        if not 0 <= t < len(self.target_ids) or not 0 <= int(group) < self.ngroups:
            raise IndexError("no item (%r, %r)" % (target, group))
        return t, int(group), t * self.ngroups + int(group)

    def ranked(self, target, group):
        """The ranked list of an item: a dict of ``idx``, ``ioa``, ``dist``, ``nlap``, ``nlap_stn``, ``keep`` (views)."""
        _, _, i = self._item(target, group)
        s = slice(int(self.off[i]), int(self.off[i + 1]))
        return {k: getattr(self, k)[s] for k in ("idx", "ioa", "dist", "nlap", "nlap_stn", "keep")}

    def day_idx(self, group):
        return np.nonzero(self.group == int(group))[0]

    def nrows(self, group):
        """The number of days of a group (the rows of its items' matrices)."""
        if getattr(self, "_nrows", None) is None:
            self._nrows = np.bincount(self.group[self.group >= 0].astype(np.int64), minlength=self.ngroups)
        return int(self._nrows[int(group)])

    def columns(self, target, group, max_cols=MAX_COLS_NORM_IMPUTE):
        """The pool columns of the stations that reach the estimator: the first ``max_cols - 1`` kept ones, in rank
        order (infill_normals.py:361-364)."""
        if max_cols < 1:
            raise ValueError("max_cols counts the target's column: at least 1")
        r = self.ranked(target, group)
        return r["idx"][r["keep"] != 0][:max_cols - 1]

    def matrix(self, target, group, max_cols=MAX_COLS_NORM_IMPUTE):
        """``[ndays_item, 1 + ncols]`` float64: the target's observations of the item's days, then the kept stations in
        rank order, cut to ``max_cols`` columns in all (the reference's ``MAX_COLS_NORM_IMPUTE``; its reanalysis columns
        are not appended).  Gathered on the host."""
        t, g, _ = self._item(target, group)
        cols = np.concatenate([[self.target_cols[t]], self.columns(t, g, max_cols)]).astype(np.int64)
        obs = getattr(self.pool, self.var)
        return obs[np.ix_(self.day_idx(g), cols)].astype(np.float64)


def build_infill_matrices(pool, var, targets=None, stns_mask=None, day_groups=None, min_daily_nnghs=MIN_DAILY_NGHBRS,
                          device=0, timing=None, exclude_cols=None, never_neighbour=None):
    """The infill neighbour matrices of ``targets`` (station ids; default: every station of ``pool``, a
    ``topowx_amd.qa.StationObsPool`` whose flagged observations are NaN) for ``var`` (``"tmin"`` / ``"tmax"``), all
    targets and day groups in one GPU call.  ``stns_mask`` [n] bool: the stations that may be neighbours (default: all;
    the target itself never is).  ``day_groups``: None = the twelve calendar months (step14's ``mth_masks``), ``"all"`` =
    one group of every day (the reference's ``day_masks=None``), or an integer array [ndays] of -1 (day not used) or
    0 .. G - 1, G <= 12.  Returns an ``InfillMatrices``.  ``timing`` (a dict) receives the device time of each kernel group
    the number of rounds and the host seconds of the transposed copy, the thresholds and the library call.
    Step15 (``XvalInfill``): ``exclude_cols`` [ntarget], -1 or the pool column that is never a neighbour of that target, and
    ``never_neighbour`` [n] bool, stations that are no target's neighbour whatever ``stns_mask`` says; both default to
    nothing."""
    if var not in ("tmin", "tmax"):
        raise ValueError("var must be 'tmin' or 'tmax'")
    n = pool.ids.size
    if targets is None:
        tcols = np.arange(n, dtype=np.int32)
    else:
        try:
            tcols = np.array([pool.idxs[str(s)] for s in np.atleast_1d(np.asarray(targets))], np.int32)
        except KeyError as e:
            raise KeyError("target station %s is not in the pool" % e)
    if tcols.size == 0:
        raise ValueError("no targets")
    if stns_mask is None:
        mask = np.ones(n, bool)
    else:
        mask = np.asarray(stns_mask)
        if mask.shape != (n,) or mask.dtype != np.bool_:
            raise ValueError("stns_mask must be a boolean array over the %d stations of the pool" % n)
    if never_neighbour is not None:
        never = np.asarray(never_neighbour)
        if never.shape != (n,) or never.dtype != np.bool_:
            raise ValueError("never_neighbour must be a boolean array over the %d stations of the pool" % n)
        mask = mask & ~never
    if exclude_cols is not None:
        exclude_cols = np.asarray(exclude_cols)
        if exclude_cols.shape != tcols.shape or exclude_cols.dtype.kind not in "iu" or \
                (exclude_cols.size and (exclude_cols.min() < -1 or exclude_cols.max() >= n)):
            raise ValueError("exclude_cols must be an integer array over the targets, -1 or a pool column")
        exclude_cols = exclude_cols.astype(np.int32)
    if not isinstance(min_daily_nnghs, (int, np.integer)) or not 1 <= min_daily_nnghs <= _qalib.IF_MAX_MIN_NNGHS:
        raise ValueError("min_daily_nnghs must be an integer in 1 .. %d" % _qalib.IF_MAX_MIN_NNGHS)
    group, ng = _groups(pool.days, day_groups)
    t0 = time.perf_counter()
    obs = np.ascontiguousarray(getattr(pool, var).T)               # station-major: a wavefront walks a row
    t1 = time.perf_counter()
    nthres_all, nthres_por = item_thresholds(obs[tcols], group, ng)
    t2 = time.perf_counter()
    res = _qalib.infill_matrix(pool.lon, pool.lat, obs, pool.days[YMD], mask, tcols, group, nthres_all, nthres_por,
                               int(min_daily_nnghs), device=device, timing=timing, exclude_idx=exclude_cols)
    if timing is not None:
        timing.update(transpose_s=t1 - t0, thresholds_s=t2 - t1, library_s=time.perf_counter() - t2)
    return InfillMatrices(pool, var, pool.ids[tcols], tcols, group, ng, res, nthres_all, nthres_por, int(min_daily_nnghs),
                          obs)


class InfillMatrix(object):
    """``_InfillMatrix`` (infill_normals.py:45-237) of one target after the widening loop: the reference's attribute names
    on the ranked stations of ``build_infill_matrices`` (one target routed through the batched call).  ``imp_tair_mat``
    [ndays_item, 1 + n]: the target, then EVERY ranked station in rank order (what ``__merge`` leaves, before the trim to
    ``nnghs`` and the shrink); ``valid_imp_mask`` its finite mask; ``ngh_ioa`` / ``ngh_dists`` with the target's 1 / 0 first;
    ``max_dist``; ``nnghs_per_day``; plus ``nnghs``, ``status`` and ``trim_matrix()``, the matrix the estimator gets.
    ``day_mask``: a boolean array [ndays], None = every day."""

    def __init__(self, stn_id, pool, stns_mask, tair_var, day_mask=None, min_daily_nnghs=MIN_DAILY_NGHBRS, device=0):
        if day_mask is None:
            groups = "all"
        else:
            day_mask = np.asarray(day_mask)
            if day_mask.shape != (pool.days.size,) or day_mask.dtype != np.bool_:
                raise ValueError("day_mask must be a boolean array [ndays]")
            groups = np.where(day_mask, 0, -1).astype(np.int8)
        self.matrices = build_infill_matrices(pool, tair_var, [stn_id], stns_mask, groups, min_daily_nnghs, device)
        m = self.matrices
        r = m.ranked(0, 0)
        self.stn_id, self.tair_var = str(stn_id), tair_var
        self.day_idx = m.day_idx(0)
        self.day_mask = m.group == 0
        cols = np.concatenate([[m.target_cols[0]], r["idx"]]).astype(np.int64)
        self.imp_tair_mat = getattr(pool, tair_var)[np.ix_(self.day_idx, cols)].astype(np.float64)
        self.valid_imp_mask = np.isfinite(self.imp_tair_mat)
        self.ngh_ioa = np.concatenate([np.ones(1), r["ioa"]])
        self.ngh_dists = np.concatenate([np.zeros(1), r["dist"]])
        self.ngh_ids = pool.ids[r["idx"]]
        self.max_dist = float(m.max_dist[0, 0])
        self.nnghs_per_day = self.valid_imp_mask[:, 1:].sum(axis=1)
        self.nnghs = int(m.nnghs[0, 0])
        self.status = int(m.status[0, 0])
        self.keep = r["keep"].astype(bool)

    def trim_matrix(self, max_cols=MAX_COLS_NORM_IMPUTE):
        """The station part of what ``infill`` hands the estimator: trimmed to ``nnghs``, shrunk, cut to ``max_cols``."""
        return self.matrices.matrix(0, 0, max_cols)
