"""The mean / variance estimate of the infill family's step14 (``_InfillMatrix.infill`` after the widening loop,
twx/infill/infill_normals.py:345-389, and ``infill_mean_variance``, :452-517) on the neighbour matrices of
``build_infill_matrices``: the columns are assembled on the host (``assemble_columns``, ``nnr_components``) and the
estimator -- ``norm``'s ``prelim.norm`` / ``em.norm`` / ``getparam.norm`` of twx/infill/rpy/norm_infill.R, restated as
include/twx_qa.h states it -- runs for every (target, day group) item in ONE call of libtwxqa's ``twxem_mean_variance``.
There is no CPU fallback: without the library the call raises.

Deviations.  Neither R nor ``norm`` can be run against the restatement: the iteration at which EM stops is not pinned
(DESIGN.md section 17).  ``nnr``: ``topowx_amd.NNRNghData`` (or any object with its ``batched_components``) gives the
reference's model, the reanalysis scores of every item from ONE ``twxnr_components`` call; any object with only the
reference's ``get_nngh_matrix(lon, lat, var, utc_offset=, nngh=)`` takes the per-target host route (``nnr_components``);
``nnr=None`` gives an estimate from station columns only.
``tair_mask`` is not an argument here: step15's cross-validation is ``topowx_amd.infill.XvalInfill``.
"""
import hashlib
import time

import numpy as np

from .. import _qalib
from .infill_matrix import MAX_COLS_NORM_IMPUTE, MIN_DAILY_NGHBRS, build_infill_matrices

__all__ = ["assemble_columns", "nnr_components", "estimate_mean_variance", "infill_mean_variance", "InfillEstimates",
           "EM_STATUS", "NNGH_NNR"]

NNGH_NNR = 4              # infill_normals.py:36

EM_STATUS = {_qalib.EM_OK: "ok", _qalib.EM_NUMERIC: "a sweep pivot is <= 0 or not finite",
             _qalib.EM_MAXITS: "maxits reached", _qalib.EM_NO_MATRIX: "no neighbour matrix",
             _qalib.EM_EMPTY_COLUMN: "a column without a finite value", _qalib.EM_ROW_CAP: "more rows than TWXEM_MAX_ROWS"}


def nnr_components(nnr_tair, max_var=0.99):
    """The principal-component scores of the reanalysis columns that reach the estimator (infill_normals.py:351-356):
    ``pca_svd(A, True, True)`` (twx/utils/pca.py: columns centred and scaled by their std(ddof=1), SVD, scores = A V) cut
    after the first component at which the cumulative explained variance reaches ``max_var``.  nnr_tair [n, k]; returns
    [n, ncomp].  The sign of a score column is arbitrary and does not move the estimate."""
    a = np.array(nnr_tair, np.float64)
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 1:
        raise ValueError("nnr_tair must be [ndays >= 2, ncells >= 1]")
    nrows, ncols = a.shape
    a = a - np.mean(a, axis=0)
    a = a / np.std(a, axis=0, ddof=1)
    _, s, v = np.linalg.svd(a, full_matrices=ncols > nrows)
    s = np.square(s) / (nrows - 1)
    var_explain = s / np.sum(s)
    scores = np.dot(a, v.T)
    i = int(np.nonzero(np.cumsum(var_explain) >= max_var)[0][0])
    return scores[:, :i + 1]


def assemble_columns(matrices, target, group, nnr_scores=None):
    """The columns of the matrix the estimator gets for an item (infill_normals.py:358-383): ``(cols, extra)`` with
    ``cols`` the pool columns of the station part after the target and ``extra`` [ndays_item, k] float64 (k may be 0).
    With more than ``MAX_COLS_NORM_IMPUTE`` kept station columns (the target counted) the matrix is cut to that many and
    gets no reanalysis column, unless a day is then left without any finite value: the last column is replaced by the first
    score.  Otherwise the scores are appended and the matrix cut to ``MAX_COLS_NORM_IMPUTE`` columns."""
    t, g, _ = matrices._item(target, group)
    r = matrices.ranked(t, g)
    kept = r["idx"][r["keep"] != 0].astype(np.int64)
    nrow = matrices.nrows(g)
    none = np.zeros((nrow, 0))
    if nnr_scores is not None:
        nnr_scores = np.asarray(nnr_scores, np.float64)
        if nnr_scores.ndim != 2 or nnr_scores.shape[0] != nrow:
            raise ValueError("nnr_scores must be [days of the item, ncomp]")
    if 1 + kept.size > MAX_COLS_NORM_IMPUTE:
        cols = kept[:MAX_COLS_NORM_IMPUTE - 1]
        if nnr_scores is not None and nnr_scores.shape[1] > 0:
            obs = getattr(matrices.pool, matrices.var)
            m = obs[np.ix_(matrices.day_idx(g), np.concatenate([[matrices.target_cols[t]], cols]))]
            if np.isfinite(m).sum(axis=1).min() == 0:
                return cols[:-1], nnr_scores[:, :1].copy()
        return cols, none
    if nnr_scores is None:
        return kept, none
    return kept, nnr_scores[:, :MAX_COLS_NORM_IMPUTE - 1 - kept.size].copy()


class InfillEstimates(object):
    """The result of ``estimate_mean_variance``, per item [ntarget, G]: ``mean``, ``variance``, ``iters`` (EM iterations),
    ``delta`` (the last iteration's largest change of a parameter, standardised scale), ``status`` (``EM_STATUS``), ``ncols``
    (columns of the matrix, the target's included) and ``ncomp`` (reanalysis score columns among them); ``rounds`` /
    ``batches``: kernel launches and workspace batches of the call."""
    EM_STATUS = EM_STATUS

    def __init__(self, matrices, res, ncols, ncomp):
        shape = ncols.shape
        self.target_ids, self.ngroups = matrices.target_ids, matrices.ngroups
        for k in ("mean", "variance", "iters", "delta", "status"):
            setattr(self, k, res[k].reshape(shape))
        self.ncols, self.ncomp = ncols, ncomp
        self.rounds, self.batches = res["rounds"], res["batches"]


def estimate_mean_variance(matrices, nnr=None, utc_offset=None, criterion=1e-4, maxits=1000, device=0, timing=None,
                           nnghs_nnr=NNGH_NNR, max_nnr_var=0.99, iters_per_launch=0, workspace_bytes=0):
    """Mean and variance of every item of ``matrices`` (an ``InfillMatrices``) in one GPU call.  ``nnr``: None (station
    columns only), an ``NNRNghData`` (anything with ``batched_components``: the scores of every item come from one
    ``twxnr_components`` call on the reader's day axis, which must be the pool's), or an object with only the reference's
    ``get_nngh_matrix(lon, lat, var, utc_offset=, nngh=)`` returning [ndays, nnghs_nnr] (the host route, one SVD per
    distinct matrix and month); ``utc_offset`` [ntarget] is handed to it.  Equal matrices share one extra-column set on
    the device.  ``criterion`` / ``maxits`` are ``em.norm``'s.
    An item whose matrix is not ``ok`` gets status ``no neighbour matrix``.  ``timing`` (a dict) receives the kernel
    milliseconds, launches and batches of the call and ``assemble_s`` / ``em_library_s``."""
    m = matrices
    nt, G = len(m.target_ids), m.ngroups
    t0 = time.perf_counter()
    day_idx = [m.day_idx(g) for g in range(G)]
    off, cols, sets, set_key, item_set = [0], [], [], {}, np.full(nt * G, -1, np.int32)
    ncols, ncomp = np.zeros((nt, G), np.int32), np.zeros((nt, G), np.int32)
    scores = {}
    batch = None
    if nnr is not None and hasattr(nnr, "batched_components"):
        batch = nnr.batched_components(m.pool.lon[m.target_cols], m.pool.lat[m.target_cols], m.var, utc_offset, day_idx,
                                       (max_nnr_var,), nnghs_nnr, device, timing)
    for t in range(nt):
        key = None
        if batch is not None:
            key = batch.key(t)
        elif nnr is not None:
            c = int(m.target_cols[t])
            a = np.asarray(nnr.get_nngh_matrix(m.pool.lon[c], m.pool.lat[c], m.var,
                                               utc_offset=None if utc_offset is None else utc_offset[t], nngh=nnghs_nnr),
                           np.float64)
            key = hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()
        for g in range(G):
            i = t * G + g
            if m.status[t, g] != _qalib.IF_OK:
                off.append(off[-1])
                continue
            sc = None
            if key is not None:
                if (key, g) not in scores:
                    scores[(key, g)] = batch.scores(t, g, max_nnr_var) if batch is not None else \
                        nnr_components(a[day_idx[g]], max_nnr_var)
                sc = scores[(key, g)]
            c, extra = assemble_columns(m, t, g, sc)
            cols.append(c)
            off.append(off[-1] + c.size)
            ncols[t, g], ncomp[t, g] = 1 + c.size + extra.shape[1], extra.shape[1]
            if extra.shape[1]:
                k = (key, g, extra.shape[1])
                if k not in set_key:
                    set_key[k] = len(sets)
                    sets.append((g, extra))
                item_set[i] = set_key[k]
    t1 = time.perf_counter()
    obs = m.obs_station_major if getattr(m, "obs_station_major", None) is not None else \
        np.ascontiguousarray(getattr(m.pool, m.var).T)
    res = _qalib.em_mean_variance(obs, m.group, np.repeat(m.target_cols, G), np.tile(np.arange(G, dtype=np.int32), nt),
                                  np.array(off, np.int64), np.concatenate(cols) if cols else np.zeros(0, np.int32), sets,
                                  item_set, m.status.ravel(), criterion, maxits, iters_per_launch, workspace_bytes,
                                  device=device, timing=timing)
    if timing is not None:
        timing.update(assemble_s=t1 - t0, em_library_s=time.perf_counter() - t1)
    return InfillEstimates(m, res, ncols, ncomp)


def infill_mean_variance(stn_id, pool, stn_mask, tair_var, nnr_ds=None, tair_mask=None, day_masks=None,
                         nnghs=MIN_DAILY_NGHBRS, nnghs_nnr=NNGH_NNR, device=0, utc_offset=None):
    """``infill_mean_variance`` (infill_normals.py:452-517) of one target, routed through the batched calls: ``(mean,
    variance)`` as two floats for ``day_masks=None`` (every day), else as two arrays over the boolean masks [ndays] of
    ``day_masks``.  ``pool``: a ``StationObsPool`` in place of the reference's ``stn_da``; ``utc_offset``: the target's (the reference reads it from
    the station table), needed with a reanalysis reader.  ``tair_mask`` is step15's
    cross-validation masking and raises ``NotImplementedError``: use ``topowx_amd.infill.XvalInfill``."""
    if tair_mask is not None:
        raise NotImplementedError("tair_mask (cross-validation masking) belongs to step15 and is not implemented")
    utc = None if utc_offset is None else [utc_offset]
    if day_masks is None:
        mats = build_infill_matrices(pool, tair_var, [stn_id], stn_mask, "all", nnghs, device)
        e = estimate_mean_variance(mats, nnr_ds, utc, device=device, nnghs_nnr=nnghs_nnr)
        return float(e.mean[0, 0]), float(e.variance[0, 0])
    masks = [np.asarray(k) for k in day_masks]
    for k in masks:
        if k.shape != (pool.days.size,) or k.dtype != np.bool_:
            raise ValueError("day_masks must be boolean arrays [ndays]")
    mean, var = np.empty(len(masks)), np.empty(len(masks))
    batched = 0 < len(masks) <= _qalib.IF_MAX_GROUPS and np.sum(masks, axis=0).max() <= 1 and all(k.any() for k in masks)
    if batched:                                                     # disjoint masks: the groups of one call
        grp = np.full(pool.days.size, -1, np.int8)
        for x, k in enumerate(masks):
            grp[k] = x
        mats = build_infill_matrices(pool, tair_var, [stn_id], stn_mask, grp, nnghs, device)
        e = estimate_mean_variance(mats, nnr_ds, utc, device=device, nnghs_nnr=nnghs_nnr)
        mean[:], var[:] = e.mean[0], e.variance[0]
    else:
        for x, k in enumerate(masks):
            mats = build_infill_matrices(pool, tair_var, [stn_id], stn_mask, np.where(k, 0, -1).astype(np.int8), nnghs, device)
            e = estimate_mean_variance(mats, nnr_ds, utc, device=device, nnghs_nnr=nnghs_nnr)
            mean[x], var[x] = e.mean[0, 0], e.variance[0, 0]
    return mean, var
