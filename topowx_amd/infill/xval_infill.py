"""Step15, the cross-validation of the infill (``XvalInfill`` of twx/infill/xval_infill.py, driven by
scripts/step15_mpi_xval_infill.py) on the GPU: every observation of a cross-validation station but its last
``ntrain_yrs`` years is hidden, the whole infill chain runs on what is left -- the neighbour matrices, the mean /
variance estimate, the matrices under the daily eligibility, the PPCA with ``chk_perf`` -- and the model is compared with
the hidden observations.  All cross-validation stations go through each stage in ONE batched call; there is no CPU
fallback: without libtwxqa.so the calls raise.

Mechanism.  The reference processes one station at a time, so every neighbour keeps its full record and its database
mean / variance, even a neighbour that is a cross-validation station itself.  Here the masked series travel as rows
APPENDED to the pool: the pool of a call is the n stations plus one row per cross-validation station with the station's
longitude and latitude and its training observations.  The targets are the appended rows; an appended row is never
eligible as a neighbour, and the station's own full row is excluded from its target's neighbours
(``twxxv_infill_matrix``).  ``twxem_mean_variance`` and ``twxpp_ppca_fit`` take the target as a row index and need no
change.  The estimates become the appended rows of ``mean`` / ``vari``; the originals are never touched, which is the
reference's set-then-restore (:139-162) without the mutation.

Every entry of the library takes host arrays: the training rows come back to the host and go up again with the pool.

Deviations, in the manner of the daily infill.  A month whose estimate or fit fails keeps NaN in that month only and the
result shows it in the item statuses (``em_status``, ``daily.status``); in the reference one exception loses the station's
whole series.  A month whose EM estimate is not finite reaches the PPCA as an empty column (``PP_EMPTY_COLUMN``).  The
default station lists (``load_default_xval_stnids``) are data files of the reference and are not shipped: ``xval_stnids``
must be given.  The returned series are float32, what step15's writer stores.
"""
import time

import numpy as np

from .. import _qalib
from ..dates import MONTH
from .infill_daily import infill_daily
from .infill_matrix import build_infill_matrices
from .infill_normals import estimate_mean_variance

__all__ = ["XvalInfill", "XvalInfillParams", "XvalInfillResult", "APPENDED_SUFFIX"]

APPENDED_SUFFIX = "~xval"          # the id of an appended row: the station's id and this


class XvalInfillParams(object):
    """The parameters of ``infill_mean_variance`` and the daily infill as step15 passes them (xval_infill.py:166-214)."""

    def __init__(self, nnr_ds, min_daily_nnghs, nnghs_nnr, max_nnr_var, chk_perf, npcs, frac_obs_initnpcs, ppca_varyexplain,
                 verbose):
        self.nnr_ds = nnr_ds
        self.min_daily_nnghs = min_daily_nnghs
        self.nnghs_nnr = nnghs_nnr
        self.max_nnr_var = max_nnr_var
        self.chk_perf = chk_perf
        self.npcs = npcs
        self.frac_obs_initnpcs = frac_obs_initnpcs
        self.ppca_varyexplain = ppca_varyexplain
        self.verbose = verbose


class XvalInfillResult(object):
    """The result of ``XvalInfill.run_all``, nx cross-validation stations.  ``stn_ids`` [nx]; ``obs_tair`` / ``infill_tair``
    [nx, ndays] float32: the hidden observation and the model on the scored days (held, and the month was fitted), NaN
    elsewhere; ``held`` [nx, ndays] bool, ``nheld`` [nx]; ``n``, ``bias``, ``mae`` [nx] of ``infill - obs`` over the scored
    days (NaN: none) and ``month_n``, ``month_bias``, ``month_mae`` [nx, 12]; ``em_status``, ``em_mean``, ``em_variance``
    [nx, 12]: the estimate from the training observations; ``daily``: the ``InfillDaily`` of the daily stage (targets: the
    appended rows)."""

    def __init__(self, stn_ids, held, nheld, score, est, daily):
        self.stn_ids = stn_ids
        self.obs_tair, self.infill_tair = score["obs_out"], score["infill_out"]
        self.held, self.nheld = held, nheld
        self.n, self.bias, self.mae = score["n"], score["bias"], score["mae"]
        self.month_n, self.month_bias, self.month_mae = score["group_n"], score["group_bias"], score["group_mae"]
        self.em_status, self.em_mean, self.em_variance = est.status, est.mean, est.variance
        self.daily = daily


class XvalInfill(object):
    """``XvalInfill`` (xval_infill.py:32-164).  ``pool``: a ``StationObsPool`` whose flagged observations are NaN, in place
    of the reference's ``stnda``; ``mean`` / ``vari`` [n, 12]: the monthly mean and variance of the station table (step14's
    result; NaN: the station is no neighbour).  The neighbour mask of the mean / variance stage is
    ``isfinite(mean[:, 0])`` (:94).  ``xval_stnids`` is required.  ``utc_offset`` [n] (the station variable step13 writes; None: none
    is handed on) goes to the reanalysis reader ``infill_params.nnr_ds`` with each station's own value.  Attributes: ``stn_ids``, ``mths``, ``stn_xval_masks``
    ([nx, ndays] bool: the held observations, one ``twxxv_holdout`` call made at first use), ``nkeep``."""

    def __init__(self, pool, var_tair, infill_params, mean, vari, xval_stnids=None, ntrain_yrs=5, device=0, utc_offset=None):
        if var_tair not in ("tmin", "tmax"):
            raise ValueError("var_tair must be 'tmin' or 'tmax'")
        if xval_stnids is None:
            raise ValueError("xval_stnids is required: the reference's default station lists are not shipped")
        ids = np.atleast_1d(np.asarray(xval_stnids)).astype(str)
        if ids.size == 0 or np.unique(ids).size != ids.size:
            raise ValueError("xval_stnids must name at least one station, each once")
        try:
            self.cols = np.array([pool.idxs[s] for s in ids], np.int32)
        except KeyError as e:
            raise KeyError("cross-validation station %s is not in the pool" % e)
        n = pool.ids.size
        self.mean, self.vari = np.asarray(mean, np.float64), np.asarray(vari, np.float64)
        if self.mean.shape != (n, 12) or self.vari.shape != (n, 12):
            raise ValueError("mean / vari must be [nstn, 12] over the stations of the pool")
        for s in ids:
            if s + APPENDED_SUFFIX in pool.idxs:
                raise ValueError("station id %s collides with the id of an appended row" % (s + APPENDED_SUFFIX))
        self.pool, self.var_tair, self.infill_params, self.device = pool, var_tair, infill_params, device
        self.stn_ids = ids
        self.mths = np.arange(1, 13)
        self.nkeep = _qalib.xval_nkeep(ntrain_yrs)                 # xval_infill.py:73
        self.ngh_stn_mask = np.isfinite(self.mean[:, 0])           # :94
        self._hold = None
        self.utc_offset = None if utc_offset is None else np.asarray(utc_offset)
        if self.utc_offset is not None and self.utc_offset.shape != (n,):
            raise ValueError("utc_offset must be [nstn] over the stations of the pool")

    def _holdout(self, timing=None):
        if self._hold is None:
            obs = np.ascontiguousarray(getattr(self.pool, self.var_tair).T[self.cols])
            tm = {}
            self._hold = _qalib.holdout(obs, np.arange(self.cols.size, dtype=np.int32), self.nkeep, device=self.device,
                                        timing=tm)
            self._hold_ms = tm["xv_holdout_kernel_ms"]
        if timing is not None:                                      # the one call's time, whoever made it first
            timing["xv_holdout_kernel_ms"] = self._hold_ms
        return self._hold

    @property
    def stn_xval_masks(self):
        return self._holdout()["held"]

    def extended_pool(self, sel=None, timing=None):
        """The pool of the batched calls for the cross-validation stations ``sel`` (rows of ``stn_ids``; None: all): ``(ext,
        app_ids, cols, never)`` -- the n stations and then one appended row per station of ``sel`` holding its training
        observations (the other variable of ``ext`` is NaN), the ids of the appended rows (the targets), the pool columns
        of the stations themselves (each target's exclusion) and the mask of the rows that are never neighbours."""
        from ..qa import StationObsPool
        pool, var = self.pool, self.var_tair
        sel = np.arange(self.stn_ids.size) if sel is None else np.asarray(sel, np.int64)
        cols = self.cols[sel]
        n, nx, nd = pool.ids.size, sel.size, pool.days.size
        ext_obs = np.concatenate([getattr(pool, var), self._holdout(timing)["train_obs"][sel].T], axis=1)
        other = np.broadcast_to(np.float32(np.nan), (nd, n + nx))
        app_ids = np.array([s + APPENDED_SUFFIX for s in self.stn_ids[sel]])
        ext = StationObsPool(np.concatenate([pool.ids, app_ids]), np.concatenate([pool.lon, pool.lon[cols]]),
                             np.concatenate([pool.lat, pool.lat[cols]]), ext_obs if var == "tmin" else other,
                             ext_obs if var == "tmax" else other, pool.days)
        never = np.zeros(n + nx, bool)
        never[n:] = True
        return ext, app_ids, cols, never

    def _chain(self, sel, timing=None):
        """The chain for the cross-validation stations ``sel`` (rows of ``stn_ids``)."""
        p, pool, var = self.infill_params, self.pool, self.var_tair
        sel = np.asarray(sel, np.int64)
        t0 = time.perf_counter()
        hold = self._holdout(timing)
        t1 = time.perf_counter()
        ext, app_ids, cols, never = self.extended_pool(sel)
        held, nx = hold["held"][sel], sel.size
        t_mat, t_em, t_day = ({} if timing is not None else None for _ in range(3))
        mats = build_infill_matrices(ext, var, app_ids, np.concatenate([self.ngh_stn_mask, np.zeros(nx, bool)]), None,
                                     p.min_daily_nnghs, self.device, timing=t_mat, exclude_cols=cols, never_neighbour=never)
        t2 = time.perf_counter()
        utc = None if self.utc_offset is None else self.utc_offset[cols]
        est = estimate_mean_variance(mats, p.nnr_ds, utc, device=self.device, timing=t_em, nnghs_nnr=p.nnghs_nnr)
        t3 = time.perf_counter()
        mean = np.concatenate([self.mean, est.mean], axis=0)
        vari = np.concatenate([self.vari, est.variance], axis=0)
        daily = infill_daily(ext, var, app_ids, mean, vari, p.nnr_ds, utc, p.min_daily_nnghs, p.nnghs_nnr, p.max_nnr_var,
                             p.npcs, p.frac_obs_initnpcs, p.ppca_varyexplain, device=self.device, timing=t_day,
                             chk_perf=p.chk_perf, exclude_cols=cols, never_neighbour=never)
        t4 = time.perf_counter()
        group = (np.asarray(pool.days[MONTH], np.int64) - 1).astype(np.int8)
        full = np.ascontiguousarray(getattr(pool, var).T[cols])
        score = _qalib.xval_score(daily.infill_tair, full, held, group, device=self.device, timing=timing)
        if timing is not None:
            timing.update(matrices=t_mat, em=t_em, daily=t_day, holdout_s=t1 - t0, matrices_s=t2 - t1, em_s=t3 - t2,
                          daily_s=t4 - t3, score_s=time.perf_counter() - t4)
        return XvalInfillResult(self.stn_ids[sel], held, hold["nheld"][sel], score, est, daily)

    def run_all(self, timing=None):
        """Every cross-validation station in one batched chain: an ``XvalInfillResult``.  ``timing`` (a dict) receives the
        kernel milliseconds of the holdout and the score, the host seconds of the five stages (``holdout_s``, ``matrices_s``
        with the appended pool's assembly, ``em_s``, ``daily_s``, ``score_s``) and, under ``matrices`` / ``em`` / ``daily``, the
        dicts of the stages."""
        return self._chain(np.arange(self.stn_ids.size), timing)

    def run_xval(self, stn_id):
        """``run_xval`` (xval_infill.py:102-164) of one station: ``(obs_tair, infill_tair)`` [ndays] float32, NaN off the
        scored days; the same chain for that station alone, and the same bytes as its row of ``run_all()``."""
        i = np.nonzero(self.stn_ids == str(stn_id))[0]
        if i.size == 0:
            raise KeyError("station %s is not a cross-validation station" % stn_id)
        r = self._chain(i[:1])
        return r.obs_tair[0], r.infill_tair[0]
