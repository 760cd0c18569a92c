"""Cross-validation callers of the same kernels (twx/interp/optimize.py:84-604).

``XvalOutlier`` (optimize.py:84-207, step20's outlier screen) lives here and is NOT exported by ``topowx_amd.interp``:
import it from ``topowx_amd.interp.optimize``.  Its fits run in libtwxqa (``topowx_amd._qalib``)."""
import time
import types

import numpy as np

from .. import _lib, _qalib
from ..stationdb import BAD, ELEV, LAT, LON, MONTHLY_FIELDS, STN_ID, TDI, get_lst_varname, get_norm_varname
from .station_select import raise_for_status

__all__ = ["build_nstn_bandwidths", "XvalTairOverall", "XvalTairAnom", "XvalTairNorm", "StationKrigParams"]


def build_nstn_bandwidths(rng_min, rng_max, pct_step):
    """optimize.py:376-405: ladder of station bandwidths (35..147 for 35, 150, 0.10)."""
    out, n = [], rng_min
    while n <= rng_max:
        out.append(n)
        n = n + np.round(pct_step * n)
    return np.array(out, dtype=np.int64)


class _XvalBase(object):
    def __init__(self, stn_da, tair_var, device=0):
        self.stn_da = stn_da
        self.var = _lib.TMAX if tair_var == "tmax" else _lib.TMIN
        self.ctx = _lib.Context(device=device)
        self.ctx.set_stations(self.var, stn_da)
        good = np.isnan(stn_da.stns[BAD])
        self.stns = stn_da.stns[good]
        self._obs_cols = np.nonzero(good)[0]
        self.idx = {s: i for i, s in enumerate(self.stns[STN_ID])}
        self.mth_masks = stn_da.mth_idx

    def _pts(self, ids):
        j = np.array([self.idx[s] for s in ids])
        st = self.stns[j]
        lst = np.column_stack([st[get_lst_varname(m)] for m in range(1, 13)])
        return j, self.ctx.make_pts(st[LON], st[LAT], st[ELEV], st[TDI], lst)

    def close(self):
        self.ctx.close()


class XvalTairOverall(_XvalBase):
    """Leave-one-out interpolation of normals + daily values (optimize.py:548-604):
    StationSelect(rm_zero_dist_stns=True) and stns_rm = the station's own id."""

    def run_interp(self, stn_id):
        d, n, s = self.run_interp_many([stn_id])
        return d[0], n[0], s[0]

    def run_interp_many(self, stn_ids, daily=True, raise_on_error=True):
        """Batched form.  ``raise_on_error=False`` is the step24 worker's behaviour (step24:52-62): a station that
        cannot be interpolated keeps NaN outputs and its TWX_CELL_* code is returned as a fourth array."""
        j, pts = self._pts(stn_ids)
        d, norms, se, st = self.ctx.interp_points(self.var, pts, excl=j, rm_zero_dist=True, daily=daily)
        if not raise_on_error:
            return d, norms, se, st
        for s in st:
            raise_for_status(s)
        return d, norms, se


class XvalTairAnom(_XvalBase):
    """Leave-one-out GWR anomalies over a ladder of bandwidths (optimize.py:476-545).
    Returns bias, MAE and r^2, each [n_bandwidths, 12] as the reference does (:510-545); the statistics are
    reduced on the device (``twx_gwr_xval_points``), only three numbers per (bandwidth, month) come back."""

    def run_xval(self, stn_id, a_nnghs):
        bias, mae, r2 = self.run_xval_many([stn_id], a_nnghs)
        return bias[0], mae[0], r2[0]

    def run_xval_many(self, stn_ids, a_nnghs, raise_on_error=True):
        """Batched form: arrays [n_stations, n_bandwidths, 12].  ``raise_on_error=False`` is the step23 worker's
        behaviour (step23:56-66): a station for which any (bandwidth, month) fails is reported in a fourth
        boolean array instead of raising."""
        a_nnghs = np.asarray(a_nnghs, np.int32)
        j, pt = self._pts(stn_ids)
        ns, nb = len(stn_ids), a_nnghs.size
        # one GPU point per (station, bandwidth, month)
        pts = np.repeat(pt, nb * 12)
        mth = np.tile(np.arange(1, 13, dtype=np.int32), ns * nb)
        nn = np.tile(np.repeat(a_nnghs, 12), ns)
        own = np.repeat(j.astype(np.int32), nb * 12)
        norm = np.column_stack([self.stns[j][get_norm_varname(m)] for m in range(1, 13)])      # [ns, 12]
        pn = np.repeat(norm, nb, axis=0).reshape(-1)                                           # (station, bw, month)
        bias, mae, r2, _, st = self.ctx.gwr_xval_points(self.var, pts, pn, mth, nn, own, own, rm_zero_dist=True)
        ok = (st.reshape(ns, nb * 12) == 0).all(axis=1)
        if raise_on_error:
            for q in st:
                raise_for_status(q)
        out = tuple(a.reshape(ns, nb, 12) for a in (bias, mae, r2))
        return out if raise_on_error else out + (ok,)


class XvalTairNorm(_XvalBase):
    """Leave-one-out xval of the normals over a ladder of bandwidths with variogram fitting
    (optimize.py:209-266, step21).  Returns err[12, n_bandwidths] = interpolated - observed."""

    def run_xval(self, stn_id, abw_nngh):
        return self.run_xval_many([stn_id], abw_nngh)[0]

    def run_xval_many(self, stn_ids, abw_nngh, raise_on_error=True):
        """Batched form: err[n_stations, 12, n_bandwidths].  ``raise_on_error=False`` (the step21 worker,
        step21:55-62) also returns ok[n_stations]: False where any (bandwidth, month) could not be solved."""
        abw = np.asarray(abw_nngh, np.int32)
        j, pt = self._pts(stn_ids)
        ns, nb = len(stn_ids), abw.size
        # one GPU point per (station, bandwidth, month)
        pts = np.repeat(pt, nb * 12)
        mth = np.tile(np.arange(1, 13, dtype=np.int32), ns * nb)
        nn = np.tile(np.repeat(abw, 12), ns)
        excl = np.repeat(j.astype(np.int32), nb * 12)
        # variogram fit + kriging with the fitted model per (station, bandwidth, month): ONE call (KrigTairAll.krigall's shape,
        # interp_tair.py:722-769): one station selection and one set of pair distances serve both stages
        mean, _, _, _, st = self.ctx.krigall_points(self.var, pts, mth, nnghs=nn, excl=excl, rm_zero_dist=True)
        if raise_on_error:
            for q in st:
                raise_for_status(q)
        obs = np.column_stack([self.stns[j][get_norm_varname(m)] for m in range(1, 13)])      # [ns, 12]
        interp = mean.reshape(ns, nb, 12)
        err = np.transpose(interp - obs[:, None, :], (0, 2, 1))                                 # [ns, 12, nb]
        if raise_on_error:
            return err
        ok = (st == 0).reshape(ns, nb * 12).all(axis=1)
        return err, ok


class StationKrigParams(_XvalBase):
    """Per-station variogram parameters for every month (optimize.py:408-474, step22).  As in the
    reference the station stays inside its own neighbourhood (rm_zero_dist_stns=False, no stns_rm)."""

    def get_krig_params(self, stn_id):
        nug, psill, rng = self.get_krig_params_many([stn_id])
        return nug[0], psill[0], rng[0]

    def get_krig_params_many(self, stn_ids, raise_on_error=True):
        """Batched form: (nug, psill, rng), each [n_stations, 12].  ``raise_on_error=False`` (the step22 worker,
        step22:52-62: a station whose fit fails gets the f8 fill value for all twelve months) also returns
        ok[n_stations]."""
        j, pt = self._pts(stn_ids)
        pts = np.repeat(pt, 12)
        mth = np.tile(np.arange(1, 13, dtype=np.int32), len(stn_ids))
        vario, _, st = self.ctx.fit_vario_points(self.var, pts, mth)
        if raise_on_error:
            for q in st:
                raise_for_status(q)
        v = vario.reshape(len(stn_ids), 12, 3)
        if raise_on_error:
            return v[:, :, 0], v[:, :, 1], v[:, :, 2]
        return v[:, :, 0], v[:, :, 1], v[:, :, 2], (st == 0).reshape(len(stn_ids), 12).all(axis=1)


def _mean_skipna(a):
    """pandas ``DataFrame.mean(axis=1)`` of a [n, 12] block: NaN skipped, NaN where a row has no value."""
    ok = ~np.isnan(a)
    cnt = ok.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, a, 0.0).sum(axis=1) / np.where(cnt > 0, cnt, np.nan)


def outlier_ids(errs, stn_ids, zscore_threshold=6):
    """``find_xval_outliers``'s rule (optimize.py:195-202) on errs [13, n] (target-major, as the reference's
    ``xval_errs``): per target, z = |err - mean| / std with pandas' semantics (NaN skipped, ``ddof=1``); a station is an
    outlier if any of its 13 z-scores exceeds ``zscore_threshold``.  Returns the ids in input order."""
    e = np.asarray(errs, np.float64)
    ids = np.asarray(stn_ids)
    if e.ndim != 2 or e.shape[1] != ids.size:
        raise ValueError("errs must be [n_targets, n_stations] with one column per id")
    ok = ~np.isnan(e)
    cnt = ok.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ok, e, 0.0).sum(axis=1) / cnt                           # nanops.nanmean
        d = np.where(ok, e - mean[:, None], 0.0)
        std = np.sqrt((d * d).sum(axis=1) / (cnt - 1))                          # nanops.nanvar, ddof=1
        std = np.where(cnt > 1, std, np.nan)
        z = np.abs(e - mean[:, None]) / std[:, None]
    return ids[(z > zscore_threshold).any(axis=0)]


class XvalOutlier(object):
    """Leave-one-out GWR of every station's 12 monthly and annual normals (norm ~ lst + elev + lon + lat,
    optimize.py:84-207): stations whose error is ``zscore_threshold`` standard deviations from the mean error are
    outliers (step20:84-97).

    Neighbours come from ``twx_knn`` on the good stations (``StationSelect(stn_mask=isnan(bad),
    rm_zero_dist_stns=True)`` with ``stns_rm`` = the left-out id); the 13 weighted least-squares fits per station run
    in libtwxqa.  Deviation: a fit whose system has no Cholesky factorisation (a predictor constant over the
    neighbours, fewer than 5 usable rows) gives NaN and status 4 where statsmodels' ``pinv`` returns a minimum-norm
    prediction."""

    def __init__(self, stn_da, device=0):
        self.stn_da = stn_da
        self.device = device
        stns = stn_da.stns
        self.var = _lib.TMIN                   # the pool's slot in the context, whichever variable the database holds
        self.good = np.isnan(stns[BAD]) if BAD in stns.dtype.names else np.ones(stns.size, bool)
        # pool position of every station of the table (-1: bad, not in the pool -- nothing to exclude)
        self._pool_pos = np.full(stns.size, -1, np.int32)
        self._pool_pos[self.good] = np.arange(int(self.good.sum()), dtype=np.int32)
        lst = np.column_stack([stns[get_lst_varname(m)] for m in range(1, 13)]).astype(np.float64)
        norm = np.column_stack([stns[get_norm_varname(m)] for m in range(1, 13)]).astype(np.float64)
        # annual means of the monthly LST and normals (optimize.py:108-109)
        lst13 = np.column_stack([lst, _mean_skipna(lst)])
        norm13 = np.column_stack([norm, _mean_skipna(norm)])
        self._pt = np.ascontiguousarray(np.column_stack([stns[LON], stns[LAT], stns[ELEV], lst13, norm13]), np.float64)
        g = self.good
        self._pool = (stns[LON][g], stns[LAT][g], stns[ELEV][g], np.ascontiguousarray(lst13[g].T),
                      np.ascontiguousarray(norm13[g].T))
        self.ctx = _lib.Context(device=device)
        self.ctx.set_stations(self.var, types.SimpleNamespace(stns=self._selection_table(stns), var=None),
                              with_obs=False)
        self.last_timing = {}

    @staticmethod
    def _selection_table(stns):
        """A copy of the table with every field ``_lib.station_columns`` reads: a step20-stage database has no
        optim_nnghs* / vario_* columns yet (steps 21 and 22 add them); missing ones are NaN, which selection ignores."""
        need = [STN_ID, LON, LAT, ELEV, TDI, BAD] + [namer(m) for _, namer in MONTHLY_FIELDS for m in range(1, 13)]
        dt = [(STN_ID, stns.dtype[STN_ID])] + [(f, np.float64) for f in need[1:]]
        out = np.empty(stns.size, dt)
        for f in need:
            out[f] = stns[f] if f in stns.dtype.names else np.nan
        return out

    def run_xval_stn(self, stn_id, bw_nngh=100):
        """errs[13]: prediction - observation of the 12 monthly normals and the annual one (optimize.py:113-153)."""
        return self.run_xval_many([stn_id], bw_nngh)[0]

    def run_xval_many(self, stn_ids, bw_nngh=100, raise_on_error=True):
        """Batched form: errs[n, 13].  Too few good stations raises IndexError (station_select.py:164); with
        ``raise_on_error=False`` it is reported instead, as status[n, 13] (TWX_CELL_* numbers: 0 ok, 1 too few
        stations, 4 singular system -- NaN error, never raised)."""
        t0 = time.perf_counter()
        ids = np.asarray(stn_ids)
        if ids.ndim != 1:
            ids = ids.reshape(-1)
        k = int(bw_nngh)
        if not 1 <= k <= _qalib.MAX_K:
            raise ValueError("bw_nngh must be in 1..%d" % _qalib.MAX_K)
        if ids.size == 0:
            e, st = np.empty((0, _qalib.NTARGET)), np.empty((0, _qalib.NTARGET), np.int32)
            return e if raise_on_error else (e, st)
        rows = np.array([self.stn_da.stn_idxs[s] for s in ids], np.int64)
        pt = self._pt[rows]
        t1 = time.perf_counter()
        idx, _, wgt, kst = self.ctx.knn(self.var, pt[:, 0], pt[:, 1], k, excl=self._pool_pos[rows], rm_zero_dist=True)
        t2 = time.perf_counter()
        tm = {}
        err, st = _qalib.outlier_wls(*self._pool, pt, idx, wgt, kst, device=self.device, timing=tm)
        t3 = time.perf_counter()
        self.last_timing = dict(host_prep_s=t1 - t0, knn_s=t2 - t1, wls_s=t3 - t2, wls_kernel_ms=tm["kernel_ms"])
        if raise_on_error:
            if np.any(kst == _qalib.STATUS_FEW_STATIONS):
                raise_for_status(_qalib.STATUS_FEW_STATIONS)
            return err
        return err, st

    def find_xval_outliers(self, stn_ids=None, bw_nngh=100, zscore_threshold=6):
        """Ids (input order) of the stations whose leave-one-out error of any target is more than
        ``zscore_threshold`` standard deviations from that target's mean error (optimize.py:155-207).
        ``stn_ids=None``: every station of the database, bad ones included (optimize.py:189-190)."""
        if stn_ids is None:
            stn_ids = self.stn_da.stn_ids
        stn_ids = np.asarray(stn_ids)
        errs = self.run_xval_many(stn_ids, bw_nngh)
        return outlier_ids(errs.T, stn_ids, zscore_threshold)

    def close(self):
        self.ctx.close()
