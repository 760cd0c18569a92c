"""The daily infill of step16 (``InfillMatrixPPCA.infill`` and ``infill_daily_obs``, twx/infill/infill_daily.py:329-561, with
``run_ppca`` of twx/infill/rpy/pca_infill.R:112-303) on the neighbour matrices of ``build_infill_matrices``: the columns are
assembled on the host, and the estimator -- ``pcaMethods``' ``ppca`` restated as include/twx_qa.h states it -- runs for
every (target, calendar month) item in rounds of ONE call of libtwxqa's ``twxpp_ppca_fit`` each: a round fits every item
that is still searching for its number of components.  There is no CPU fallback: without the library the call raises.

Deviations (none of them is built).  Neither R nor ``pcaMethods`` can be run: the start C0 comes from numpy's frozen
``RandomState(4324)``, not from R's ``rnorm`` stream, which moves the iteration EM stops at.  The
warning branch of ``run_ppca`` parses a ``pcaMethods`` warning text and is replaced by a stated rule: a request is never
above ``min(D - 1, TWXPP_MAX_PCS)``; the bound is tried once and accepted, flagged ``r2_not_reached`` if it misses
``max_r2cum``.  ``tair_mask`` is not an argument here (step15 is ``topowx_amd.infill.XvalInfill``).  ``nnr``:
``topowx_amd.NNRNghData`` gives the reference's model, with the scores of every item and of the ladder's 0.90 attempt
from ONE ``twxnr_components`` call; an object with only ``get_nngh_matrix`` takes the per-target host route; ``nnr=None``:
station columns only.

``chk_perf=True`` adds the reference's judgement of every fit (``_is_nonoptimal_infill``, :563-595) and its retry ladder
(:438-518): libtwxqa's ``twxck_infill_check`` judges all items of a stage in ONE call, and ``RetryLadder`` decides per item
which attempt runs next and which is kept.  ``hasVarChgPt`` (R's ``changepoint``) is restated as include/twx_qa.h states it,
not executed.  Two rules of ours: an attempt whose inputs equal an earlier one's is not fitted again
and takes that attempt's result; an attempt that is not fitted is non-optimal and is never kept while a fitted one exists
(the reference would raise).
"""
import hashlib
import time

import numpy as np

from .. import _qalib
from ..dates import MONTH
from .infill_matrix import MIN_DAILY_NGHBRS, build_infill_matrices
from .infill_normals import NNGH_NNR, nnr_components

__all__ = ["infill_daily", "infill_daily_obs", "InfillDaily", "PcSearch", "assemble_daily_columns", "daily_items",
           "item_matrix", "first_npcs", "add_npcs", "PP_STATUS", "MAX_NNR_VAR", "IMPOSSIBLE_HIGH", "IMPOSSIBLE_LOW",
           "RetryLadder", "MIN_NNR_VAR", "RETRY_THRESHOLDS", "NATTEMPTS"]

MAX_NNR_VAR = 0.99                 # infill_daily.py:44
MIN_NNR_VAR = 0.90                 # infill_daily.py:45: the reanalysis variance of the ladder's first retry
RETRY_THRESHOLDS = (1e-6, 1e-7)    # infill_daily.py:471: the PPCA thresholds of the second and third retry
NATTEMPTS = 4
IMPOSSIBLE_HIGH, IMPOSSIBLE_LOW = 57.7, -89.4      # infill_daily.py:584

PP_STATUS = {_qalib.PP_OK: "ok", _qalib.PP_NUMERIC: "a pivot or ss is <= 0 or not finite",
             _qalib.PP_MAXITS: "maxits reached", _qalib.PP_NO_MATRIX: "no neighbour matrix",
             _qalib.PP_EMPTY_COLUMN: "a column without a finite value", _qalib.PP_ROW_CAP: "more rows than TWXPP_MAX_ROWS",
             _qalib.PP_COL_CAP: "more columns than TWXPP_MAX_COLS", _qalib.PP_PCS_CAP: "more components than TWXPP_MAX_PCS"}
_FITTED = (_qalib.PP_OK, _qalib.PP_MAXITS)


def first_npcs(ncols, frac_obs, bound):
    """The first request of the search (pca_infill.R:163-167): ``max(2, round((D - 1) frac_obs))``, R's ``round`` (half to
    even), never above ``bound``."""
    return min(max(2, int(round(float((ncols - 1) * frac_obs)))), bound)


def add_npcs(r2cum, max_r2cum):
    """The components added after a fit that misses ``max_r2cum`` (:276-277): ``max(1, min(10, round((max_r2cum -
    R2cum[last]) / R2[last])))``.  A quotient of 10 or more (infinity included) gives 10; one below 1, negative or NaN
    gives 1."""
    r2last = r2cum[-1] - r2cum[-2] if len(r2cum) > 1 else r2cum[-1]
    with np.errstate(all="ignore"):
        q = np.float64(max_r2cum - r2cum[-1]) / np.float64(r2last)
    if q >= 10:
        return 10
    if not q >= 1:
        return 1
    return max(1, min(10, int(round(float(q)))))


class PcSearch(object):
    """``run_ppca``'s search for the number of components of ONE item as a state machine: ``request`` is the number of
    components to fit next (None: finished); ``feed(status, r2cum, payload)`` hands in the fit of that request.  After the
    end: ``npcs``, ``nfits``, ``r2_not_reached``, ``status`` and ``payload`` of the accepted fit."""

    def __init__(self, ncols, npcs=0, frac_obs=0.5, max_r2cum=0.99, max_pcs=_qalib.PP_MAX_PCS):
        self.bound = min(int(ncols) - 1, int(max_pcs))
        self.max_r2cum = max_r2cum
        self.fixed = npcs != 0
        self.request = int(npcs) if self.fixed else first_npcs(ncols, frac_obs, max(self.bound, 1))
        self.cache = {}
        self.refit = False
        self.nfits, self.npcs, self.r2_not_reached, self.status, self.payload = 0, 0, False, None, None

    def _final(self, k, status, payload, bogus=True):
        if bogus and k == 1 and self.cache and max(self.cache) > 1:        # "Removed bogus PC1" (:286-298)
            k = max(self.cache)
            status, payload = self.cache[k]
        self.npcs, self.status, self.payload, self.request = k, status, payload, None

    def feed(self, status, r2cum, payload=None):
        k = self.request
        if k is None:
            raise ValueError("the search has ended")
        self.nfits += 1
        if self.fixed:
            return self._final(k, status, payload, bogus=False)
        if status not in _FITTED or self.refit:
            return self._final(k, status, payload)
        r2 = np.asarray(r2cum, np.float64)[:k]
        if np.max(r2) >= self.max_r2cum:
            n = int(np.nonzero(r2 >= self.max_r2cum)[0][0]) + 1
            if n == k:
                return self._final(k, status, payload)
            if n in self.cache:
                return self._final(n, *self.cache[n])
            self.refit, self.request = True, n
        elif k >= self.bound:
            self.r2_not_reached = True
            self._final(k, status, payload)
        else:
            self.cache[k] = (status, payload)
            self.request = min(k + add_npcs(r2, self.max_r2cum), self.bound)


class RetryLadder(object):
    """The ``chk_perf`` block of ``InfillMatrixPPCA.infill`` (infill_daily.py:438-518) for ONE item as a state machine.
    ``inputs``: what identifies the inputs of the attempts 0 .. 3 (anything comparable; None: the attempt does not exist,
    which only attempt 1 may: ``MIN_NNR_VAR < max_nnr_var`` fails).  ``request`` is the attempt to run next (None:
    finished) and ``duplicate`` the earlier attempt with equal inputs, whose result the caller feeds again instead of
    fitting (None: fit).  ``feed(reasons, mae, fitted=True)`` hands in the check of that attempt (``reasons``: the bit mask of
    ``twxck_infill_check``; 0 = optimal).  After the end: ``kept`` (the attempt whose series is the result), ``attempts``
    (those that ran, in order), ``nonoptimal`` (the kept attempt is) and ``retry_fixed`` (a retry was optimal).

    Attempt 0 optimal: done.  Otherwise attempt 1, if it exists; while the latest attempt is non-optimal, attempts 2 and 3.
    The first optimal attempt is kept.  If none is: among the attempts whose reasons are exactly {low performance}, or among
    all of them if there is none, the one of least MAE, the first on ties (``np.argmin``); an attempt that was not fitted
    is left out of that choice while a fitted one exists."""

    def __init__(self, inputs):
        self.inputs = list(inputs)
        if len(self.inputs) != NATTEMPTS or any(self.inputs[a] is None for a in (0, 2, 3)):
            raise ValueError("inputs must describe the attempts 0 .. 3; only attempt 1 may be None")
        self.request, self.kept, self.nonoptimal, self.retry_fixed = 0, -1, False, False
        self.attempts, self.reasons, self.mae, self.fitted = [], [], [], []

    @property
    def duplicate(self):
        if self.request is None:
            return None
        for a in self.attempts:
            if self.inputs[a] == self.inputs[self.request]:
                return a
        return None

    def feed(self, reasons, mae, fitted=True):
        a = self.request
        if a is None:
            raise ValueError("the ladder has ended")
        self.attempts.append(a)
        self.reasons.append(int(reasons))
        self.mae.append(float(mae))
        self.fitted.append(bool(fitted))
        if fitted and int(reasons) == 0:
            self.kept, self.request, self.retry_fixed = a, None, a > 0
        elif a == 0:
            self.request = 1 if self.inputs[1] is not None else 2
        elif a < NATTEMPTS - 1:
            self.request = a + 1 if a > 1 else 2
        else:
            self.request = None
        if self.request is None and self.kept < 0:
            self.nonoptimal = True
            idx = [k for k in range(len(self.attempts)) if self.fitted[k]] or list(range(len(self.attempts)))
            pure = [k for k in idx if self.reasons[k] == _qalib.CK_LOW_PERF]
            idx = pure or idx
            self.kept = self.attempts[idx[int(np.argmin([self.mae[k] for k in idx]))]]


def assemble_daily_columns(matrices, target, group, mean_g, vari_g, nnr_scores=None):
    """The matrix ``infill`` hands ``ppca_tair`` for an item (infill_daily.py:373-419): ``(cols, extra, norms, stds)`` with
    ``cols`` the pool columns of the station part after the target (every kept station in rank order: no 31-column cut),
    ``extra`` [ndays_item, k] the reanalysis scores (k may be 0), and the norms / stds of all 1 + len(cols) + k columns:
    ``mean_g`` / ``sqrt(vari_g)`` [nstn] of the month for the stations, the scores' own mean and ``std(ddof=1)``."""
    t, g, _ = matrices._item(target, group)
    r = matrices.ranked(t, g)
    kept = r["idx"][r["keep"] != 0].astype(np.int64)
    allc = np.concatenate([[int(matrices.target_cols[t])], kept]).astype(np.int64)
    norms = np.asarray(mean_g, np.float64)[allc]
    with np.errstate(invalid="ignore"):
        stds = np.sqrt(np.asarray(vari_g, np.float64)[allc])
    extra = np.zeros((matrices.nrows(g), 0))
    if nnr_scores is not None:
        extra = np.array(nnr_scores, np.float64)
        if extra.ndim != 2 or extra.shape[0] != matrices.nrows(g):
            raise ValueError("nnr_scores must be [days of the item, ncomp]")
        if extra.size > 0:
            norms = np.concatenate([norms, np.mean(extra, axis=0)])
            stds = np.concatenate([stds, np.std(extra, axis=0, ddof=1)])
    return kept, extra, norms, stds


def month_mask_groups(mean, vari, never_neighbour=None):
    """The calendar months grouped by equal eligibility masks (the reference's ``stns_mask``: finite mean and variance of
    the month): a list of (mask [nstn] bool, months).  ``never_neighbour`` [nstn] bool: rows that are eligible in no month
    (step15's appended rows: their estimates must not split the months into more groups)."""
    elig = np.isfinite(mean) & np.isfinite(vari)
    if never_neighbour is not None:
        elig[np.asarray(never_neighbour, bool)] = False
    out, seen = [], {}
    for g in range(12):
        key = elig[:, g].tobytes()
        if key not in seen:
            seen[key] = len(out)
            out.append((elig[:, g].copy(), []))
        out[seen[key]][1].append(g)
    return out


def daily_items(pool, tair_var, target_ids, mean, vari, nnr=None, utc_offset=None, min_daily_nnghs=MIN_DAILY_NGHBRS,
                nnghs_nnr=NNGH_NNR, max_nnr_var=MAX_NNR_VAR, device=0, timing=None, exclude_cols=None,
                never_neighbour=None):
    """The items of ``infill_daily``, item = target * 12 + month - 1: a list of dicts of ``t`` (row of ``target_ids``),
    ``col`` (the target's pool column), ``g``, ``matrix_status``, ``max_dist``, ``cols``, ``extra``, ``norms``, ``stds``,
    ``ncomp``, ``key`` (None or what identifies the item's extra columns), ``nnr`` (None or the target's reanalysis
    matrix over every day, shared between its items: the host route) and ``nnr_batch`` (None or the ``NnrBatch`` of the call and
    the target's row in it: the batched route); and the station-major observations of the call.  One ``build_infill_matrices`` call per group of months with equal eligibility masks.
    ``exclude_cols`` / ``never_neighbour``: as ``build_infill_matrices`` takes them (step15)."""
    mean, vari = np.asarray(mean, np.float64), np.asarray(vari, np.float64)
    n = pool.ids.size
    if mean.shape != (n, 12) or vari.shape != (n, 12):
        raise ValueError("mean / vari must be [nstn, 12] over the stations of the pool")
    month = np.asarray(pool.days[MONTH], np.int64) - 1
    items, obs = {}, None
    batch = None                                                     # ONE reanalysis call for all targets and months
    for mask, months in month_mask_groups(mean, vari, never_neighbour):
        grp = np.where(np.isin(month, months), month, -1).astype(np.int8)
        if not (grp >= 0).any():
            continue
        m = build_infill_matrices(pool, tair_var, target_ids, mask, grp, min_daily_nnghs, device, timing=timing,
                                  exclude_cols=exclude_cols)
        obs = m.obs_station_major
        scores = {}
        if batch is None and nnr is not None and hasattr(nnr, "batched_components"):
            cuts = (max_nnr_var, MIN_NNR_VAR) if MIN_NNR_VAR < max_nnr_var else (max_nnr_var,)
            batch = nnr.batched_components(pool.lon[m.target_cols], pool.lat[m.target_cols], tair_var, utc_offset,
                                           [np.nonzero(month == g)[0] for g in range(12)], cuts, nnghs_nnr, device, timing)
        for t in range(len(m.target_ids)):
            key = a = None
            if batch is not None:
                key = batch.key(t)
            elif nnr is not None:
                c = int(m.target_cols[t])
                a = np.asarray(nnr.get_nngh_matrix(pool.lon[c], pool.lat[c], tair_var,
                                                   utc_offset=None if utc_offset is None else utc_offset[t],
                                                   nngh=nnghs_nnr), np.float64)
                key = hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()
            for g in months:
                if g >= m.ngroups or m.nrows(g) == 0:
                    continue
                it = dict(t=t, col=int(m.target_cols[t]), g=g, matrix_status=int(m.status[t, g]),
                          max_dist=float(m.max_dist[t, g]), cols=np.zeros(0, np.int64), extra=np.zeros((m.nrows(g), 0)),
                          norms=np.array([mean[m.target_cols[t], g]]),
                          stds=np.sqrt(np.array([vari[m.target_cols[t], g]])), ncomp=0, key=None, nnr=None, nnr_batch=None)
                if it["matrix_status"] == _qalib.IF_OK:
                    sc = None
                    if key is not None:
                        if (key, g) not in scores:
                            scores[(key, g)] = batch.scores(t, g, max_nnr_var) if batch is not None else \
                                nnr_components(a[m.day_idx(g)], max_nnr_var)
                        sc = scores[(key, g)]
                    it["cols"], it["extra"], it["norms"], it["stds"] = assemble_daily_columns(m, t, g, mean[:, g], vari[:, g], sc)
                    it["ncomp"] = it["extra"].shape[1]
                    it["key"] = (key, g) if it["ncomp"] else None
                    it["nnr"] = a if key is not None and batch is None else None
                    it["nnr_batch"] = (batch, t) if batch is not None else None
                items[(t, g)] = it
    if obs is None:
        raise ValueError("no day belongs to a calendar month")
    return [items[k] for k in sorted(items)], obs


def item_matrix(obs, group_days, item):
    """The standardised matrix of an item, [N, D] float64 with NaN = missing: what ``run_ppca`` works on after its two
    ``sweep`` calls.  ``obs`` station-major [nstn, ndays]; ``group_days``: the day indices of the item's month."""
    cols = np.concatenate([[item["col"]], item["cols"]]).astype(np.int64)
    y = obs[np.ix_(cols, group_days)].T.astype(np.float64)
    if item["extra"].shape[1]:
        y = np.hstack([y, item["extra"]])
    with np.errstate(all="ignore"):
        y = (y - item["norms"]) / item["stds"]
    y[~np.isfinite(y)] = np.nan
    return y


class InfillDaily(object):
    """The result of ``infill_daily``.  Per target [ntarget, ndays]: ``fnl_tair`` (observations, missing ones infilled),
    ``mask_infill``, ``infill_tair`` (the model everywhere); per series [ntarget]: ``mae`` / ``bias`` of the model against
    the observations (post_infill.update_daily_infill:63-66).  A month whose item was not fitted (any status but ok /
    maxits) keeps NaN in ``infill_tair`` and on its missing days in ``fnl_tair`` (``mask_infill`` is still True there) and is
    left out of ``mae`` / ``bias``, which are NaN only if no month was fitted.  Per item [ntarget, 12]: ``status`` (``PP_STATUS``; -1: the
    month has no day), ``matrix_status``, ``npcs``, ``nfits``, ``iters`` and ``rel`` of the accepted fit, ``r2_not_reached``,
    ``ncols``, ``ncomp``, and the diagnostics of ``_is_nonoptimal_infill`` that need no R, reported and not acted on:
    ``item_mae``, ``item_r2`` (squared correlation of observed against fit), ``item_impossible`` (fitted values above 57.7 or
    below -89.4).  ``calls``: library calls (rounds of the search).

    With ``chk_perf`` everything above describes the KEPT attempt of the item (``nfits`` and ``calls`` count all attempts),
    the diagnostics are acted on and ``item_mae`` / ``item_r2`` / ``item_impossible`` are the device's values
    (``twxck_infill_check``), and per item [ntarget, 12]: ``attempt`` (the kept attempt 0 .. 3; -1: no item or no check),
    ``nattempts``, ``nonoptimal`` (the kept attempt is), ``retry_fixed`` (a retry was optimal), ``cpt_stat`` / ``cpt_tau`` /
    ``cpt_pen`` of the kept attempt; per attempt [ntarget, 12, 4]: ``reasons`` (the ``CK_*`` bits of ``_qalib``; -1: the attempt
    did not run), ``attempt_mae``, ``attempt_r2``.  Without ``chk_perf`` these hold their initial values."""
    PP_STATUS = PP_STATUS

    def __init__(self, target_ids, ndays):
        nt = len(target_ids)
        self.target_ids = target_ids
        self.fnl_tair = np.full((nt, ndays), np.nan)
        self.infill_tair = np.full((nt, ndays), np.nan)
        self.mask_infill = np.zeros((nt, ndays), bool)
        self.mae, self.bias = np.full(nt, np.nan), np.full(nt, np.nan)
        for k in ("status", "matrix_status", "npcs", "nfits", "iters", "ncols", "ncomp", "item_impossible"):
            setattr(self, k, np.zeros((nt, 12), np.int32))
        self.status[:] = -1
        self.rel, self.item_mae, self.item_r2 = (np.full((nt, 12), np.nan) for _ in range(3))
        self.r2_not_reached = np.zeros((nt, 12), bool)
        self.calls = 0
        self.attempt = np.full((nt, 12), -1, np.int32)
        self.nattempts = np.zeros((nt, 12), np.int32)
        self.nonoptimal, self.retry_fixed = np.zeros((nt, 12), bool), np.zeros((nt, 12), bool)
        self.reasons = np.full((nt, 12, NATTEMPTS), -1, np.int32)
        self.attempt_mae, self.attempt_r2 = np.full((nt, 12, NATTEMPTS), np.nan), np.full((nt, 12, NATTEMPTS), np.nan)
        self.cpt_stat, self.cpt_pen = np.full((nt, 12), np.nan), np.full((nt, 12), np.nan)
        self.cpt_tau = np.zeros((nt, 12), np.int32)


def run_search(obs, group, items, npcs=0, frac_obs=0.5, max_r2cum=0.99, threshold=1e-5, maxits=1000, device=0, timing=None,
               iters_per_launch=0, workspace_bytes=0):
    """The component search of every item in rounds: each round is one ``twxpp_ppca_fit`` call for the items still
    searching.  Returns the ``PcSearch`` of every item (payload: fit [N], iters, rel, r2cum [d]) and the number of calls."""
    ncols = [1 + len(it["cols"]) + it["extra"].shape[1] for it in items]
    search = [PcSearch(ncols[i], npcs, frac_obs, max_r2cum) for i in range(len(items))]
    for i, it in enumerate(items):
        if it["matrix_status"] != _qalib.IF_OK:
            search[i].request = 1                                    # one call gives it its status; nothing is fitted
            search[i].fixed = True
    calls = 0
    while True:
        act = [i for i, s in enumerate(search) if s.request is not None]
        if not act:
            break
        sets, set_key, item_set = [], {}, np.full(len(act), -1, np.int32)
        for a, i in enumerate(act):
            it = items[i]
            if it["extra"].shape[1]:
                k = it["key"] if it["key"] is not None else ("item", i)
                if k not in set_key:
                    set_key[k] = len(sets)
                    sets.append((it["g"], it["extra"]))
                item_set[a] = set_key[k]
        off = np.concatenate([[0], np.cumsum([len(items[i]["cols"]) for i in act])]).astype(np.int64)
        cols = np.concatenate([items[i]["cols"] for i in act]).astype(np.int32)
        res = _qalib.ppca_fit(obs, group, [items[i]["col"] for i in act], [items[i]["g"] for i in act],
                              [search[i].request for i in act], off, cols,
                              np.concatenate([items[i]["norms"] for i in act]),
                              np.concatenate([items[i]["stds"] for i in act]), None, sets, item_set,
                              [items[i]["matrix_status"] for i in act], threshold, maxits, iters_per_launch,
                              workspace_bytes, device=device, timing=timing)
        calls += 1
        for a, i in enumerate(act):
            d = search[i].request
            fit = res["fit"][res["fit_off"][a]:res["fit_off"][a + 1]].copy()
            search[i].feed(int(res["status"][a]), res["r2cum"][a, :d],
                           (fit, int(res["iters"][a]), float(res["rel"][a]), res["r2cum"][a, :d].copy()))
    return search, calls


def retry_item(item, nnr_var, day_idx):
    """The item of the ladder's attempt at ``nnr_var``: the reanalysis scores cut at that variance, the station columns as
    they are.  ``day_idx``: the day indices of the item's month.  An item of the batched route (``nnr_batch``) takes the
    leading columns of the decomposition it already has; the host route runs ``nnr_components`` again."""
    if (item["nnr"] is None and item.get("nnr_batch") is None) or item["matrix_status"] != _qalib.IF_OK:
        return item
    if item.get("nnr_batch") is not None:
        batch, t = item["nnr_batch"]
        extra = np.array(batch.scores(t, item["g"], nnr_var), np.float64)
    else:
        extra = nnr_components(item["nnr"][day_idx], nnr_var)
    nst = 1 + len(item["cols"])
    it = dict(item, extra=extra, ncomp=extra.shape[1], key=(item["key"][0], item["g"], float(nnr_var)) if item["key"] else None)
    it["norms"] = np.concatenate([item["norms"][:nst], np.mean(extra, axis=0)])
    it["stds"] = np.concatenate([item["stds"][:nst], np.std(extra, axis=0, ddof=1)])
    return it


def run_ladder(obs, group, items, day_idx, first, max_nnr_var=MAX_NNR_VAR, npcs=0, frac_obs=0.5, max_r2cum=0.99,
               threshold=1e-5, maxits=1000, cpt_sig=_qalib.CK_SIG, device=0, timing=None, iters_per_launch=0,
               workspace_bytes=0):
    """The retry ladder of every item in stages: stage a is one ``run_search`` over the items that take attempt a (``first``:
    the searches of attempt 0, already run) and ONE ``infill_check`` call for them.  Returns per item its ``RetryLadder``,
    a dict attempt -> (item, ``PcSearch``, the check's values of the item), and the number of library calls of the search."""
    has1 = MIN_NNR_VAR < max_nnr_var
    alt = [retry_item(it, MIN_NNR_VAR, day_idx[it["g"]]) if has1 else None for it in items]
    thr = (threshold, threshold) + RETRY_THRESHOLDS
    ladders = [RetryLadder([(it["ncomp"], thr[0]), (alt[i]["ncomp"], thr[1]) if has1 else None, (it["ncomp"], thr[2]),
                            (it["ncomp"], thr[3])]) for i, it in enumerate(items)]
    done = [dict() for _ in items]
    calls, per_attempt = 0, [0] * NATTEMPTS
    for a in range(NATTEMPTS):
        stage = [i for i, lad in enumerate(ladders) if lad.request == a]
        if not stage:
            continue
        per_attempt[a] = len(stage)
        fitl = [i for i in stage if ladders[i].duplicate is None]
        fitted_here = set(fitl)
        its = [alt[i] if a == 1 else items[i] for i in fitl]
        if a == 0:
            found = dict(zip(fitl, first))
        elif fitl:
            srch, n = run_search(obs, group, its, npcs, frac_obs, max_r2cum, thr[a], maxits, device, timing, iters_per_launch,
                                 workspace_bytes)
            calls += n
            found = dict(zip(fitl, srch))
        if fitl:
            off = np.concatenate([[0], np.cumsum([found[i].payload[0].size for i in fitl])]).astype(np.int64)
            ck = _qalib.infill_check(off, np.concatenate([found[i].payload[0] for i in fitl]),
                                     np.concatenate([obs[items[i]["col"], day_idx[items[i]["g"]]].astype(np.float64)
                                                     for i in fitl]), None, cpt_sig, device=device, timing=timing)
            for k, i in enumerate(fitl):
                done[i][a] = (its[k], found[i], {name: ck[name][k] for name in
                                                 ("nobs", "mae", "r2", "nimpossible", "cpt_stat", "cpt_tau", "reasons",
                                                  "status", "pen")})
        for i in stage:
            if i not in fitted_here:
                done[i][a] = done[i][ladders[i].duplicate]
            it, s, c = done[i][a]
            ladders[i].feed(int(c["reasons"]), float(c["mae"]), s.status in _FITTED and int(c["status"]) != _qalib.CK_NOT_FITTED
                            and int(c["status"]) != _qalib.CK_ROW_CAP)
    if timing is not None:
        timing["attempt_items"] = per_attempt
    return ladders, done, calls


def infill_daily(pool, tair_var, target_ids, mean, vari, nnr=None, utc_offset=None, min_daily_nnghs=MIN_DAILY_NGHBRS,
                 nnghs_nnr=NNGH_NNR, max_nnr_var=MAX_NNR_VAR, npcs=0, frac_obs_initnpcs=0.5, ppca_varyexplain=0.99,
                 ppcaConThres=1e-5, maxits=1000, device=0, timing=None, iters_per_launch=0, workspace_bytes=0,
                 chk_perf=False, cpt_sig=_qalib.CK_SIG, exclude_cols=None, never_neighbour=None):
    """Step16 for ``target_ids`` (station ids of ``pool``, a ``StationObsPool`` whose flagged observations are NaN) and
    ``tair_var``, every target and calendar month in batched GPU calls.  ``mean`` / ``vari`` [nstn, 12]: the monthly mean
    and variance of every station of the pool as step14 estimates them (NaN: the station is no neighbour that month).
    ``nnr``: None, an ``NNRNghData`` (batched route) or an object with the reference's ``get_nngh_matrix``.  The other parameters are ``infill_daily_obs``'s.
    ``chk_perf``: judge every fit and refit the non-optimal ones up the reference's ladder (``RetryLadder``; ``cpt_sig``: the
    level of the variance change-point check); False, the default, stops at every item's first attempt.
    ``exclude_cols`` [ntarget] / ``never_neighbour`` [nstn]: as ``build_infill_matrices`` takes them (step15's ``XvalInfill``).
    Returns an ``InfillDaily``.  ``timing`` (a dict) receives kernel milliseconds, launches, calls and host seconds; with
    ``chk_perf`` also the check's ``ck_*`` figures, ``attempt_items`` (items per attempt), ``nonoptimal`` and ``retry_fixed``."""
    t0 = time.perf_counter()
    items, obs = daily_items(pool, tair_var, target_ids, mean, vari, nnr, utc_offset, min_daily_nnghs, nnghs_nnr,
                             max_nnr_var, device, timing, exclude_cols, never_neighbour)
    t1 = time.perf_counter()
    group = (np.asarray(pool.days[MONTH], np.int64) - 1).astype(np.int8)
    search, calls = run_search(obs, group, items, npcs, frac_obs_initnpcs, ppca_varyexplain, ppcaConThres, maxits, device,
                               timing, iters_per_launch, workspace_bytes)
    t2 = time.perf_counter()
    ids = pool.ids[[pool.idxs[str(s)] for s in np.atleast_1d(np.asarray(target_ids))]]
    out = InfillDaily(ids, pool.days.size)
    day_idx = [np.nonzero(group == g)[0] for g in range(12)]
    checks = [None] * len(items)
    if chk_perf:
        ladders, done, more = run_ladder(obs, group, items, day_idx, search, max_nnr_var, npcs, frac_obs_initnpcs,
                                         ppca_varyexplain, ppcaConThres, maxits, cpt_sig, device, timing, iters_per_launch,
                                         workspace_bytes)
        calls += more
        nfits = [sum(s.nfits for s in {id(d[1]): d[1] for d in done[i].values()}.values()) for i in range(len(items))]
        for i, (it, lad) in enumerate(zip(items, ladders)):
            t, g = it["t"], it["g"]
            out.attempt[t, g], out.nattempts[t, g] = lad.kept, len(lad.attempts)
            out.nonoptimal[t, g], out.retry_fixed[t, g] = lad.nonoptimal, lad.retry_fixed
            for a in lad.attempts:
                out.reasons[t, g, a] = done[i][a][2]["reasons"]
                out.attempt_mae[t, g, a], out.attempt_r2[t, g, a] = done[i][a][2]["mae"], done[i][a][2]["r2"]
            items[i], search[i], checks[i] = done[i][lad.kept]
            out.cpt_stat[t, g], out.cpt_tau[t, g], out.cpt_pen[t, g] = (checks[i][k] for k in ("cpt_stat", "cpt_tau", "pen"))
        t2 = time.perf_counter()
    out.calls = calls
    for i, (it, s) in enumerate(zip(items, search)):
        t, g = it["t"], it["g"]
        fit = s.payload[0]
        o = obs[it["col"], day_idx[g]].astype(np.float64)
        miss = np.isnan(o)                                           # infill_daily.py:520-522
        out.fnl_tair[t, day_idx[g]] = np.where(miss, fit, o)
        out.mask_infill[t, day_idx[g]] = miss
        out.infill_tair[t, day_idx[g]] = fit
        out.status[t, g], out.matrix_status[t, g] = s.status, it["matrix_status"]
        out.nfits[t, g], out.r2_not_reached[t, g] = s.nfits, s.r2_not_reached
        out.ncols[t, g], out.ncomp[t, g] = 1 + len(it["cols"]) + it["ncomp"], it["ncomp"]
        if s.status in _FITTED:
            out.npcs[t, g], out.iters[t, g], out.rel[t, g] = s.npcs, s.payload[1], s.payload[2]
            v = np.isfinite(o)
            with np.errstate(all="ignore"):
                out.item_mae[t, g] = np.mean(np.abs(fit[v] - o[v])) if v.any() else np.nan
                out.item_r2[t, g] = np.corrcoef(o[v], fit[v])[0, 1] ** 2 if v.sum() > 1 else np.nan
            out.item_impossible[t, g] = int(np.sum(fit > IMPOSSIBLE_HIGH) + np.sum(fit < IMPOSSIBLE_LOW))
            if chk_perf:
                out.item_mae[t, g], out.item_r2[t, g] = checks[i]["mae"], checks[i]["r2"]
                out.item_impossible[t, g] = checks[i]["nimpossible"]
        if chk_perf:
            out.nfits[t, g] = nfits[i]
    for t in range(len(ids)):                                        # post_infill.update_daily_infill:63-66
        om = ~out.mask_infill[t] & (group >= 0) & np.isfinite(out.infill_tair[t])      # a month without a fit has no part
        with np.errstate(all="ignore"):
            difs = out.infill_tair[t, om] - out.fnl_tair[t, om]
            if difs.size:
                out.mae[t], out.bias[t] = np.mean(np.abs(difs)), np.mean(difs)
    if timing is not None:
        timing.update(assemble_s=t1 - t0, search_s=t2 - t1, writeback_s=time.perf_counter() - t2, pp_items=len(items),
                      pp_fits=int(out.nfits.sum()) if chk_perf else int(sum(s.nfits for s in search)))
        if chk_perf:
            timing.update(nonoptimal=int(out.nonoptimal.sum()), retry_fixed=int(out.retry_fixed.sum()))
    return out


def infill_daily_obs(stn_id, pool, tair_var, nnr_ds, mean, vari, tair_mask=None, day_masks=None, add_bestngh=True,
                     min_daily_nnghs=MIN_DAILY_NGHBRS, nnghs_nnr=NNGH_NNR, max_nnr_var=MAX_NNR_VAR, chk_perf=False, npcs=0,
                     frac_obs_initnpcs=0.5, ppca_varyexplain=0.99, ppcaConThres=1e-5, verbose=False, device=0, utc_offset=None):
    """``infill_daily_obs`` (infill_daily.py:526-561) of one target, routed through the batched call: ``(fnl_tair,
    mask_infill, infill_tair)`` over the days of the pool.  ``pool`` stands for the reference's ``stn_da``; ``mean`` / ``vari``
    [nstn, 12] for its ``vname_mean`` / ``vname_vari`` (the twelve monthly variables); ``day_masks`` must be the twelve
    calendar-month masks in order, as step16 passes them (``None``, one matrix over every day with one mean and variance, is
    not implemented).  ``tair_mask`` raises ``NotImplementedError`` (step15 is ``topowx_amd.infill.XvalInfill``), and so does ``chk_perf=True`` here: the retry
    ladder is batched over items, call ``infill_daily(chk_perf=True)`` for it; ``add_bestngh=False`` is not supported by the
    matrix builder.  ``utc_offset``: the target's (the reference reads it from the station table), needed with a reanalysis
    reader."""
    if tair_mask is not None:
        raise NotImplementedError("tair_mask (cross-validation masking) belongs to step15 and is not implemented")
    if chk_perf:
        raise NotImplementedError("chk_perf (the retry ladder of InfillMatrixPPCA.infill) is not implemented for one "
                                  "target at a time: call infill_daily(chk_perf=True), which batches it over the items")
    if not add_bestngh:
        raise NotImplementedError("add_bestngh=False is not supported by build_infill_matrices")
    month = np.asarray(pool.days[MONTH], np.int64)
    masks = [] if day_masks is None else [np.asarray(k) for k in day_masks]
    if len(masks) != 12 or any(k.shape != month.shape or not np.array_equal(k, month == g + 1) for g, k in enumerate(masks)):
        raise NotImplementedError("day_masks other than the twelve calendar months are not implemented")
    r = infill_daily(pool, tair_var, [stn_id], mean, vari, nnr_ds, None if utc_offset is None else [utc_offset], min_daily_nnghs, nnghs_nnr, max_nnr_var, npcs,
                     frac_obs_initnpcs, ppca_varyexplain, ppcaConThres, device=device)
    return r.fnl_tair[0], r.mask_infill[0], r.infill_tair[0]
