"""A numpy restatement of the infill neighbour matrices (``twxif_infill_matrix``, include/twx_qa.h; the reference's
``_InfillMatrix.__init__`` / ``infill`` / ``_shrink_matrix``, twx/infill/infill_normals.py:52-237, 324-343, 391-420) in a
formulation of its own: all pair statistics of a ring at once as masked matrix sums, the best-neighbour candidate as the
first maximum of the candidates' ioa, the daily neighbour counts as cumulative sums over the rank-ordered columns
(``cum[:, k - 1]`` is the count among the first k), the selection loop and the shrink on those.  Used by the CPU tests
against the executed-reference golden and by the GPU tests as the expectation on random pools.

``run`` returns the arrays of the GPU call plus, per item, the decision margins the tests use to leave knife-edge items
out: the smallest gap between two ioa of a ranking that was used, the distance of a best-neighbour candidate's ioa from
0.7 / from the ring's best ranked ioa / from another candidate's, and the distance of a station from a ring boundary.
"""
import numpy as np

OK, NUMERIC, NGH_CAP, NO_TARGET_OBS, UNSATISFIED = 0, 4, 7, 18, 19
RADIAN, EARTH_KM = 0.017453292519943295, 6371.009
MAX_DISTANCE, RING_KM, MIN_POR_OVERLAP, BEST_MIN_IOA = 75.0, 37.5, 2.0 / 3.0, 0.7


def haversine(lon1, lat1, lon2, lat2):
    la1, la2, lo1, lo2 = lat1 * RADIAN, lat2 * RADIAN, lon1 * RADIAN, lon2 * RADIAN
    h = np.sin((la1 - la2) / 2) ** 2 + np.cos(la1) * np.cos(la2) * np.sin((lo1 - lo2) / 2) ** 2
    return EARTH_KM * 2 * np.arcsin(np.sqrt(h))


def thresholds(target_obs, group, ngroups):
    """nthres_all [G], nthres_target_por [ntarget, G] (infill_normals.py:110-115); target_obs [ntarget, ndays]."""
    nall = np.array([np.round(MIN_POR_OVERLAP * int((group == g).sum())) for g in range(ngroups)])
    npor = np.array([[np.round(MIN_POR_OVERLAP * int(np.isfinite(row[group == g]).sum())) for g in range(ngroups)]
                     for row in target_obs]).reshape(len(target_obs), ngroups)
    return nall.astype(np.int32), npor.astype(np.int32)


class _Rings(object):
    """The ring sequence of one target: stations by ascending distance (stable: equal distances in table order)."""

    def __init__(self, dist, eligible, self_col):
        ok = eligible.copy()
        ok[self_col] = False
        cols = np.nonzero(ok)[0]
        order = np.argsort(dist[cols], kind="stable")
        self.cols, self.d = cols[order], dist[cols][order]
        self.rings = []                                            # (outer radius, first, last, boundary margin)
        self.pos, self.rout = 0, None

    def ring(self, k):
        """Ring k as (outer radius, columns, distances), or None when no station lies beyond the inner radius."""
        while len(self.rings) <= k:
            if self.pos >= self.cols.size:
                return None
            rout = MAX_DISTANCE if self.rout is None else self.rout + RING_KM
            while not self.d[self.pos] <= rout:
                rout += RING_KM
            end = int(np.searchsorted(self.d, rout, side="right"))
            # the stations of the ring and just beyond it against every boundary k * 37.5 >= 75 that was tried
            near = self.d[self.pos:int(np.searchsorted(self.d, rout + 1.0, side="right"))]
            bound = np.round(near / RING_KM) * RING_KM
            sel = bound >= MAX_DISTANCE
            margin = float(np.abs(near - bound)[sel].min()) if sel.any() else np.inf
            self.rings.append((rout, self.pos, end, margin))
            self.pos, self.rout = end, rout
        rout, a, b, margin = self.rings[k]
        return rout, self.cols[a:b], self.d[a:b], margin


def _pair_stats(T, X):
    """T [nd] target, X [nd, k] ring stations (float64, NaN = missing): nlap, nlap_stn, ioa, denominator."""
    fx, ft = np.isfinite(X), np.isfinite(T)
    both = fx & ft[:, None]
    nlap, nst = fx.sum(axis=0), both.sum(axis=0)
    Tz = np.where(ft, T, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (both * Tz[:, None]).sum(axis=0) / nst
        Xz = np.where(both, X, 0.0)
        num = np.where(both, np.abs(Xz - Tz[:, None]), 0.0).sum(axis=0)
        den = np.where(both, np.abs(Xz - mean[None, :]) + np.abs(Tz[:, None] - mean[None, :]), 0.0).sum(axis=0)
        ioa = 1.0 - num / den
    return nlap, nst, ioa, den


def run_item(T, pool_obs, rings, nthres_all, nthres_por, min_nnghs=3, cap=256):
    """One item.  T [nd]: the target on the item's days; pool_obs [nd, n]: the pool on them (float32 or float64)."""
    out = dict(status=UNSATISFIED, nnghs=min_nnghs, max_dist=np.nan, idx=np.zeros(0, np.int32), ioa=np.zeros(0),
               dist=np.zeros(0), nlap=np.zeros(0, np.int32), nlap_stn=np.zeros(0, np.int32), keep=np.zeros(0, np.uint8),
               ioa_gap=np.inf, cand_margin=np.inf, ring_margin=np.inf, nrings=0, cand_kept=False, cand_rejected="")
    if nthres_por == 0:
        out["status"] = NO_TARGET_OBS
        return out
    T = T.astype(np.float64)
    L = {k: [] for k in ("idx", "ioa", "dist", "nlap", "nlap_stn")}
    rank = np.zeros(0, np.int64)                                   # positions of L in ranked order
    V = np.zeros((T.size, 0), bool)                                # finite mask of the ranked columns, in list order
    nn, k = min_nnghs, 0

    def fail(status):
        out.update(status=status, idx=np.zeros(0, np.int32), ioa=np.zeros(0), dist=np.zeros(0), nlap=np.zeros(0, np.int32),
                   nlap_stn=np.zeros(0, np.int32), keep=np.zeros(0, np.uint8), nnghs=nn)
        return out

    def finish(keep):
        o = rank
        out.update(idx=np.array(L["idx"], np.int32)[o], ioa=np.array(L["ioa"], np.float64)[o],
                   dist=np.array(L["dist"], np.float64)[o], nlap=np.array(L["nlap"], np.int32)[o],
                   nlap_stn=np.array(L["nlap_stn"], np.int32)[o], keep=keep, nnghs=nn)
        return out

    while True:
        n = len(L["idx"])
        cum = np.cumsum(V[:, rank], axis=1) if n else np.zeros((T.size, 0), np.int64)
        if n >= nn:
            if cum[:, nn - 1].min() < min_nnghs:
                nn += 1
                continue
            break
        r = rings.ring(k)                                          # fewer than nn ranked: the next ring
        if r is None:
            return finish(np.zeros(n, np.uint8))                   # unsatisfied, the list as far as it got
        rout, cols, d, margin = r
        k += 1
        out["nrings"], out["max_dist"] = k, rout
        out["ring_margin"] = min(out["ring_margin"], margin)
        if cols.size > cap:
            return fail(NGH_CAP)
        X = pool_obs[:, cols].astype(np.float64)
        nlap, nst, ioa, den = _pair_stats(T, X)
        por = nst >= nthres_por
        acc = por & (nlap >= nthres_all)
        cnd = por & ~acc if k == 1 else np.zeros(cols.size, bool)
        # the ring is scanned in distance order and the first station that fails decides: a d1 denominator of 0 at a
        # station the reference would rank or weigh as a candidate, or a full-record station that would be entry cap + 1
        # of the list (at one and the same station the denominator is looked at first)
        p_num = np.nonzero((acc | cnd) & (den == 0))[0]
        p_cap = np.nonzero(acc & (len(L["idx"]) + np.cumsum(acc) > cap))[0]
        if p_num.size and (not p_cap.size or p_num[0] <= p_cap[0]):
            return fail(NUMERIC)
        if p_cap.size:
            return fail(NGH_CAP)
        take = acc.copy()
        pos = np.nonzero(cnd & (ioa > 0))[0]
        if pos.size:
            best = pos[np.argmax(ioa[pos])]                        # the first maximum: only a strictly larger ioa displaces
            top = ioa[acc].max() if acc.any() else 0.0
            cs = np.sort(ioa[pos])
            m = min(abs(ioa[best] - BEST_MIN_IOA), abs(ioa[best] - top), float(cs[0]))
            if cs.size > 1:
                m = min(m, float(np.diff(cs).min()))
            out["cand_margin"] = min(out["cand_margin"], m)
            if ioa[best] >= top and ioa[best] >= BEST_MIN_IOA:
                take[best] = True
                out["cand_kept"] = True
            else:
                out["cand_rejected"] += "m" if ioa[best] < top else ""
                out["cand_rejected"] += "7" if ioa[best] < BEST_MIN_IOA else ""
        for j in np.nonzero(take)[0]:
            L["idx"].append(int(cols[j])); L["ioa"].append(float(ioa[j])); L["dist"].append(float(d[j]))
            L["nlap"].append(int(nlap[j])); L["nlap_stn"].append(int(nst[j]))
        if len(L["idx"]) > cap:
            return fail(NGH_CAP)
        V = np.concatenate([V, np.isfinite(X[:, take])], axis=1)
        rank = np.lexsort((np.array(L["idx"]), -np.array(L["dist"]), -np.array(L["ioa"]))).astype(np.int64)
        if len(L["idx"]) > 1:
            out["ioa_gap"] = min(out["ioa_gap"], float(-np.diff(np.array(L["ioa"])[rank]).max()))
    # the shrink on the first nn ranked columns
    n = len(L["idx"])
    F = V[:, rank[:nn]]
    keep = np.zeros(n, np.uint8)
    keep[:min_nnghs] = 1
    count = F[:, :min_nnghs].sum(axis=1)
    for c in range(min_nnghs, nn):
        if (F[:, c] & (count < min_nnghs)).any():
            keep[c] = 1
            count = count + F[:, c]
    out["status"] = OK
    return finish(keep)


def run(lon, lat, obs, eligible, targets, group, min_nnghs=3, cap=256):
    """lon, lat [n]; obs [ndays, n] float32 (NaN = missing); eligible [n] bool; targets [nt] columns; group [ndays]
    (-1 or 0 .. G - 1).  Returns a dict shaped like the GPU call's result (item = target * G + group), with the per-item
    margins ``ioa_gap``, ``cand_margin``, ``ring_margin`` [nt, G]."""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    group = np.asarray(group)
    G = int(group.max()) + 1
    targets = np.asarray(targets)
    nt = targets.size
    nall, npor = thresholds(obs[:, targets].T, group, G)
    res = dict(status=np.zeros((nt, G), np.int32), nnghs=np.zeros((nt, G), np.int32), max_dist=np.zeros((nt, G)),
               nthres_all=nall, nthres_target_por=npor, ioa_gap=np.zeros((nt, G)), cand_margin=np.zeros((nt, G)),
               ring_margin=np.zeros((nt, G)), nrings=np.zeros((nt, G), np.int32), cand_kept=np.zeros((nt, G), bool),
               cand_rejected=np.zeros((nt, G), "U2"))
    cols = {k: [] for k in ("idx", "ioa", "dist", "nlap", "nlap_stn", "keep")}
    off = [0]
    day_sets = [np.nonzero(group == g)[0] for g in range(G)]
    sub = [obs[d] for d in day_sets]
    for t, s in enumerate(targets):
        rings = _Rings(haversine(lon[s], lat[s], lon, lat), np.asarray(eligible, bool), int(s))
        for g in range(G):
            it = run_item(sub[g][:, s], sub[g], rings, int(nall[g]), int(npor[t, g]), min_nnghs, cap)
            for k in ("status", "nnghs", "max_dist", "ioa_gap", "cand_margin", "ring_margin", "nrings", "cand_kept",
                      "cand_rejected"):
                res[k][t, g] = it[k]
            for k in cols:
                cols[k].append(it[k])
            off.append(off[-1] + it["idx"].size)
    res["off"] = np.array(off, np.int64)
    for k in cols:
        res[k] = np.concatenate(cols[k])
    return res


def knife(res, ioa_gap=1e-9, cand=1e-9, ring=1e-6):
    """The items whose decisions are within the margins the golden maker asserts."""
    return (res["ioa_gap"] < ioa_gap) | (res["cand_margin"] < cand) | (res["ring_margin"] < ring)


def matrix(obs, group, res, targets, t, g, max_cols=31):
    """``.matrix()`` from a result dict: the target, then the first ``max_cols - 1`` kept stations in rank order."""
    G = res["status"].shape[1]
    i = t * G + g
    s = slice(int(res["off"][i]), int(res["off"][i + 1]))
    kept = res["idx"][s][res["keep"][s] != 0][:max_cols - 1]
    c = np.concatenate([[targets[t]], kept]).astype(np.int64)
    return obs[np.ix_(np.nonzero(np.asarray(group) == g)[0], c)].astype(np.float64)
