#!/usr/bin/env python3
"""Golden vectors of step15's cross-validation of the infill (build container only; needs the reference tree, see
make_golden.py):

    python tests/golden/make_golden_xvalinfill.py

Executed: twx/infill/xval_infill.py:32-164 (``XvalInfill.__init__`` and ``run_xval``), twx/infill/infill_normals.py:452-517
(``infill_mean_variance``) on ``_InfillMatrix`` as make_golden_infillmat.py loads it, twx/infill/infill_daily.py:526-561
(``infill_daily_obs``) on ``InfillMatrixPPCA`` as make_golden_ppca.py loads it -- both called with the ``tair_mask`` that
``XvalInfill.__init__`` made.  The loaders and stubs of those two makers are imported; the makers are unchanged.  No
reference text is stored.

Shims and stand-ins.  The R boundary is stood in for by the project's restatements: ``r.infill_mu_sigma`` is
tests/restate_emnorm.py on the matrix the reference hands it, ``r.ppca_tair`` is tests/restate_ppca.py (``search``) on
its arguments, scaled back with the target's norm and std.  What is recorded of the estimators is therefore NOT a result of
R; the golden pins the orchestration: masks, neighbour lists, the station table's set-then-restore, the NaN patterns.
``InfillMatrixPPCA.infill`` is the slice of make_golden_ppca.py, which leaves the ``chk_perf`` block out (Python-2 ``print``
statements), so ``chk_perf`` is False here.  Stage 1 gets the seeded stand-in reanalysis of make_golden_infillmat, stage 2
none (make_golden_ppca's pool A).  A stub station table carries the fields ``mean_tminMM`` / ``vari_tminMM`` (the names of
``get_mean_varname`` / ``get_variance_varname``, twx/db/station_data.py:76-88, restated as two one-line functions), ``days``,
``stn_idxs`` and ``load_all_stn_obs_var``.

Pool (``case_inputs()``, pinned by ``input_hash``): make_golden_ppca's 18 stations x 4 years, with station 7 moved onto
station 6 (a co-located pair, distance 0).  Cross-validation stations 0, 1 (each other's neighbours), 6 (one of the
pair) and 15 (records only the second half: at most ``nkeep`` finite days, so nothing of it is held).  ``ntrain_yrs`` = 2:
``nkeep`` = 730, about half of a full record is held.

Recorded per cross-validation station: the held mask; per stage (1: mean / variance, 2: daily) and month the ranked
stations (each ranked column matched to its station by distance and content), ``ioa``, ``dist``, ``nnghs`` (the width of the
matrix handed to the shrink, less the target) and ``max_dist``; the twelve means and variances the station table holds
when ``infill_daily_obs`` is entered and after ``run_xval`` has returned; the NaN pattern of the two returned series.

The script asserts, and refuses to write otherwise (the remedy is another seed): the restatement of the matrix builder
(tests/restate_infillmat.py on a pool copy with the target's column masked) equals the executed lists, nnghs and
max_dist, with ioa within 1e-10; the margins of DESIGN.md section 16 (no two ioa of an item within 1e-9, no candidate
within 1e-9 of its bounds, no distance within 1e-6 km of a ring boundary); 0 and 1 rank each other; 6 ranks 7 at
distance 0; the table is restored bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_infillmat as mk  # noqa: E402
import make_golden_ppca as mp  # noqa: E402
import restate_emnorm as RE  # noqa: E402
import restate_infillmat as RI  # noqa: E402
import restate_ppca as RP  # noqa: E402
from topowx_amd.dates import MONTH  # noqa: E402

XVAL = (0, 1, 6, 15)
TWIN = (6, 7)
NTRAIN_YRS = 2
OUT = os.path.join(HERE, "golden_xvalinfill_v1.npz")


def case_inputs():
    """(ids, lon, lat, tmin [ndays, n] float32, days): make_golden_ppca's pool with a co-located pair."""
    ids, lon, lat, tmin, days = mp.case_inputs()
    lon, lat = lon.copy(), lat.copy()
    lon[TWIN[1]], lat[TWIN[1]] = lon[TWIN[0]], lat[TWIN[0]]
    return ids, lon, lat, tmin, days


def mean_name(var, mth):
    return "mean_%s%02d" % (var, mth)


def vari_name(var, mth):
    return "vari_%s%02d" % (var, mth)


def stn_table(ids, lon, lat, tmin, days, mean, vari):
    da = mk._StnDa(ids, lon, lat, tmin)
    dt = da.stns.dtype.descr + [(mean_name("tmin", m), np.float64) for m in range(1, 13)] + \
        [(vari_name("tmin", m), np.float64) for m in range(1, 13)]
    stns = np.empty(ids.size, dtype=dt)
    for name in da.stns.dtype.names:
        stns[name] = da.stns[name]
    for g in range(12):
        stns[mean_name("tmin", g + 1)], stns[vari_name("tmin", g + 1)] = mean[:, g], vari[:, g]
    da.stns, da.stn_ids, da.days = stns, stns["station_id"], days
    da.stn_idxs = {s: i for i, s in enumerate(ids)}
    return da


def match(mat_cols, d, dall, rows):
    """The station of every ranked column: nearest in distance, equal distances told apart by the column's content."""
    out = []
    for c in range(d.size):
        cand = [s for s in np.nonzero(np.abs(dall - d[c]) < 1e-9)[0] if s not in out]
        if len(cand) > 1:
            cand = [s for s in cand if np.array_equal(mat_cols[:, c], rows[:, s], equal_nan=True)]
        assert len(cand) == 1, "a ranked column matches %d stations: try another seed" % len(cand)
        out.append(int(cand[0]))
    return np.array(out, np.int32)


def main():
    import make_golden as mg
    ids, lon, lat, tmin, days = case_inputs()
    mean, vari = mp.normals_of(tmin, days)
    n, nd = ids.size, days.size
    month = np.asarray(days[MONTH]) - 1
    log, rec = mk._Log(), mp._Rec()
    log.reset()
    ns1 = mk.load_slice(log)                                        # _InfillMatrix
    ns2 = mp.load_slice(rec)                                        # InfillMatrixPPCA (its own namespace: both define _shrink_matrix)
    state = dict(stage1=[], stage2=[], entered=None, shrink2=None)

    class R1(object):
        @staticmethod
        def infill_mu_sigma(m):
            log.given = np.array(m)
            r = RE.run(np.array(m, np.float64))
            return r["mean"], r["variance"]

    class Rx(object):
        def __init__(self, fit):
            self.fit = fit

        def rx(self, name):
            assert name == "ppca_fit"
            return self.fit[None, :]

    class R2(object):
        @staticmethod
        def ppca_tair(m, norms, stds, **kw):
            m, norms, stds = np.array(m, np.float64), np.array(norms, np.float64), np.array(stds, np.float64)
            a = RP.search((m - norms) / stds, None, kw["npcs"], kw["frac_obs"], kw["max_r2cum"], kw["convThres"])
            assert a["status"] in (RP.OK, RP.MAXITS), "a month was not fitted: try another seed"
            return Rx(np.asarray(a["fit"], np.float64) * stds[0] + norms[0])

    ns1.update(r=R1, _load_R=lambda: None)
    ns2.update(r=R2)
    exec(compile("\n" * 451 + mg._slice("twx/infill/infill_normals.py", 452, 517), "infill_normals.py", "exec"), ns1)
    exec(compile("\n" * 525 + mg._slice("twx/infill/infill_daily.py", 526, 561), "infill_daily.py", "exec"), ns2)
    infill1, infill2, shrink2 = ns1["_InfillMatrix"].infill, ns2["InfillMatrixPPCA"].infill, ns2["_shrink_matrix"]

    def rec_infill1(self, *a, **k):
        out = infill1(self, *a, **k)
        state["stage1"].append(dict(d=np.array(self.ngh_dists[1:], np.float64), ioa=np.array(self.ngh_ioa[1:], np.float64),
                                    cols=np.array(self.imp_tair_mat[:, 1:], np.float64), max_dist=float(self.max_dist),
                                    nnghs=log.shrink_in.shape[1] - 1, mask=np.array(self.day_mask, bool)))
        return out

    def rec_shrink2(m, *a):
        state["shrink2"] = np.asarray(m).shape[1] - 1
        return shrink2(m, *a)

    def rec_infill2(self, *a, **k):
        out = infill2(self, *a, **k)
        state["stage2"].append(dict(d=np.array(self.ngh_dists[1:], np.float64), ioa=np.array(self.ngh_ioa[1:], np.float64),
                                    cols=np.array(self.pca_tair[:, 1:], np.float64), max_dist=float(self.max_dist),
                                    nnghs=state["shrink2"], mask=np.array(self.day_mask, bool)))
        return out

    ns1["_InfillMatrix"].infill, ns2["InfillMatrixPPCA"].infill, ns2["_shrink_matrix"] = rec_infill1, rec_infill2, rec_shrink2
    stn_da = stn_table(ids, lon, lat, tmin, days, mean, vari)
    daily0 = ns2["infill_daily_obs"]

    def daily(stn_id, da, *a, **k):
        x = da.stn_idxs[stn_id]
        state["entered"] = (np.array([da.stns[mean_name("tmin", m)][x] for m in range(1, 13)]),
                            np.array([da.stns[vari_name("tmin", m)][x] for m in range(1, 13)]))
        return daily0(stn_id, da, *a, **k)

    nsx = dict(np=np, os=os, MONTH=MONTH, get_mean_varname=mean_name, get_variance_varname=vari_name,
               infill_mean_variance=ns1["infill_mean_variance"], infill_daily_obs=daily, InfillMatrixPPCA=ns2["InfillMatrixPPCA"])
    exec(compile("\n" * 31 + mg._slice("twx/infill/xval_infill.py", 32, 164), "xval_infill.py", "exec"), nsx)

    class Params(object):
        nnr_ds, min_daily_nnghs, nnghs_nnr, max_nnr_var, chk_perf, npcs = None, 3, 4, 0.99, False, 0
        frac_obs_initnpcs, ppca_varyexplain, verbose = 0.5, 0.99, False

    class Nnr12(object):                                            # stage 1: the stand-in reanalysis; stage 2: none
        one, two = mk._Nnr(nd), mp._NoNnr(nd)

    xids = ids[list(XVAL)]
    assert list(xids) == sorted(xids)                               # the stub loads columns in table order
    xv = nsx["XvalInfill"](stn_da, "tmin", Params, xids, NTRAIN_YRS)
    held = np.array(xv.stn_xval_masks)
    nkeep = int(np.round(NTRAIN_YRS * 365.25))
    assert nkeep == 730 and held.shape == (len(XVAL), nd)
    nfin = np.isfinite(tmin[:, list(XVAL)]).sum(axis=0)
    assert nfin[3] <= nkeep and not held[3].any()
    assert ((0.35 < held[:3].sum(axis=1) / nfin[:3]) & (held[:3].sum(axis=1) / nfin[:3] < 0.6)).all()      # about half of a record
    table0 = stn_da.stns.copy()
    out = dict(input_hash=mk.input_hash(ids, lon, lat, tmin, days), xval=np.array(XVAL, np.int32), nkeep=np.int32(nkeep),
               ntrain_yrs=np.float64(NTRAIN_YRS), held=np.packbits(held, axis=1), ndays=np.int32(nd), mean=mean, vari=vari)
    margins = dict(ioa=np.inf, cand=np.inf, ring=np.inf)
    with np.errstate(divide="raise", invalid="raise"):
        for t, s in enumerate(XVAL):
            state.update(stage1=[], stage2=[], entered=None)
            # the reference's nnr_ds is one object for both stages; the two loaders need different stand-ins
            Params.nnr_ds = Nnr12.one
            ms0 = ns1["infill_mean_variance"]

            def ms(*a, **k):
                r = ms0(*a, **k)
                Params.nnr_ds = Nnr12.two
                return r
            nsx["infill_mean_variance"] = ms
            obs_tair, infill_tair = xv.run_xval(ids[s])
            assert len(state["stage1"]) == 12 and len(state["stage2"]) == 12
            after = (np.array([stn_da.stns[mean_name("tmin", m)][s] for m in range(1, 13)]),
                     np.array([stn_da.stns[vari_name("tmin", m)][s] for m in range(1, 13)]))
            assert stn_da.stns.tobytes() == table0.tobytes(), "the station table was not restored"
            assert np.array_equal(after[0], mean[s]) and np.array_equal(after[1], vari[s])
            assert not np.array_equal(state["entered"][0], mean[s]) or not held[t].any()
            out["entered_mean_%d" % t], out["entered_vari_%d" % t] = state["entered"]
            out["after_mean_%d" % t], out["after_vari_%d" % t] = after
            out["obs_nan_%d" % t], out["infill_nan_%d" % t] = np.packbits(np.isnan(obs_tair)), np.packbits(np.isnan(infill_tair))
            assert np.array_equal(np.isnan(obs_tair), ~held[t]) and np.array_equal(np.isnan(infill_tair), ~held[t])
            # the lists of both stages, and the restatement on a pool copy with the target's column masked
            cp = tmin.copy()
            cp[held[t], s] = np.nan
            dall = ns1["grt_circle_dist"](lon[s], lat[s], lon, lat)
            dall[s] = -1.0
            m2 = mean.copy()
            m2[s] = state["entered"][0]
            v2 = vari.copy()
            v2[s] = state["entered"][1]
            for stage, key in ((1, "stage1"), (2, "stage2")):
                off, idx, ioa, dist, nnghs, maxd = [0], [], [], [], [], []
                for g in range(12):
                    it = state[key][g]
                    assert np.array_equal(it["mask"], month == g)
                    cols = match(it["cols"], it["d"], dall, cp[month == g].astype(np.float64))
                    elig = np.isfinite(mean[:, 0]) if stage == 1 else np.isfinite(m2[:, g]) & np.isfinite(v2[:, g])
                    grp = np.where(month == g, 0, -1).astype(np.int8)
                    w = RI.run(lon, lat, cp, elig, [s], grp)
                    assert w["status"][0, 0] == RI.OK and not RI.knife(w).any(), "a knife-edge item: try another seed"
                    assert np.array_equal(w["idx"], cols), "the restatement ranks other stations (stage %d, %d, %d)" % (stage, s, g)
                    assert w["nnghs"][0, 0] == it["nnghs"] and w["max_dist"][0, 0] == it["max_dist"]
                    assert np.abs(w["ioa"] - it["ioa"]).max() < 1e-10
                    margins["ioa"] = min(margins["ioa"], float(w["ioa_gap"].min()))
                    margins["cand"] = min(margins["cand"], float(w["cand_margin"].min()))
                    margins["ring"] = min(margins["ring"], float(w["ring_margin"].min()))
                    off.append(off[-1] + cols.size)
                    idx.append(cols); ioa.append(it["ioa"]); dist.append(it["d"])
                    nnghs.append(it["nnghs"]); maxd.append(it["max_dist"])
                out["s%d_off_%d" % (stage, t)] = np.array(off, np.int32)
                out["s%d_idx_%d" % (stage, t)] = np.concatenate(idx)
                out["s%d_ioa_%d" % (stage, t)] = np.concatenate(ioa)
                out["s%d_dist_%d" % (stage, t)] = np.concatenate(dist)
                out["s%d_nnghs_%d" % (stage, t)] = np.array(nnghs, np.int32)
                out["s%d_max_dist_%d" % (stage, t)] = np.array(maxd)
            print("station %d: held %d of %d finite days" % (s, held[t].sum(), nfin[t]), flush=True)
    print("margins: ioa gap %.3g, candidate %.3g, ring boundary %.3g km" % (margins["ioa"], margins["cand"], margins["ring"]))
    assert margins["ioa"] > mk.IOA_GAP and margins["cand"] > mk.CAND_GAP and margins["ring"] > mk.RING_GAP, "try another seed"
    # two cross-validation stations that are each other's neighbours, with their FULL records; the co-located twin
    assert XVAL[1] in out["s1_idx_0"] and XVAL[0] in out["s1_idx_1"] and XVAL[1] in out["s2_idx_0"] and XVAL[0] in out["s2_idx_1"]
    a = out["s1_idx_2"][:out["s1_off_2"][1]]
    assert TWIN[1] in a and out["s1_dist_2"][:a.size][a == TWIN[1]][0] == 0.0
    out.update(ioa_gap=margins["ioa"], cand_margin=margins["cand"], ring_margin=margins["ring"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(HERE, "golden_ppca_v1.npz"))


if __name__ == "__main__":
    main()
