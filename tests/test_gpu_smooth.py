"""k_select's smoothing of the station parameters (twx_select.h: the kriging bandwidth kk[m], the GWR bandwidth ka[m] and the
variogram of every month, each a bisquare-weighted mean over the neighbours whose field is finite, and the month-ordered
status) on station tables whose fields are NaN raggedly -- by station, month and family (tests/smooth_cases.py).  The
all-months form of the kernel reuses the previous month's sum of weights when the ballot masks of the finite neighbours are
equal; every other table of the suite has the same mask in every month and family.  The integers -- status, kk through
last_bandwidths, `used` of the point entries -- must be EXACTLY the oracle's on every pattern; tests/test_oracle_smooth.py
shows on the CPU that a kernel which took a sum of weights from the previous month, from another family's mask, from the
ranks past init_nnghs, or rounded ties away from zero would change them in hundreds of items.  Floating-point results are
compared where the status is 0, at the bars of tests/grid_bars.py (normals, SE, kriged mean / variance and the fp64 series of
the point entries within FAST_BAR = 1e-5 degC, packed daily values within 1).

(a) grid, all-months form, k_select<4, 0>: 24 x 24 (normals) and 12 x 12 (daily: ka shows only there), both variables;
(b) points, all-months form: interp_points on 48 of those cells, normals, then daily;
(c) points, month-by-month form (smooth3): krig_points / gwr_points of every (point, month) without nnghs -- against the oracle
    and against (b)'s kk: the two forms must agree with each other;
(d) init_nnghs = 63, 64, 65, 100, 128, 129 (the kernel keeps 3 slots of 64 ranks per lane) through (b), independent NaN, p = 0.5;
(e) k_select<1, 1>: a 16 x 16 window inside a dense ragged cluster whose tiles cannot have taken the short-list launch.

Measured on gfx950 (the tests print these): every integer equal on all nine patterns and all five paths; grids within 1.9e-6
degC of the oracle's in normals / SE (f4 outputs) with 0 .. 9 int16 days of a window off by one; points within 9.7e-7 degC in
normals and daily values, 1.7e-7 in SE and kriging variance; the month form's GWR series within 8.8e-14.  The dead table
fails 226 of the 576 cells of the normals window and 97 of the 144 of the daily one.  No kernel needed a fix.  With the sum of
weights reused whenever there is a previous month (a scratch build, run once) 32 of the 34 tests fail -- the independent
pattern at p = 0.5 in 502 of 576 (point, month) bandwidths of Tmin; the month form of the dead and the families tables
passes, as it must: smooth3 has no sum to reuse."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

import smooth_cases as sc  # noqa: E402
from grid_bars import FAST_BAR, assert_fast_oracle_where  # noqa: E402

pytestmark = pytest.mark.gpu
VARS = ("tmin", "tmax")
NCLUSTER = 2500                                              # (e): 1500 leaves fewer than 512 stations within 2 hd of a tile


def _var(lib, var):
    return lib.TMIN if var == "tmin" else lib.TMAX


@pytest.fixture(scope="module", params=sc.PATTERNS)
def cs(request, golden_case):
    return sc.case(request.param, golden_case)


def _context(table, init=sc.INIT):
    from topowx_amd import _lib as lib
    ctx = lib.Context(init_nnghs=init)
    for var in VARS:
        ctx.set_stations(_var(lib, var), table[var])
    return lib, ctx


def _pts(ctx, grid, cells, var):
    r, c = cells[:, 0], cells[:, 1]
    return ctx.make_pts(grid["lon"][c], grid["lat"][r], grid["elev"][r, c], grid["tdi"][r, c], grid[sc.lst_key(var)][:, r, c].T)


def _bandwidths(lib, ctx, var, ncell):
    kk = ctx.last_bandwidths(_var(lib, var), max_cells=ncell)
    assert kk.shape == (ncell, 12), kk.shape
    return kk


def _assert_kk(kk, want, what):
    bad = np.argwhere(kk != want)
    assert bad.size == 0, (what, "%d (cell, month) items" % len(bad), bad[:8].tolist(), kk[kk != want][:8].tolist(),
                           want[kk != want][:8].tolist())


def _grid_run(cs_name, lib, ctx, orc, grid, dbs, prims, win, daily):
    """One window through interp_grid: the oracle's status, its kk of both variables at every cell and month the reference
    reaches (0 elsewhere), and the floating-point outputs where the status is 0."""
    got = ctx.interp_grid(grid, daily=daily, rows=win[0], cols=win[1])
    ncell = got["status"].size
    kk = {v: _bandwidths(lib, ctx, v, ncell) for v in VARS}
    want = orc.interp_grid(dbs["tmin"], dbs["tmax"], orc.params(), grid, daily=daily, nthreads=8, rows=win[0], cols=win[1])
    assert np.array_equal(got["status"], want["status"]), (cs_name, daily, got["status"].tolist(), want["status"].tolist())
    for v in VARS:                                           # the integers first: a wrong bandwidth is named as one
        _assert_kk(kk[v], sc.walked(prims[v], daily)[0], (cs_name, v, "daily" if daily else "normals"))
    worst, off = assert_fast_oracle_where(got, want, (cs_name, daily))
    print("%s grid %s: %d of %d cells fail; normals / SE within %.2g degC; int16 days off by one: %d"
          % (cs_name, "daily" if daily else "normals", int((want["status"] != 0).sum()), ncell, worst, off))
    return want


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def test_grid_all_months_form(cs, orc):
    lib, ctx = _context(cs.table)
    dbs = {v: cs.db(orc, v) for v in VARS}
    for win, daily in ((sc.WIN, False), (sc.DWIN, True)):
        prims = {v: cs.oracle(orc, v, sc.window_cells(win)) for v in VARS}
        want = _grid_run(cs.name, lib, ctx, orc, cs.grid, dbs, prims, win, daily)
        if cs.name == "dead" and not daily:                  # both failures show in one grid
            assert (want["status"] == sc.ERR_NNGHS).sum() >= 20 and (want["status"] == sc.ERR_VARIO).sum() >= 20
        elif cs.name != "dead":
            assert np.all(want["status"] == 0)
    ctx.close()


# ---- (b), (d) -------------------------------------------------------------------------------------------------------------------
def _points_all_months(cs, orc, init):
    """interp_points (normals, then daily) on the 48 point cells with init_nnghs = init; returns {var: kk of the normals run}."""
    lib, ctx = _context(cs.table, init)
    cells, prm, out = sc.point_cells(), orc.params(init_nnghs=init), {}
    for var in VARS:
        db, prims, pts = cs.db(orc, var), cs.oracle(orc, var, cells, init=init), _pts(ctx, cs.grid, cells, var)
        worst = np.zeros(3)
        for daily in (False, True):
            d, norms, se, st = ctx.interp_points(_var(lib, var), pts, daily=daily)
            kk = _bandwidths(lib, ctx, var, len(cells))
            wkk, _, wst = sc.walked(prims, daily)
            ref = [orc.interp(db, prm, cs.oracle_pt(orc, var, r, c), daily=daily) for r, c in cells]
            assert np.array_equal(st, [x[0] for x in ref]) and np.array_equal(st, wst), (cs.name, var, init, daily, st.tolist())
            _assert_kk(kk, wkk, (cs.name, var, init, "daily" if daily else "normals"))
            if not daily:
                out[var] = kk
            for i in np.nonzero(st == 0)[0]:
                _, wd, wn, ws = ref[i]
                e = [np.abs(norms[i] - wn).max(), np.abs(se[i] - ws).max(), 0.0]
                assert max(e) <= FAST_BAR, (cs.name, var, init, i, e)
                if daily:
                    e[2] = np.abs(d[i] - wd).max()
                    assert np.abs(orc.pack_i16(d[i]).astype(int) - orc.pack_i16(wd).astype(int)).max() <= 1, (cs.name, var, init, i, e)
                worst = np.maximum(worst, e)
        print("%s init_nnghs %d %s points: %d of %d fail; worst |GPU - oracle| (normals, SE, daily): %s"
              % (cs.name, init, var, int((wst != 0).sum()), len(cells), worst.tolist()))
    ctx.close()
    return out


def test_points_all_months_form(cs, orc):
    _points_all_months(cs, orc, sc.INIT)


@pytest.mark.parametrize("init", sc.K_EDGES)
def test_slot_edges_of_init_nnghs(golden_case, orc, init):
    kk = _points_all_months(sc.case("indep50", golden_case), orc, init)
    assert np.unique(kk["tmin"]).size > 4


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def test_points_month_form(cs, orc):
    """Every (point, month) as a request of its own (no nnghs, no variogram: smooth3).  A month alone does not see the earlier
    months' failures: the statuses are the oracle's of that month.  Where the all-months form reached the month, `used` is
    its kk."""
    lib, ctx = _context(cs.table)
    cells, prm = sc.point_cells(), orc.params()
    rep, mth = np.repeat(np.arange(len(cells)), 12), np.tile(np.arange(1, 13), len(cells))
    for var in VARS:
        db, pts = cs.db(orc, var), _pts(ctx, cs.grid, cells, var)
        ctx.interp_points(_var(lib, var), pts, daily=False)
        kk_all = _bandwidths(lib, ctx, var, len(cells)).ravel()
        mean, var_, used, st, _ = ctx.krig_points(_var(lib, var), pts[rep], mth)
        out, used_a, st_a = ctx.gwr_points(_var(lib, var), pts[rep], 0.0, mth)
        worst = np.zeros(3)
        for i, (p, m) in enumerate(zip(rep, mth)):
            pt = cs.oracle_pt(orc, var, *cells[p])
            rc, wm, wv, wu, _ = orc.krig(db, prm, pt, int(m))
            assert st[i] == rc and (rc or used[i] == wu), (cs.name, var, "krig", cells[p].tolist(), m, st[i], rc, used[i], wu)
            rc_a, series, wu_a, _, _ = orc.gwr_mth(db, prm, pt, 0.0, int(m))
            assert st_a[i] == rc_a and (rc_a or used_a[i] == wu_a), (cs.name, var, "gwr", cells[p].tolist(), m, st_a[i], rc_a, used_a[i], wu_a)
            e = np.zeros(3)
            if not rc:
                e[:2] = abs(mean[i] - wm), abs(var_[i] - wv)
            if not rc_a:
                e[2] = np.abs(out[i, :series.size] - series).max()
            assert e.max() <= FAST_BAR, (cs.name, var, cells[p].tolist(), m, e.tolist())
            worst = np.maximum(worst, e)
        reached = kk_all > 0
        assert reached.sum() >= 12 and np.array_equal(used[reached], kk_all[reached]), (cs.name, var, "the two forms disagree")
        print("%s %s month form: %d krig / %d gwr requests of %d fail; worst |GPU - oracle| (mean, var, series): %s"
              % (cs.name, var, int((st != 0).sum()), int((st_a != 0).sum()), rep.size, worst.tolist()))
    ctx.close()


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
def test_long_list_launch(golden_case, orc):
    """k_select<1, 1>: every candidate list of a tile holds the stations within 2 hd of its centre, so a tile with more than
    TWX_CAND_SMALL of them cannot have gone through the short-list launch."""
    tables, inside = sc.cluster_tables(golden_case, NCLUSTER)
    for v in VARS:
        assert max(inside[v]) > sc.CAND_SMALL, (v, inside[v])
    print("stations within 2 hd of the tile centres:", inside)
    lib, ctx = _context(tables)
    grid = golden_case[0]
    dbs = {v: orc.Db(tables[v]) for v in VARS}
    cells = sc.window_cells(sc.CLUSTER_WIN)
    prims = {v: [sc.primitives_oracle(orc, dbs[v], orc.params(), grid["lon"][c], grid["lat"][r]) for r, c in cells] for v in VARS}
    want = _grid_run("cluster", lib, ctx, orc, grid, dbs, prims, sc.CLUSTER_WIN, True)
    ctx.close()
    assert np.all(want["status"] == 0) and len({tuple(p["k"]) for p in prims["tmin"]}) > 4
