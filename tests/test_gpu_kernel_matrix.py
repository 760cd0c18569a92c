"""Every kriging kernel instance, in every build, against the oracle (and the 40-digit arbiter where the oracle's bar fails).

run_uk_stage (twx_hip.hip) sends each system to one of ~30 kernel instances: the fast build (k_ukw / k_ukwz <3..6>,
k_uk<7..10>; PREC = 0), the fp64 build of the system's own size (the same 12 shapes, PREC = 1: TWX_FLAG_UK_F64_ALL and
routed systems), the fp64 build inside one of four coarse sizes (the tie guard's second pass, twx_f64_coarse_bucket) and
the fp64 build with per-element distances in the 112- or 160-row kernel (PREC = 2: TWX_FLAG_NO_HOST_SYNC).  A kernel that
is wrong at one matrix size, in one build, on one path fails one of these tests:

(a) point mode (k_cell_dist), EVERY k from 6 to TWX_MAX_NNGHS, four variograms, four contexts;
(b) grid mode (k_tile_dist) with every station's bandwidth set to a per-month constant K_m, three sets of K_m covering the
    bucket edges, against the oracle's daily grid;
(c) the same K_m with a Tmax table that is the Tmin table + delta: every day of every cell is a near tie, so every cell
    goes through the tie guard and hence through the coarse fp64 buckets at every size.

Measured on gfx950 (max |d| against the oracle over mean and variance, point mode, all k and variograms): fast build
1.4e-6 degC; fp64 build of the own size 6.9e-14; PREC = 2 6.9e-14.  Against the arbiter at each fp64 instance's largest k
(long range): own size 3.2e-14, PREC = 2 3.2e-14, oracle 1.8e-14.  Grid mode: the fp64 builds and the coarse tie-guard
build give the oracle's f4 bits, status, ninvalid and daily values everywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

from grid_bars import F64_BAR, FAST_BAR, assert_f4_oracle as _assert_f4_oracle, assert_fast_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

KMIN, KMAX = 6, 152                                          # TWX_MAX_NNGHS (include/twx.h)
VARIOS = (None, (0.25, 1.4, 60.0), (0.8, 0.0, 0.0), (0.05, 2.0, 900.0))   # default, mid, pure nugget, long range
LONG = 3                                                     # the ill-conditioned one
# largest k of each fp64 kernel instance (twx_krig_bucket: 40, 48, .. 96 one-wave; 104 k_uk<7>, 120 <8>, 136 <9>, 152 <10>)
INSTANCE_KMAX = (40, 48, 56, 64, 72, 80, 88, 96, 104, 120, 136, 152)
# per-month constant bandwidths: every bucket edge of twx_krig_bucket and of twx_f64_coarse_bucket
KSETS = ((6, 9, 16, 17, 31, 33, 40, 41, 48, 49, 56, 57),
         (63, 65, 72, 73, 80, 81, 88, 89, 95, 97, 104, 105),
         (119, 121, 136, 137, 151, 152, 7, 8, 32, 64, 96, 120))
ROWS, COLS = slice(40, 52), slice(30, 42)                    # 144 cells
TIE_DELTA = 1e-5                                             # degC: Tmax twin = Tmin + delta (see test (c))


def _ctx_flags(lib):
    return {"fast": 0, "f64_all": lib.FLAG_UK_F64_ALL, "no_sync": lib.FLAG_NO_HOST_SYNC,
            "no_sync_f64_all": lib.FLAG_NO_HOST_SYNC | lib.FLAG_UK_F64_ALL}


@pytest.fixture(scope="module")
def points(orc, golden_case):
    """One point per k (cells spread over the grid), its oracle solve per variogram, once for all builds."""
    grid, tmin, _ = golden_case
    ks = np.arange(KMIN, KMAX + 1)
    cells = np.argwhere(np.asarray(grid["mask"]) != 0)
    cells = cells[np.linspace(0, len(cells) - 1, ks.size).astype(int)]
    dbn, prm = orc.Db(tmin), orc.params()
    want = {}
    for vi, vario in enumerate(VARIOS):
        mth = 1 + (vi * 5) % 12
        rows = []
        for i, (r, c) in enumerate(cells):
            pt = orc.make_pt(grid["lon"][c], grid["lat"][r], grid["elev"][r, c], grid["tdi"][r, c], grid["lst_night"][:, r, c])
            rc, m, v, u, idx = orc.krig(dbn, prm, pt, mth, nnghs=int(ks[i]), vario=vario)
            assert rc == 0 and u == ks[i], (ks[i], vario, rc, u)
            rows.append((m, v))
        want[vi] = np.array(rows)
    return dict(grid=grid, tmin=tmin, ks=ks, cells=cells, want=want, dbn=dbn)


def _may_route(vario):
    """uk_may_need_f64 (twx_select.h): can this explicit variogram route a system to the fp64 build at all?"""
    nug, psill, rng = vario
    return rng > 0 and psill > 0 and 2 * 8.0 * nug < psill


def test_point_mode_every_k_every_build(points):
    """(a) Every k from 6 to 152 in one call per (variogram, context): the fast build within 1e-5 degC of the oracle, the
    fp64 builds (own size: TWX_FLAG_UK_F64_ALL and the routed long-range systems; per element in the 112- / 160-row
    kernels: | TWX_FLAG_NO_HOST_SYNC) within 1e-10 degC (they measure ~7e-14), and the timing
    counters show which build ran."""
    from topowx_amd import _lib as lib
    grid, ks, cells, want = points["grid"], points["ks"], points["cells"], points["want"]
    worst, fast_routed = {}, None
    for name, flags in _ctx_flags(lib).items():
        ctx = lib.Context(flags=flags)
        ctx.set_stations(lib.TMIN, points["tmin"], with_obs=False)
        r, c = cells[:, 0], cells[:, 1]
        pts = ctx.make_pts(grid["lon"][c], grid["lat"][r], grid["elev"][r, c], grid["tdi"][r, c], grid["lst_night"][:, r, c].T)
        routed = {}
        for vi, vario in enumerate(VARIOS):
            mth = 1 + (vi * 5) % 12
            mean, var, used, st, _ = ctx.krig_points(lib.TMIN, pts, mth, nnghs=ks,
                                                     vario=None if vario is None else [vario] * ks.size)
            t = ctx.timing()
            assert t["uk_solves"] == ks.size, (name, vario, t["uk_solves"])
            if flags & lib.FLAG_UK_F64_ALL:
                assert t["uk_f64_solves"] == t["uk_solves"], (name, vario, t)
            elif vario is not None and not _may_route(vario):
                assert t["uk_f64_solves"] == 0, (name, vario, t)
            routed[vi] = t["uk_f64_solves"]
            bar = F64_BAR if t["uk_f64_solves"] == ks.size else FAST_BAR          # (routed systems: the fp64 build's bar)
            err = np.maximum(np.abs(mean - want[vi][:, 0]), np.abs(var - want[vi][:, 1]))
            bad = np.nonzero((st != 0) | (used != ks) | ~(err <= bar))[0]              # every failing k at once
            assert bad.size == 0, (name, vario, "k =", ks[bad].tolist(), "status", st[bad].tolist(), err[bad].tolist())
            worst[name] = max(worst.get(name, 0.0), float(err.max()))
        if name == "no_sync":                                   # the same routing decision with and without the host read-back
            assert routed == fast_routed, (routed, fast_routed)
        if name == "fast":
            fast_routed = routed
            assert routed[LONG] == ks.size                      # the long range routes every system (fp64 own size, PREC = 1)
        ctx.close()
    print("point mode, max |d| vs oracle:", worst)


def test_fp64_instances_at_their_largest_k_against_the_arbiter(points):
    """(a) Each fp64 kernel instance at its largest k, long-range variogram (the ill-conditioned one), against the augmented
    system in 40 digits: the own-size build and the per-element build within 1e-10 degC, the fast build within 1e-5 --
    and the oracle too, so that a failure of the oracle bar above says which side is wrong."""
    from oracle import arbiter
    from topowx_amd import _lib as lib
    grid, ks, cells = points["grid"], points["ks"], points["cells"]
    vario, mth = VARIOS[LONG], 1 + (LONG * 5) % 12
    sel = np.searchsorted(ks, INSTANCE_KMAX)
    cols = points["dbn"].cols
    got = {}
    for name, flags in _ctx_flags(lib).items():
        if name == "no_sync":
            continue
        ctx = lib.Context(flags=flags)
        ctx.set_stations(lib.TMIN, points["tmin"], with_obs=False)
        r, c = cells[sel, 0], cells[sel, 1]
        pts = ctx.make_pts(grid["lon"][c], grid["lat"][r], grid["elev"][r, c], grid["tdi"][r, c], grid["lst_night"][:, r, c].T)
        mean, var, used, st, ngh = ctx.krig_points(lib.TMIN, pts, mth, nnghs=ks[sel], vario=[vario] * sel.size, want_idx=True)
        ctx.close()
        assert np.all(st == 0) and np.array_equal(used, ks[sel])
        got[name] = (mean, var, ngh)
    worst = {}
    for j, i in enumerate(sel):
        k = int(ks[i])
        idx = got["f64_all"][2][j, :k]
        for name in got:
            assert np.array_equal(got[name][2][j, :k], idx), (name, k)
        r, c = cells[i]
        pt = (grid["lon"][c], grid["lat"][r], float(grid["elev"][r, c]), float(grid["lst_night"][mth - 1, r, c]))
        am, av = arbiter.uk(cols["lon"][idx], cols["lat"][idx], cols["elev"][idx], cols["lst"][mth - 1, idx],
                            cols["norm"][mth - 1, idx], pt, *vario)
        both = {n: (g[0][j], g[1][j]) for n, g in got.items()}
        both["oracle"] = tuple(points["want"][LONG][i])
        for name, (m, v) in both.items():
            e = max(abs(m - am), abs(v - av))
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= (FAST_BAR if name == "fast" else F64_BAR), (name, k, m, am, v, av)
    print("largest k per fp64 instance, max |d| vs arbiter:", worst)


def _with_bandwidths(stns, K):
    from topowx_amd import stationdb as sdb
    s = stns.copy()
    for m in range(1, 13):
        s[sdb.get_optim_varname(m)] = K[m - 1]
    return s


def _grid_run(lib, grid, tmin, tmax, flags):
    ctx = lib.Context(flags=flags)
    ctx.set_stations(lib.TMIN, tmin)
    ctx.set_stations(lib.TMAX, tmax)
    got = ctx.interp_grid(grid, daily=True, rows=ROWS, cols=COLS)
    t = ctx.timing()
    bw = ctx.last_bandwidths(lib.TMIN)
    ctx.close()
    return got, t, bw


@pytest.mark.parametrize("K", KSETS, ids=lambda K: "K%d" % K[0])
def test_grid_mode_constant_bandwidths(golden_case, orc, K):
    """(b) Grid mode (pair distances through k_tile_dist) with every station's optim_nnghs of month m set to K_m: the
    smoothed bandwidth (a weighted mean rounded half-even) is K_m in every cell.  The fp64 builds (own size; per element
    with TWX_FLAG_NO_HOST_SYNC) give the oracle's status, ninvalid, f4 normals / SE and daily values; the fast build is
    within 1e-5 degC with the same status and ninvalid."""
    from topowx_amd import _lib as lib, stationdb as sdb
    grid, tmin, tmax = golden_case
    dbn = sdb.StationDataWrkChk(_with_bandwidths(tmin.stns, K), "tmin", tmin.days, tmin.var)
    dbx = sdb.StationDataWrkChk(_with_bandwidths(tmax.stns, K), "tmax", tmax.days, tmax.var)
    want = orc.interp_grid(orc.Db(dbn), orc.Db(dbx), orc.params(), grid, daily=True, nthreads=8, rows=ROWS, cols=COLS)
    for name, flags in (("fast", 0), ("f64_all", lib.FLAG_UK_F64_ALL),
                        ("no_sync_f64_all", lib.FLAG_NO_HOST_SYNC | lib.FLAG_UK_F64_ALL)):
        got, t, bw = _grid_run(lib, grid, dbn, dbx, flags)
        assert bw.shape == (144, 12) and np.all(bw == np.array(K)), (name, np.unique(bw))
        if name == "fast":
            assert_fast_oracle(got, want)
        else:
            assert t["uk_f64_solves"] == t["uk_solves"] > 0, (name, t)
            _assert_f4_oracle(got, want, name)


def _tie_twin(tmin, K):
    """A Tmax table that is the Tmin table (same stations, variograms, bandwidths K) with normals and observations
    raised by TIE_DELTA (the observations in f4)."""
    from topowx_amd import stationdb as sdb
    s = _with_bandwidths(tmin.stns, K)
    for m in range(1, 13):
        s[sdb.get_norm_varname(m)] = s[sdb.get_norm_varname(m)] + TIE_DELTA
    obs = (np.asarray(tmin.var, np.float64) + TIE_DELTA).astype(np.float32)
    return sdb.StationDataWrkChk(s, "tmax", tmin.days, obs)


@pytest.mark.parametrize("K", KSETS, ids=lambda K: "K%d" % K[0])
def test_tie_guard_in_every_cell_equals_the_fp64_build(golden_case, orc, K):
    """(c) Tmax = Tmin + 1e-5 degC (normals, f4 observations; grid lst_day = lst_night): Tmax - Tmin of every day of every
    cell is 1e-5 +- ~1e-6 in the oracle (all days valid) and below the guard's 2e-5 in the fast build, so EVERY cell is
    re-kriged by the tie guard, i.e. through twx_f64_coarse_bucket at every size of the K_m set.  The default run then
    equals a TWX_FLAG_UK_F64_ALL run bit for bit in every output (a k-row system in a 64 / 96 / 128 / 160-row kernel
    eliminates identity rows: twx_select.h), and status, ninvalid and the daily values are the oracle's; with
    TWX_FLAG_NO_HOST_SYNC the guard's pass runs in k_uk<7, 2> / k_uk<10, 2> and ninvalid is the oracle's."""
    from topowx_amd import _lib as lib, stationdb as sdb
    grid, tmin, _ = golden_case
    g = dict(grid)
    g["lst_day"] = grid["lst_night"]
    dbn = sdb.StationDataWrkChk(_with_bandwidths(tmin.stns, K), "tmin", tmin.days, tmin.var)
    dbx = _tie_twin(tmin, K)
    want = orc.interp_grid(orc.Db(dbn), orc.Db(dbx), orc.params(), g, daily=True, nthreads=8, rows=ROWS, cols=COLS)
    assert np.all(want["status"] == 0) and np.all(want["ninvalid"] == 0)        # delta leaves every oracle day valid
    ncell = int((np.asarray(grid["mask"])[ROWS, COLS] != 0).sum())
    got, t, bw = _grid_run(lib, g, dbn, dbx, 0)
    assert np.all(bw == np.array(K))
    assert t["tie_cells"] == ncell and t["tie_solves"] == 24 * ncell, t         # the guard fired in every cell
    exact, te, _ = _grid_run(lib, g, dbn, dbx, lib.FLAG_UK_F64_ALL)
    assert te["tie_cells"] == 0 and te["uk_f64_solves"] == te["uk_solves"]
    for k in got:
        assert np.array_equal(got[k], exact[k]), k                              # coarse fp64 build == own-size fp64 build
    assert np.array_equal(got["status"], want["status"])
    for k in ("ninvalid", "daily_tmin", "daily_tmax"):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    for k in ("norm_tmin", "norm_tmax", "se_tmin", "se_tmax"):
        assert np.array_equal(got[k], want[k].astype(np.float32)), k
    nosync, tn, _ = _grid_run(lib, g, dbn, dbx, lib.FLAG_NO_HOST_SYNC)
    assert tn["tie_cells"] == ncell, tn
    assert np.array_equal(nosync["status"], want["status"])
    assert np.array_equal(nosync["ninvalid"], want["ninvalid"])
