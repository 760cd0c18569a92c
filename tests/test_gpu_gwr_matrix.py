"""The GWR hat rows and the daily sums built on them (twx_daily.h: k_gwr_z, k_gwr_z_cell, k_perm, k_tile_uidx, k_daily_tile,
k_daily_tile_gather, k_daily_grid, k_daily_points) at every bandwidth, on every path, against the oracle and the 40-digit
arbiter (oracle/arbiter.py gwr_hat).  In this module ka is a cell's GWR bandwidth of one month.  A kernel that is wrong at one
edge of the 16-lane walk (r = tr + 16 s, TWX_GZ_SLOTS = 10), of the 64-lane loops of k_perm / k_tile_uidx, at ka = 152
(s_d[ka]) or at the table's capacity (TWX_UROWS = 208) fails one of these tests:

(a) point mode (k_gwr_z, k_perm, k_daily_points, k_xval_stats): EVERY ka from 6 to 152 in one call, Tmin and Tmax, within
    max(1e-10, 100 x e_k) degC of the arbiter's series (e_k: the fp64 oracle's own distance from the arbiter at that ka,
    tests/gwr_cases.py); the statistics of gwr_xval_points from the same series; the failure statuses above 152; a failing
    point among the 147; interp_points on the 64 cells of a tile whose ka differ from cell to cell;
(b) grid mode (k_gwr_z_cell, k_tile_uidx, k_daily_tile) with every station's optim_nnghs_anom of month m set to a constant: three
    pairs of sets covering every slot edge, kp (the cell's largest bandwidth) differing between Tmin and Tmax in both
    directions (the kc = min(kpn, kpx) loop of daily_value2 and both tails);
(c) grid mode with bandwidths that vary inside a tile (the table's zero-weight rows, k_tile_uidx's union of unequal lists);
(d) grid mode on a station lattice that puts the union of a tile-month's neighbourhoods at 196 .. 218 rows: tile-months that
    walk a full 208-row table (dt_value4's last chunk and its prefetch clamp), tile-months one row over (nurow = -1: they
    gather) and tile-months where only one variable fits (nurow2), side by side in one launch.
Each grid case runs the fp64 build and the default build against the oracle's grid and TWX_FLAG_DAILY_GATHER,
TWX_FLAG_OBS_ADDR64, TWX_FLAG_FIX_FULL, 4 x 4 tiles (tile_cells = 4) and the one-variable requests (k_daily_grid) against the
default run: "which path a tile-month takes does not show in any output" (include/twx.h).

Measured on gfx950 (the tests print these).  Point mode (k_gwr_z), worst |GPU - arbiter| over a month's series: Tmin 2.6e-12
degC at ka = 7, Tmax 4.2e-13 at ka = 6; the oracle's own worst is 6.9e-13 at ka = 8 (Tmin) and 2.0e-13 at ka = 12 (Tmax),
1.4e-14 from ka = 10 up.  gwr_xval_points against numpy on the arbiter's series: bias 2.1e-13, mae 5.9e-13, r2 2.6e-14.
interp_points on the tile of unequal ka: normals and daily values within 7.1e-7 degC of the oracle, SE within 1.0e-7 (the fast
kriging build).  Grid mode (k_gwr_z_cell and the daily kernels; its outputs are int16 and f4, so its distance from the arbiter
is counted in packed values, through the oracle, which is within 6.9e-13 degC of the arbiter), all five cases: the fp64 build gives the oracle's status,
ninvalid, f4 normals / SE and ALL 2 x 420 864 int16 days; the default build is within 2.4e-6 degC in normals / SE and has 10
.. 29 days of 841 728 off by one; gather, 64-bit gather, 4 x 4 tiles, the full fixer and the one-variable requests equal the
default run wherever the test asks.  No kernel needed a fix."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

import gwr_cases as gc  # noqa: E402
from grid_bars import assert_f4_oracle, assert_fast_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F64_BAR = 1e-10                                              # degC: fp64 arithmetic against 40 digits
MARGIN = 100.0                                               # the same formula in a different, equally stable order (README)
TOL = 1e-4                                                   # degC (test_gpu_parity.py)
CELL_RANGE = 6                                               # TWX_CELL_RANGE
OBS_STATION = 17                                             # gwr_xval_points: the station whose observations are the truth
MIXED_TILE = 1                                               # the window's tile that holds the west / east boundary of GRADED


def _var(lib, var):
    return lib.TMIN if var == "tmin" else lib.TMAX


@pytest.fixture(scope="module")
def every_k(orc, golden_case):
    """Oracle and arbiter series of one point per ka, both variables, once for the module."""
    grid, tmin, tmax = golden_case
    return {"tmin": gc.every_k_series(orc, grid, tmin, "tmin"), "tmax": gc.every_k_series(orc, grid, tmax, "tmax")}


def _point_ctx(lib, golden_case, var):
    grid, tmin, tmax = golden_case
    ctx = lib.Context()
    ctx.set_stations(_var(lib, var), tmin if var == "tmin" else tmax)
    return ctx


def _pts(ctx, grid, cells, var):
    r, c = cells[:, 0], cells[:, 1]
    return ctx.make_pts(grid["lon"][c], grid["lat"][r], grid["elev"][r, c], grid["tdi"][r, c], grid[gc.lst_key(var)][:, r, c].T)


# ---- (a) point mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", ["tmin", "tmax"])
def test_point_mode_every_bandwidth_against_the_arbiter(every_k, golden_case, var):
    """Every ka from 6 to 152 in ONE gwr_points call (pt_norm = 0): status 0, used == ka and the series within
    max(1e-10, 100 x e_k) degC of the arbiter's; every failing ka is reported at once."""
    from topowx_amd import _lib as lib
    s, grid = every_k[var], golden_case[0]
    assert np.all(s["rc"] == 0) and np.all(s["e_k"] <= F64_BAR), "the oracle itself (tests/test_oracle_gwr.py)"
    ctx = _point_ctx(lib, golden_case, var)
    out, used, st = ctx.gwr_points(_var(lib, var), _pts(ctx, grid, s["cells"], var), 0.0, s["mths"], nnghs=s["ks"])
    ctx.close()
    err = np.array([np.abs(out[i, :a.size] - a).max() for i, a in enumerate(s["arbiter"])])
    bar = np.maximum(F64_BAR, MARGIN * s["e_k"])
    print("%s point mode: worst |GPU - arbiter| %.3g degC at ka = %d (oracle's own worst %.3g at ka = %d)"
          % (var, np.nanmax(err), s["ks"][np.nanargmax(err)], s["e_k"].max(), s["ks"][s["e_k"].argmax()]))
    bad = np.nonzero((st != 0) | (used != s["ks"]) | ~(err <= bar))[0]
    assert bad.size == 0, (var, "ka =", s["ks"][bad].tolist(), "status", st[bad].tolist(), err[bad].tolist(), bar[bad].tolist())


def test_xval_statistics_from_the_arbiter_series(every_k, golden_case):
    """gwr_xval_points on the same points: bias / mae / r2 against station OBS_STATION's observations, computed in numpy from
    the arbiter's series (bars of test_xval_tair_anom_vs_executed_reference: 1e-4, 1e-4, 1e-6)."""
    from topowx_amd import _lib as lib
    s, grid = every_k["tmin"], golden_case[0]
    db = s["db"]
    pn = db.cols["norm"][s["mths"] - 1, OBS_STATION]
    ctx = _point_ctx(lib, golden_case, "tmin")
    bias, mae, r2, used, st = ctx.gwr_xval_points(lib.TMIN, _pts(ctx, grid, s["cells"], "tmin"), pn, s["mths"], s["ks"], None,
                                                  OBS_STATION, rm_zero_dist=False)
    ctx.close()
    assert np.all(st == 0) and np.array_equal(used, s["ks"])
    want = np.zeros((s["ks"].size, 3))
    for i, a in enumerate(s["arbiter"]):                      # (interp_anom = series - pt_norm = the arbiter's pt_norm = 0 series)
        xa = db.obs[db.day_month == s["mths"][i], OBS_STATION].astype(np.float64) - pn[i]
        want[i] = (a - xa).mean(), np.abs(a - xa).mean(), np.corrcoef(a, xa)[0, 1] ** 2
    d = np.abs(np.column_stack([bias, mae, r2]) - want)
    print("xval statistics, worst |GPU - numpy on the arbiter's series| (bias, mae, r2):", d.max(axis=0).tolist())
    bad = np.nonzero(~((d[:, 0] < 1e-4) & (d[:, 1] < 1e-4) & (d[:, 2] < 1e-6)))[0]
    assert bad.size == 0, ("ka =", s["ks"][bad].tolist(), d[bad].tolist())


def test_bandwidths_above_the_maximum_fail_alone(every_k, golden_case, orc):
    """nnghs = 153 gives TWX_CELL_RANGE and nnghs = 399 (of 400 stations) fails: the maximum is the LIBRARY's (TWX_MAX_NNGHS =
    152: z slots, table rows).  The oracle has no such limit (ORC_MAXK = 512, as the reference has none) and computes both, so
    where the GPU's status reads TWX_CELL_RANGE the oracle's reads 0 -- and 400 of 400 stations is ORC_ERR_FEW_STATIONS there.
    A failing point in the middle of the 147 leaves every other series as it was, bit for bit, and its own at NaN / 0."""
    from topowx_amd import _lib as lib
    s, grid = every_k["tmin"], golden_case[0]
    ctx = _point_ctx(lib, golden_case, "tmin")
    pts = _pts(ctx, grid, s["cells"], "tmin")
    out, used, st = ctx.gwr_points(lib.TMIN, pts[:4], 0.0, s["mths"][:4], nnghs=[153, 399, 153, 152])
    assert st.tolist() == [CELL_RANGE, st[1], CELL_RANGE, 0] and st[1] != 0, st
    pt = gc.oracle_pt(orc, grid, *s["cells"][0], "tmin")
    assert [orc.gwr_mth(s["db"], orc.params(), pt, 0.0, int(s["mths"][0]), nnghs=k)[0] for k in (153, 399, 400)] == [0, 0, 1]
    base, _, st0 = ctx.gwr_points(lib.TMIN, pts, 0.0, s["mths"], nnghs=s["ks"])
    ks = s["ks"].copy()
    mid = ks.size // 2
    ks[mid] = 153
    got, used, st = ctx.gwr_points(lib.TMIN, pts, 0.0, s["mths"], nnghs=ks)
    ctx.close()
    others = np.arange(ks.size) != mid
    assert np.all(st0 == 0) and st[mid] == CELL_RANGE and np.all(st[others] == 0)
    assert np.array_equal(got[others], base[others], equal_nan=True)
    assert not np.isfinite(got[mid]).any() or np.all(np.nan_to_num(got[mid]) == 0.0)


@pytest.mark.parametrize("var", ["tmin", "tmax"])
def test_interp_points_on_a_tile_of_unequal_bandwidths(golden_case, orc, var):
    """interp_points(daily=True) on the 64 cells of the window's tile that holds the west / east boundary of the GRADED table:
    the twelve months of a point, and neighbouring points, have different ka.  Against orc.interp at the bars
    test_interp_points_golden_and_xval uses against its goldens (1e-4 degC)."""
    from topowx_amd import _lib as lib
    grid, tmin, tmax = golden_case
    da = tmin if var == "tmin" else tmax
    table = gc.with_gwr_bandwidths(da, var, gc.graded_bandwidths(da, grid, var))
    rr, cc = gc.window_cells()
    cells = np.column_stack([gc.tile_view(rr)[MIXED_TILE], gc.tile_view(cc)[MIXED_TILE]])
    db, prm = orc.Db(table), orc.params()
    ka = gc.tile_view(gc.ka_table(orc, db, grid, var))[MIXED_TILE]
    assert max(np.unique(ka[:, m]).size for m in range(12)) >= 4 and min(np.unique(k).size for k in ka) >= 6, "precondition"
    ctx = lib.Context()
    ctx.set_stations(_var(lib, var), table)
    d, norms, se, st = ctx.interp_points(_var(lib, var), _pts(ctx, grid, cells, var))
    ctx.close()
    assert np.all(st == 0)
    worst = np.zeros(3)
    for i, (r, c) in enumerate(cells):
        rc, wd, wn, ws = orc.interp(db, prm, gc.oracle_pt(orc, grid, r, c, var))
        assert rc == 0
        e = np.array([np.abs(norms[i] - wn).max(), np.abs(se[i] - ws).max(), np.abs(d[i] - wd).max()])
        assert np.all(e < TOL), (r, c, e.tolist())
        worst = np.maximum(worst, e)
    print("%s interp_points, worst |GPU - oracle| (normals, SE, daily):" % var, worst.tolist())


# ---- (b) - (d) grid mode -----------------------------------------------------------------------------------------------------
class _GridCase(object):
    """The two station tables of a case, the oracle's grid on the window, what the case's preconditions need -- and the GPU
    runs, each made once."""

    def __init__(self, name, orc, golden_case):
        grid, tmin, tmax = golden_case
        self.name, self.grid, self.pre = name, grid, {}
        if name in gc.CONSTANT_CASES:
            Kn, Kx = gc.CONSTANT_CASES[name]
            self.dbn, self.dbx = gc.with_gwr_bandwidths(tmin, "tmin", Kn), gc.with_gwr_bandwidths(tmax, "tmax", Kx)
        elif name == "graded":
            self.dbn = gc.with_gwr_bandwidths(tmin, "tmin", gc.graded_bandwidths(tmin, grid, "tmin"))
            self.dbx = gc.with_gwr_bandwidths(tmax, "tmax", gc.graded_bandwidths(tmax, grid, "tmax"))
            self.pre["ka"] = gc.ka_table(orc, orc.Db(self.dbn), grid, "tmin")
        else:
            self.dbn, self.dbx = gc.lattice_table(tmin, grid, "tmin"), gc.lattice_table(tmax, grid, "tmax")
            for var, t in (("tmin", self.dbn), ("tmax", self.dbx)):
                db = orc.Db(t)
                self.pre["union_" + var] = gc.tile_unions(orc, db, grid, gc.ka_table(orc, db, grid, var))
        self.want = orc.interp_grid(orc.Db(self.dbn), orc.Db(self.dbx), orc.params(), grid, daily=True, nthreads=8,
                                    rows=gc.ROWS, cols=gc.COLS)
        self.runs = {}

    def check_preconditions(self):
        """What the case's recipe was checked to give, on the oracle's output alone: a drifted generator fails here."""
        w, name = self.want, self.name
        assert w["status"].shape == (16, 24) and np.all(w["status"] == 0), name
        for k in ("daily_tmin", "daily_tmax"):
            assert np.abs(w[k].astype(int)).max() < 32000, (name, k)
        if name == "AB":
            assert w["ninvalid"].max() > 0                    # the fixer's lists run with small bandwidths too
        if name == "graded":
            ka = self.pre["ka"]
            u = np.unique(ka)
            assert u.size >= 90, u.size
            kt = gc.tile_view(ka)
            assert max(np.unique(kt[t, :, m]).size for t in range(kt.shape[0]) for m in range(12)) >= 4
            edges = [33] + [e + d for e in (48, 64, 80, 96, 112, 128) for d in (-1, 0, 1)]   # both sides of every slot edge
            assert u.min() < 32 and all(e in u for e in edges), u.tolist()
        if name == "capacity":
            un, ux = self.pre["union_tmin"], self.pre["union_tmax"]
            for u in (un, ux):                                # a full (or nearly full) table, and one row over, per variable
                assert ((u >= 205) & (u <= gc.UROWS)).any() and (u > gc.UROWS).any(), u.tolist()
                assert (u == gc.UROWS).any() and (u == gc.UROWS + 1).any(), u.tolist()
            both = (un <= gc.UROWS) & (ux <= gc.UROWS)        # a (tile, month) walks the tables only when BOTH unions fit
            assert both.any() and (~both).any() and ((un <= gc.UROWS) ^ (ux <= gc.UROWS)).any()

    def run(self, flags=0, tile_cells=0, variables=("tmin", "tmax")):
        from topowx_amd import _lib as lib
        key = (flags, tile_cells, variables)
        if key not in self.runs:
            ctx = lib.Context(flags=flags, tile_cells=tile_cells)
            ctx.set_stations(lib.TMIN, self.dbn)
            ctx.set_stations(lib.TMAX, self.dbx)
            got = ctx.interp_grid(self.grid, variables=variables, daily=True, rows=gc.ROWS, cols=gc.COLS)
            t = ctx.timing()
            ctx.close()
            self.runs[key] = (got, t)
        return self.runs[key]


@pytest.fixture(scope="module", params=list(gc.CONSTANT_CASES) + ["graded", "capacity"])
def case(request, orc, golden_case):
    return _GridCase(request.param, orc, golden_case)


def test_grid_fp64_build_equals_the_oracle(case):
    """TWX_FLAG_UK_F64_ALL: status, ninvalid, the f4 normals and SE equal the oracle's; fewer than 2e-6 of the daily values
    differ (_assert_f4_oracle of test_gpu_kernel_matrix.py)."""
    from topowx_amd import _lib as lib
    case.check_preconditions()
    got, t = case.run(flags=lib.FLAG_UK_F64_ALL)
    assert t["uk_f64_solves"] == t["uk_solves"] > 0, t
    print("%s fp64 build: int16 days other than the oracle's: %d + %d of %d" % (
        case.name, (got["daily_tmin"] != case.want["daily_tmin"]).sum(), (got["daily_tmax"] != case.want["daily_tmax"]).sum(),
        got["daily_tmin"].size))
    assert_f4_oracle(got, case.want, case.name)


def test_grid_default_build_against_the_oracle(case):
    """The default build by the fast branch of test_grid_mode_constant_bandwidths: the oracle's status and ninvalid, normals
    and SE within 1e-5 degC, packed daily values within 1."""
    case.check_preconditions()
    got, want = case.run()[0], case.want
    print("%s default build: normals / SE within %.2g degC; int16 days off by one: %d + %d of %d" % (
        case.name, max(np.abs(got[k].astype(np.float64) - want[k]).max() for k in ("norm_tmin", "norm_tmax", "se_tmin", "se_tmax")),
        (got["daily_tmin"] != want["daily_tmin"]).sum(), (got["daily_tmax"] != want["daily_tmax"]).sum(), got["daily_tmin"].size))
    assert_fast_oracle(got, want)


def test_grid_gather_paths_equal_the_table_walk(case):
    """TWX_FLAG_DAILY_GATHER (every tile-month gathers, 32-bit offsets), TWX_FLAG_OBS_ADDR64 (64-bit) and 4 x 4 tiles equal the
    default run in EVERY output on all cells.  In the capacity case the default run has tile-months that walk a full
    208-row table, tile-months of 209 rows that gather and tile-months where one variable fits and the other does not, side
    by side."""
    from topowx_amd import _lib as lib
    case.check_preconditions()
    base = case.run()[0]
    assert np.all(base["status"] == 0)
    for what, kw in (("gather", dict(flags=lib.FLAG_DAILY_GATHER)), ("addr64", dict(flags=lib.FLAG_OBS_ADDR64)),
                     ("tile_cells=4", dict(tile_cells=4))):
        other = case.run(**kw)[0]
        for k in base:
            assert np.array_equal(base[k], other[k]), (case.name, what, k, int((base[k] != other[k]).sum()))


def test_grid_full_fixer_equals_the_sparse_fixer(case):
    """TWX_FLAG_FIX_FULL: the same status, fixed days and packed int16 values; the recomputed f4 normals may differ in the last
    bit of the f8 sum (4e-6: test_fixer_limits_of_the_sparse_path_vs_oracle)."""
    from topowx_amd import _lib as lib
    case.check_preconditions()
    base, full = case.run()[0], case.run(flags=lib.FLAG_FIX_FULL)[0]
    for k in ("daily_tmin", "daily_tmax", "ninvalid", "status"):
        assert np.array_equal(base[k], full[k]), (case.name, k)
    for k in ("norm_tmin", "norm_tmax"):
        assert np.abs(base[k].astype(np.float64) - full[k]).max() <= 4e-6, (case.name, k)
    for k in ("se_tmin", "se_tmax"):
        assert np.array_equal(base[k], full[k]), (case.name, k)


def test_grid_single_variable_requests_equal_the_two_variable_run(case):
    """Tmin-only and Tmax-only requests (k_daily_grid: gathers through perm) give the two-variable run's packed days on the
    cells the fixer left alone, and its kriged normals and SE wherever the fixer recomputed none."""
    case.check_preconditions()
    both = case.run()[0]
    clean = both["ninvalid"] == 0
    assert clean.any()
    for v in ("tmin", "tmax"):
        one = case.run(variables=(v,))[0]
        assert np.array_equal(one["status"], both["status"])
        assert np.array_equal(one["daily_" + v][:, clean], both["daily_" + v][:, clean]), (case.name, v)
        assert np.array_equal(one["se_" + v], both["se_" + v]), (case.name, v)
        assert np.array_equal(one["norm_" + v][:, clean], both["norm_" + v][:, clean]), (case.name, v)
