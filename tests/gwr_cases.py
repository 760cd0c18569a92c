"""Inputs of the GWR tests (tests/test_oracle_gwr.py, tests/test_gpu_gwr_matrix.py): everything derives from the golden case
(100 x 100 grid, 400 stations, 1096 days) with fixed seeds.

* every_k_series: one point per GWR bandwidth ka = 6 .. 152 (cells spread over the mask, month 1 + i % 12, as
  test_gpu_kernel_matrix.py picks its points), the oracle's series of that month (orc.gwr_mth, pt_norm = 0) and the series
  from the 40-digit hat row (oracle/arbiter.py gwr_hat) summed in numpy float64 over the same neighbours and weights.
* with_gwr_bandwidths / graded_bandwidths / lattice_table: station tables whose optim_nnghs_anomMM are per-month constants,
  differ west and east of the window (so that the smoothed ka varies inside a tile), or whose stations sit on a jittered
  lattice under the window (so that the union of a tile-month's neighbourhoods lands on both sides of TWX_UROWS = 208).
* ka_table / tile_unions: the oracle's own smoothed bandwidths and the size of the union of a tile-month's neighbour lists.
"""
import numpy as np

KMIN, KMAX = 6, 152                                          # TWX_MAX_NNGHS (include/twx.h)
UROWS = 208                                                  # TWX_UROWS (twx_daily.h)
ROWS, COLS = slice(40, 56), slice(24, 48)                    # 2 x 3 whole 8 x 8 tiles
TS = 8

# per-month constants: every edge of the 16-lane slots (r = tr + 16 s), of the 64-lane loops and the maximum
KA_A = (8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)
KA_B = (64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127)
KA_C = (128, 129, 143, 144, 145, 151, 152, 10, 12, 24, 56, 120)
CONSTANT_CASES = {"AB": (KA_A, KA_B), "BC": (KA_B, KA_C), "CA": (KA_C, KA_A)}      # (Tmin set, Tmax set)
# (lo, hi) by month: stations west of the window's mean longitude get lo, the others hi (Tmax: reverse month order)
GRADED = ((6, 30), (6, 60), (10, 80), (20, 100), (30, 120), (40, 140), (60, 152), (80, 152), (100, 152), (120, 152),
          (6, 152), (140, 152))
# the table's capacity: GWR bandwidths by month (Tmin; Tmax reversed) on the lattice
CAPACITY_KA = tuple(range(141, 153))
LATTICE_SEED = {"tmin": 11, "tmax": 12}


def lst_key(var):
    return "lst_night" if var == "tmin" else "lst_day"


def every_k_points(grid):
    """(ks, cells, months): one masked-in cell per bandwidth, spread over the grid."""
    ks = np.arange(KMIN, KMAX + 1)
    cells = np.argwhere(np.asarray(grid["mask"]) != 0)
    cells = cells[np.linspace(0, len(cells) - 1, ks.size).astype(int)]
    return ks, cells, 1 + np.arange(ks.size) % 12


def oracle_pt(orc, grid, r, c, var):
    return orc.make_pt(grid["lon"][c], grid["lat"][r], grid["elev"][r, c], grid["tdi"][r, c], grid[lst_key(var)][:, r, c])


def every_k_series(orc, grid, stn_da, var):
    """The oracle's and the arbiter's series of every_k_points for one variable.  Returns a dict: ks, cells, mths, db, rc
    [n] (the oracle's status), oracle / arbiter (lists of [days of the month] arrays, pt_norm = 0), e_k [n] = max |oracle -
    arbiter| in degC, idx (the neighbours, ascending station index)."""
    from oracle import arbiter
    ks, cells, mths = every_k_points(grid)
    db, prm = orc.Db(stn_da), orc.params()
    c = db.cols
    out = dict(ks=ks, cells=cells, mths=mths, db=db, rc=np.zeros(ks.size, int), oracle=[], arbiter=[], idx=[],
               e_k=np.full(ks.size, np.inf))
    for i, (row, col) in enumerate(cells):
        k, m = int(ks[i]), int(mths[i])
        pt = oracle_pt(orc, grid, row, col, var)
        rc, series, used, _, idx = orc.gwr_mth(db, prm, pt, 0.0, m, nnghs=k)
        rs, sidx, _, wgt = orc.select(db, pt.lat, pt.lon, k)
        assert rs == 0 and used == k and np.array_equal(sidx, idx), (k, rc, rs, used)   # the same neighbours on both sides
        X5 = np.column_stack([c["lon"][idx], c["lat"][idx], c["elev"][idx], c["tdi"][idx], c["lst"][m - 1, idx]])
        z = np.array(arbiter.gwr_hat(X5, wgt, [pt.lon, pt.lat, pt.elev, pt.tdi, pt.lst[m - 1]]))
        obs = db.obs[db.day_month == m][:, idx].astype(np.float64)
        arb = (obs - c["norm"][m - 1, idx]) @ z
        out["rc"][i] = rc
        out["oracle"].append(series)
        out["arbiter"].append(arb)
        out["idx"].append(idx)
        out["e_k"][i] = float(np.abs(series - arb).max())
    return out


# ---- station tables for grid mode ------------------------------------------------------------------------------------------
def _table(stn_da, var, stns):
    from topowx_amd import stationdb as sdb
    return sdb.StationDataWrkChk(stns, var, stn_da.days, stn_da.var)


def with_gwr_bandwidths(stn_da, var, K):
    """The table with optim_nnghs_anomMM of month m set to K[m - 1] (a constant or one value per station); the kriging
    bandwidths stay as they are."""
    from topowx_amd import stationdb as sdb
    s = stn_da.stns.copy()
    for m in range(1, 13):
        s[sdb.get_optim_anom_varname(m)] = K[m - 1]
    return _table(stn_da, var, s)


def graded_bandwidths(stn_da, grid, var):
    """GRADED as per-station values: lo west of the window's mean longitude, hi elsewhere; Tmax in reverse month order."""
    from topowx_amd import stationdb as sdb
    west = stn_da.stns[sdb.LON] < np.asarray(grid["lon"])[COLS].mean()
    pairs = GRADED if var == "tmin" else GRADED[::-1]
    return [np.where(west, float(lo), float(hi)) for lo, hi in pairs]


def lattice_table(stn_da, grid, var):
    """The good stations re-positioned on a jittered 20 x 20 lattice centred on the window, spacing 3 cell heights, GWR
    bandwidths CAPACITY_KA (Tmax reversed); every other column and the observations stay as they are."""
    from topowx_amd import stationdb as sdb
    s = stn_da.stns.copy()
    good = np.nonzero(np.isnan(s[sdb.BAD]))[0]
    assert good.size == 400
    lat, lon = np.asarray(grid["lat"], np.float64), np.asarray(grid["lon"], np.float64)
    dlat = abs(lat[1] - lat[0])
    cy, cx = lat[ROWS].mean(), lon[COLS].mean()
    rng = np.random.default_rng(LATTICE_SEED[var])
    jy = rng.uniform(-.25, .25, 400)                          # latitude jitter first, then longitude
    jx = rng.uniform(-.25, .25, 400)
    iy, ix = np.divmod(np.arange(400), 20)
    s[sdb.LAT][good] = cy + (iy - 9.5 + jy) * 3 * dlat
    s[sdb.LON][good] = cx + (ix - 9.5 + jx) * 3 * dlat / np.cos(np.radians(cy))
    K = CAPACITY_KA if var == "tmin" else CAPACITY_KA[::-1]
    for m in range(1, 13):
        s[sdb.get_optim_anom_varname(m)] = K[m - 1]
    return _table(stn_da, var, s)


def window_cells():
    rr, cc = np.meshgrid(np.arange(ROWS.start, ROWS.stop), np.arange(COLS.start, COLS.stop), indexing="ij")
    return rr, cc


def ka_table(orc, db, grid, var):
    """The oracle's smoothed GWR bandwidth of every (cell of the window, month): [nrow, ncol, 12] (orc.gwr_mth, nnghs = 0)."""
    rr, cc = window_cells()
    prm = orc.params()
    ka = np.zeros(rr.shape + (12,), int)
    for i in np.ndindex(rr.shape):
        pt = oracle_pt(orc, grid, rr[i], cc[i], var)
        for m in range(1, 13):
            rc, _, used, _, _ = orc.gwr_mth(db, prm, pt, 0.0, m)
            assert rc == 0, (i, m, rc)
            ka[i + (m - 1,)] = used
    return ka


def tile_view(a):
    """[nrow, ncol, ...] of the window -> [ntile, 64, ...] (8 x 8 tiles, row-major)."""
    ny, nx = a.shape[0] // TS, a.shape[1] // TS
    t = a.reshape((ny, TS, nx, TS) + a.shape[2:])
    return np.moveaxis(t, 2, 1).reshape((ny * nx, TS * TS) + a.shape[2:])


def tile_unions(orc, db, grid, ka):
    """Rows of every tile-month's table: the size of the union of the cells' GWR neighbourhoods, from the oracle's own lists
    (orc.nearest(..., 153)[:ka]).  ka [nrow, ncol, 12] -> [ntile, 12]."""
    rr, cc = window_cells()
    near = np.zeros(rr.shape + (KMAX + 1,), np.int64)
    for i in np.ndindex(rr.shape):
        idx, _ = orc.nearest(db, grid["lat"][rr[i]], grid["lon"][cc[i]], KMAX + 1)
        near[i] = idx
    nt, kt = tile_view(near), tile_view(ka)
    un = np.zeros((nt.shape[0], 12), int)
    for t in range(nt.shape[0]):
        for m in range(12):
            un[t, m] = np.unique(np.concatenate([nt[t, ci, :kt[t, ci, m]] for ci in range(TS * TS)])).size
    return un
