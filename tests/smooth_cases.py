"""Inputs and restatements of the smoothing tests (tests/test_oracle_smooth.py, tests/test_gpu_smooth.py): what k_select
(topowx_amd/csrc/twx_select.h) makes of the neighbours' station parameters -- the kriging bandwidth kk[m], the GWR bandwidth
ka[m] and the variogram (nug, psill, rng)[m] of every month, each a bisquare-weighted mean over the neighbours whose field is
finite (interp_tair.py:821-835, :245-259, :837-851), and the month-ordered status (interp_tair.py:429-437) -- on station
tables whose fields are NaN raggedly: by station, month and family (optim_nnghs, optim_nnghs_anom, vario_nug with its psill
and range).  Everything derives from the golden case (100 x 100 grid, 400 stations, 1096 days) with fixed seeds.

* PATTERNS: the named tables (``case(name, golden_case)``); CATCHES: the mutants each of them must tell from the truth.
* ``primitives_numpy``: a plain numpy restatement on fp64 -- haversine ranks with ties in table order, sums taken one addend
  after the other in station order, as the oracle takes them -- and the MUTANTS of it that a wrong kernel would compute.
* ``primitives_oracle``: the same quantities from the oracle's own C functions (orc_nearest, orc_select, orc_smooth_nnghs,
  orc_smooth_vario).
* ``walk``: the reference's month loop (krig(m), then gwr(m); the first failure ends the point) over either.
"""
import numpy as np

MAXK = 152                                                   # TWX_MAX_NNGHS (include/twx.h)
INIT = 100                                                   # init_nnghs
GA = 4                                                       # TWX_SEL_GA: months whose gathers are in flight together
CAND_SMALL = 512                                             # TWX_CAND_SMALL: the longest list of the short-list launch
TS = 8                                                       # cells per tile side
WIN = (slice(35, 59), slice(29, 53))                         # 24 x 24, its origin on no tile edge of the golden grid
DWIN = (slice(35, 47), slice(29, 41))                        # 12 x 12 (one whole tile and three partial ones): the daily runs
BLOCK_A = (slice(0, 6), slice(0, 6))                         # window-relative: the chosen cells of slot1 / beyond / dead / one
BLOCK_C = (slice(16, 22), slice(16, 22))                     # dead: the cells whose variogram fails (Tmax)
K_EDGES = (63, 64, 65, 100, 128, 129)                        # init_nnghs at the edges of the kernel's 64-rank slots
ONE_MONTHS = (2, 6, 10)                                      # one: months (0-based) with a single finite neighbour ...
ONE_VALUES = (36.5, 37.5, 80.5)                              # ... whose value is a tie: half to even gives 36, 38, 80
DEAD_OPTIM, DEAD_ANOM, DEAD_NUG = 5, (2, 8), 3               # dead: months (0-based) without a finite neighbour
CLUSTER_BOX = (45.55, 45.85, -110.7, -110.4)                 # (e): test_gpu_stream._cluster_db's box
CLUSTER_WIN = (slice(30, 46), slice(44, 60))

MUTANTS = {
    "M1": "the previous month's sum of weights",
    "M2": "optim_nnghs's finite mask behind optim_nnghs_anom's sum of weights",
    "M3": "optim_nnghs's finite mask behind the variogram's sum of weights",
    "M4": "the ranks >= init_nnghs included",
    "M5": "round half away from zero",
}
PATTERNS = ("indep05", "indep50", "runs", "runs_shift", "slot1", "beyond", "dead", "one", "families")
CATCHES = {"indep05": ("M1", "M2", "M3"), "indep50": ("M1", "M2", "M3"), "runs": ("M1",), "runs_shift": ("M1",),
           "slot1": ("M1",), "beyond": ("M4",), "dead": (), "one": ("M5",), "families": ("M2", "M3")}
_SEED = {name: 4100 + 10 * i for i, name in enumerate(PATTERNS)}

ERR_FEW, ERR_NNGHS, ERR_VARIO, ERR_NUMERIC, ERR_RANGE = 1, 2, 3, 4, 6


def lst_key(var):
    return "lst_night" if var == "tmin" else "lst_day"


def window_cells(win=WIN, block=None):
    """[ncell, 2] (row, col) of the golden grid, row-major; ``block``: window-relative slices."""
    rows, cols = np.arange(win[0].start, win[0].stop), np.arange(win[1].start, win[1].stop)
    if block is not None:
        rows, cols = rows[block[0]], cols[block[1]]
    rr, cc = np.meshgrid(rows, cols, indexing="ij")
    return np.column_stack([rr.ravel(), cc.ravel()])


def point_cells():
    """48 cells of WIN (every 4th row, every 3rd column): the points of the point-mode paths."""
    return window_cells(WIN)[[r * 24 + c for r in range(0, 24, 4) for c in range(0, 24, 3)]]


# ---- tables -------------------------------------------------------------------------------------------------------------------
def _table(stn_da, var, stns):
    from topowx_amd import stationdb as sdb
    return sdb.StationDataWrkChk(stns, var, stn_da.days, stn_da.var)


def _fields(m):
    from topowx_amd import stationdb as sdb
    return (sdb.get_optim_varname(m), sdb.get_optim_anom_varname(m), sdb.get_krigparam_varname(m, sdb.VARIO_NUG),
            sdb.get_krigparam_varname(m, sdb.VARIO_PSILL), sdb.get_krigparam_varname(m, sdb.VARIO_RNG))


def filled(stns, seed):
    """A copy of the table with every smoothing field finite (the generator's out-of-domain stations get values drawn as
    the generator draws them): the patterns decide alone where the NaN are."""
    from topowx_amd import synth
    s = stns.copy()
    rng = np.random.default_rng(seed)
    for m in range(1, 13):
        ko, ka, nug, psill, rg = _fields(m)
        for name, draw in ((ko, lambda k: rng.choice(synth.NNGH_LADDER, k)), (ka, lambda k: rng.choice(synth.NNGH_LADDER, k)),
                           (nug, lambda k: rng.uniform(0.1, 0.6, k)), (psill, lambda k: rng.uniform(0.2, 2.0, k)),
                           (rg, lambda k: rng.uniform(10.0, 80.0, k))):
            nan = np.isnan(s[name])
            s[name][nan] = draw(int(nan.sum()))
    return s


def columns(stns):
    """fp64 columns of a table: lon, lat [n]; optim, anom, nug, psill, rng [12, n]."""
    from topowx_amd import stationdb as sdb
    assert np.all(np.isnan(stns[sdb.BAD]))
    out = {"lon": np.ascontiguousarray(stns[sdb.LON], np.float64), "lat": np.ascontiguousarray(stns[sdb.LAT], np.float64)}
    for i, key in enumerate(("optim", "anom", "nug", "psill", "rng")):
        out[key] = np.ascontiguousarray(np.stack([stns[_fields(m)[i]] for m in range(1, 13)]), np.float64)
    return out


def apply_masks(s, nan_k, nan_a, nan_v):
    """NaN into optim_nnghs / optim_nnghs_anom / the variogram triple where the [12, n] masks say so."""
    for m in range(1, 13):
        ko, ka, nug, psill, rg = _fields(m)
        s[ko][nan_k[m - 1]] = np.nan
        s[ka][nan_a[m - 1]] = np.nan
        for name in (nug, psill, rg):
            s[name][nan_v[m - 1]] = np.nan
    return s


# ---- ranks --------------------------------------------------------------------------------------------------------------------
def hav_km(lon1, lat1, lon2, lat2):
    """util_geo.py:24-40 in the oracle's operation order (orc_grt_circle_dist)."""
    f = 0.017453292519943295
    la1, la2, lo1, lo2 = lat1 * f, lat2 * f, lon1 * f, lon2 * f
    s1, s2 = np.sin((la1 - la2) / 2), np.sin((lo1 - lo2) / 2)
    return 6371.009 * (2 * np.arcsin(np.sqrt(s1 * s1 + np.cos(la1) * np.cos(la2) * (s2 * s2))))


class Ranker(object):
    """All stations of one coordinate set by distance from a cell, ties in table order; cached by cell."""

    def __init__(self, lon, lat, grid):
        self.lon, self.lat, self.grid, self.cache = lon, lat, grid, {}

    def __call__(self, r, c):
        key = (int(r), int(c))
        if key not in self.cache:
            d = hav_km(self.grid["lon"][c], self.grid["lat"][r], self.lon, self.lat)
            order = np.argsort(d, kind="stable")
            self.cache[key] = (order, d[order])
        return self.cache[key]

    def union(self, cells, k):
        return np.unique(np.concatenate([self(r, c)[0][:k] for r, c in cells]))

    def common(self, cells, lo, hi):
        """Stations that every one of the cells ranks lo .. hi - 1."""
        sets = [set(self(r, c)[0][lo:hi].tolist()) for r, c in cells]
        return np.array(sorted(set.intersection(*sets)), np.int64)


def ksel_of(cols, init=INIT):
    """orc pick_ksel / the library's: one more than the largest bandwidth the table or init_nnghs can ask for."""
    km = int(np.rint(max(np.nanmax(cols["optim"]), np.nanmax(cols["anom"]))))
    return min(max(km, init), MAXK) + 1


# ---- the restatement and its mutants ------------------------------------------------------------------------------------------
def _seq_sum(a):
    """Row sums taken one addend after the other (np.sum adds pairwise)."""
    return np.cumsum(a, axis=-1)[..., -1] if a.shape[-1] else np.zeros(a.shape[:-1])


def _select(order, dist, nnear, k, upto=None):
    """orc_select / station_select.py:121-192: (status, stations ascending, weights); ``upto``: ranks kept (M4)."""
    if k < 0 or k >= nnear:
        return ERR_FEW, None, None
    dbw = dist[k]
    if not dbw > 0.0:
        return ERR_NUMERIC, None, None
    kk = k if upto is None else upto
    pos = np.argsort(order[:kk], kind="stable")
    r = dist[:kk][pos] / dbw
    t = 1.0 - r * r
    return 0, order[:kk][pos], t * t


def _round(x, mutant):
    return np.floor(x + 0.5) if mutant == "M5" else np.rint(x)


def primitives_numpy(cols, order, dist, init=INIT, mutant=None):
    """One point's smoothing, every month on its own: dict of rk [12] (status of the month's kriging selection: bandwidth,
    range, Select(k), variogram -- the first that fails), k [12], vario [12, 3], ra [12] (the GWR selection's) and ka [12]."""
    n = order.size
    nnear = min(n, ksel_of(cols, init))
    out = dict(rk=np.zeros(12, int), k=np.zeros(12, int), vario=np.zeros((12, 3)), ra=np.zeros(12, int), ka=np.zeros(12, int))
    rc, idx, w = _select(order, dist, nnear, init, nnear if mutant == "M4" else None)
    if rc:
        out["rk"][:] = rc
        out["ra"][:] = rc
        return out
    fin_k = np.isfinite(cols["optim"][:, idx])
    for key, rkey, kkey in (("optim", "rk", "k"), ("anom", "ra", "ka")):
        f = cols[key][:, idx]
        fin = np.isfinite(f)
        num = _seq_sum(np.where(fin, f * w, 0.0))
        den = _seq_sum(np.where(fin_k if (mutant == "M2" and key == "anom") else fin, w, 0.0))
        if mutant == "M1":
            den = np.concatenate([den[:1], den[:-1]])
        for m in range(12):
            if not fin[m].any():
                out[rkey][m] = ERR_NNGHS
            elif not den[m] != 0.0:
                out[rkey][m] = ERR_NUMERIC
            else:
                k = int(_round(num[m] / den[m], mutant))
                out[kkey][m] = k
                if k < 1 or k > MAXK:
                    out[rkey][m] = ERR_RANGE
                else:
                    out[rkey][m] = _select(order, dist, nnear, k)[0]
    for m in range(12):
        if out["rk"][m]:
            continue
        _, idx, w = _select(order, dist, nnear, out["k"][m])
        nug = cols["nug"][m, idx]
        fin = np.isfinite(nug)
        den = _seq_sum(np.where(np.isfinite(cols["optim"][m, idx]) if mutant == "M3" else fin, w, 0.0))
        if not fin.any():
            out["rk"][m] = ERR_VARIO
        elif not den != 0.0:
            out["rk"][m] = ERR_NUMERIC
        else:
            out["vario"][m] = [_seq_sum(np.where(fin, cols[key][m, idx] * w, 0.0)) / den for key in ("nug", "psill", "rng")]
    return out


def primitives_oracle(orc, db, prm, lon, lat):
    """primitives_numpy's quantities from the oracle's C functions (the steps of krig_with_near / gwr_with_near before the
    solves, twx_oracle.c)."""
    import ctypes as C
    L = orc.lib()
    c = db.cols
    ksel = ksel_of({"optim": c["optim_nnghs"], "anom": c["optim_nnghs_anom"]}, prm.init_nnghs)
    nidx, ndist = orc.nearest(db, lat, lon, ksel)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    idx, dist, wgt = np.zeros(MAXK + 1, np.int32), np.zeros(MAXK + 1), np.zeros(MAXK + 1)

    def select(k):
        if k > MAXK:
            return ERR_RANGE
        return L.orc_select(nidx.ctypes.data_as(ip), ndist.ctypes.data_as(dp), C.c_int64(nidx.size), C.c_int(k),
                            idx.ctypes.data_as(ip), dist.ctypes.data_as(dp), wgt.ctypes.data_as(dp))
    out = dict(rk=np.zeros(12, int), k=np.zeros(12, int), vario=np.zeros((12, 3)), ra=np.zeros(12, int), ka=np.zeros(12, int))
    for key, rkey, kkey in (("optim_nnghs", "rk", "k"), ("optim_nnghs_anom", "ra", "ka")):
        rc0 = select(prm.init_nnghs)
        i0, w0 = idx[:prm.init_nnghs].copy(), wgt[:prm.init_nnghs].copy()
        for m in range(12):
            rc, k = (rc0, 0) if rc0 else orc.smooth_nnghs(c[key][m], i0, w0)
            if not rc and (k < 1 or k > MAXK):
                rc = ERR_RANGE
            if not rc:
                rc = select(k)
            if not rc and key == "optim_nnghs":
                rc, out["vario"][m] = orc.smooth_vario(c["vario_nug"][m], c["vario_psill"][m], c["vario_rng"][m], idx[:k], wgt[:k])
            out[rkey][m], out[kkey][m] = rc, k
    return out


def walk(p, daily):
    """interp_tair.py:429-437: krig(m), then (daily) gwr(m), month by month; the first failure ends the point.  Returns
    (kk [12], ka [12], status): kk[m] is set for every month whose kriging the loop reaches and whose selection holds."""
    kk, ka, status = np.zeros(12, int), np.zeros(12, int), 0
    for m in range(12):
        if not status:
            status = int(p["rk"][m])
        if not status:
            kk[m] = p["k"][m]
        if daily and not status:
            status = int(p["ra"][m])
            if not status:
                ka[m] = p["ka"][m]
    return kk, ka, status


# ---- the patterns -------------------------------------------------------------------------------------------------------------
def _months_that_differ(rng, nst, p=0.5):
    """[12, nst] masks, each month's different from the one before."""
    out = np.zeros((12, nst), bool)
    for m in range(12):
        out[m] = rng.random(nst) < p
        while m and np.array_equal(out[m], out[m - 1]):
            out[m] = rng.random(nst) < p
    return out


def _pattern_masks(name, var, s, rk):
    """The NaN masks (optim, anom, variogram) [12, n] of a pattern for one variable; ``s`` (the filled table) may get values."""
    n = s.size
    rng = np.random.default_rng(_SEED["runs" if name == "runs_shift" else name] + (var == "tmax"))
    nan_k, nan_a, nan_v = (np.zeros((12, n), bool) for _ in range(3))
    block = window_cells(WIN, BLOCK_A)
    if name in ("indep05", "indep50"):
        p = 0.05 if name == "indep05" else 0.5
        nan_k, nan_a, nan_v = (rng.random((12, n)) < p for _ in range(3))
    elif name in ("runs", "runs_shift"):
        # months 1-4, 5-8, 9-12 (runs): the changes fall on the edges of the GA groups; shifted by a month: inside them
        grp = (np.arange(12) - (name == "runs_shift")) % 12 // GA
        nan_k, nan_a, nan_v = (np.stack([rng.random(n) < 0.3 for _ in range(3)])[grp] for _ in range(3))
    elif name == "slot1":
        # a constant mask everywhere, and month after month other stations of the chosen cells' ranks 64 .. 99
        ring = rk.common(block, 64, INIT)
        flips = [_months_that_differ(rng, ring.size) for _ in range(3)]
        for mask, fl in zip((nan_k, nan_a, nan_v), flips):
            mask[:] = rng.random(n) < 0.2
            mask[:, ring] = fl
        # the ring's weights are small (bisquare: < 0.13): its stations ask for the ends of the ladder, so that they count
        for m in range(1, 13):
            for name_f in _fields(m)[:2]:
                s[name_f][ring] = np.where(np.arange(ring.size) % 2 == 0, 35.0, 147.0)
    elif name == "beyond":
        # every month asks the same of a station; only stations that no chosen cell ranks below init_nnghs come and go
        far = np.setdiff1d(np.arange(n), rk.union(block, INIT))
        for m in range(2, 13):
            for f1, fm in zip(_fields(1), _fields(m)):
                s[fm] = s[f1]
        for mask in (nan_k, nan_a, nan_v):
            mask[:] = rng.random(n) < 0.2
            mask[:, far] = _months_that_differ(rng, far.size)
    elif name == "dead":
        if var == "tmin":
            u = rk.union(block, INIT)
            nan_k[DEAD_OPTIM, u] = True
            for m in DEAD_ANOM:
                nan_a[m, u] = True
        else:                                                # (optim_nnghs stays finite: k_m is the filled table's)
            cols = columns(s)
            for r, c in window_cells(WIN, BLOCK_C):
                order, dist = rk(r, c)
                nan_v[DEAD_NUG, order[:primitives_numpy(cols, order, dist)["k"][DEAD_NUG]]] = True
    elif name == "one":
        # one station that every chosen cell ranks below 100 keeps a value; its neighbours of those months have none
        u, keep = rk.union(block, INIT), rk.common(block, 0, 32)[0]
        for i, m in enumerate(ONE_MONTHS):
            ko, ka = _fields(m + 1)[:2]
            nan_k[m, u] = nan_a[m, u] = True
            nan_k[m, keep] = nan_a[m, keep] = False
            s[ko][keep], s[ka][keep] = ONE_VALUES[i], ONE_VALUES[(i + 1) % 3]
    elif name == "families":
        nan_a, nan_v = rng.random((12, n)) < 0.3, rng.random((12, n)) < 0.3
    else:
        raise KeyError(name)
    return nan_k, nan_a, nan_v


class Case(object):
    """The two tables of a pattern, their columns and rankers, and the restatements of chosen cells (cached)."""

    def __init__(self, name, golden_case, rankers):
        grid, tmin, tmax = golden_case
        self.name, self.grid, self.table, self.cols, self.rk, self._np, self._orc = name, grid, {}, {}, rankers, {}, {}
        for var, da in (("tmin", tmin), ("tmax", tmax)):
            s = filled(da.stns, 7 + (var == "tmax"))
            apply_masks(s, *_pattern_masks(name, var, s, rankers[var]))
            self.table[var], self.cols[var] = _table(da, var, s), columns(s)

    def numpy(self, var, cells, mutant=None, init=INIT):
        """primitives_numpy of the cells: a list of dicts."""
        out = []
        for r, c in cells:
            key = (var, int(r), int(c), mutant, init)
            if key not in self._np:
                self._np[key] = primitives_numpy(self.cols[var], *self.rk[var](r, c), init=init, mutant=mutant)
            out.append(self._np[key])
        return out

    def db(self, orc, var):
        if ("db", var) not in self._orc:
            self._orc[("db", var)] = orc.Db(self.table[var])
        return self._orc[("db", var)]

    def oracle(self, orc, var, cells, init=INIT):
        db, prm = self.db(orc, var), orc.params(init_nnghs=init)
        out = []
        for r, c in cells:
            key = (var, int(r), int(c), init)
            if key not in self._orc:
                self._orc[key] = primitives_oracle(orc, db, prm, self.grid["lon"][c], self.grid["lat"][r])
            out.append(self._orc[key])
        return out

    def oracle_pt(self, orc, var, r, c):
        g = self.grid
        return orc.make_pt(g["lon"][c], g["lat"][r], g["elev"][r, c], g["tdi"][r, c], g[lst_key(var)][:, r, c])


_CASES, _RANKERS = {}, {}


def case(name, golden_case):
    """The pattern's Case, built once per process."""
    grid, tmin, tmax = golden_case
    if not _RANKERS:
        from topowx_amd import stationdb as sdb
        for var, da in (("tmin", tmin), ("tmax", tmax)):
            _RANKERS[var] = Ranker(np.asarray(da.stns[sdb.LON], np.float64), np.asarray(da.stns[sdb.LAT], np.float64), grid)
    if name not in _CASES:
        _CASES[name] = Case(name, golden_case, _RANKERS)
    return _CASES[name]


def walked(prims, daily):
    """walk over a list of primitives: kk [n, 12], ka [n, 12], status [n]."""
    w = [walk(p, daily) for p in prims]
    return np.array([x[0] for x in w]), np.array([x[1] for x in w]), np.array([x[2] for x in w])


def mask_facts(cs, var, cells):
    """What a pattern promises of its chosen cells, per family: [ncell, 11] booleans -- do consecutive months' finite masks
    differ among the ranks 0 .. 63, 64 .. 99, >= 100?"""
    out = {}
    for key in ("optim", "anom", "nug"):
        fin = np.isfinite(cs.cols[var][key])
        d = np.zeros((len(cells), 11, 3), bool)
        for i, (r, c) in enumerate(cells):
            f = fin[:, cs.rk[var](r, c)[0]]
            ch = f[1:] != f[:-1]
            d[i] = np.stack([ch[:, :64].any(1), ch[:, 64:INIT].any(1), ch[:, INIT:].any(1)], axis=1)
        out[key] = d
    return out


# ---- (e) the long-list launch -------------------------------------------------------------------------------------------------
def cluster_tables(golden_case, nclust, p=0.3):
    """test_gpu_stream._cluster_db's tables (the golden stations plus ``nclust`` inside CLUSTER_BOX) for both variables, with
    observations, every (station, month, family) NaN with probability p -- and the number of stations within 2 hd of the
    centre of each tile of CLUSTER_WIN (hd: centre to corner), which every valid candidate list of that tile holds."""
    from topowx_amd import stationdb as sdb, synth
    grid, tmin, tmax = golden_case
    tables, inside = {}, {}
    for var, base in (("tmin", tmin), ("tmax", tmax)):
        extra = synth.make_stations(CLUSTER_BOX, nclust, 77, var, base.days, with_obs=True, expand_deg=0.0)
        extra.stns[sdb.STN_ID] = ["T%07d" % i for i in range(extra.stns.size)]
        s = filled(np.concatenate([base.stns, extra.stns]), 9 + (var == "tmax"))
        rng = np.random.default_rng(_SEED["indep50"] + 5 + (var == "tmax"))
        apply_masks(s, *(rng.random((12, s.size)) < p for _ in range(3)))
        tables[var] = sdb.StationDataWrkChk(s, var, base.days, np.concatenate([base.var, extra.var], axis=1))
        lat, lon = np.asarray(grid["lat"], np.float64), np.asarray(grid["lon"], np.float64)
        cnt = []
        for r0 in range(CLUSTER_WIN[0].start, CLUSTER_WIN[0].stop, TS):
            for c0 in range(CLUSTER_WIN[1].start, CLUSTER_WIN[1].stop, TS):
                r1, c1 = min(r0 + TS, CLUSTER_WIN[0].stop) - 1, min(c0 + TS, CLUSTER_WIN[1].stop) - 1
                clat, clon = 0.5 * (lat[r0] + lat[r1]), 0.5 * (lon[c0] + lon[c1])
                hd = max(hav_km(clon, clat, lon[q], lat[r]) for q in (c0, c1) for r in (r0, r1))
                cnt.append(int((hav_km(clon, clat, s[sdb.LON], s[sdb.LAT]) <= 2.0 * hd).sum()))
        inside[var] = cnt
    return tables, inside
