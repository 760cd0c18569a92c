"""Synthetic pools and station databases for the corroboration / mega-inconsistency tests (tests/test_corrob_host.py,
tests/test_gpu_corrob.py) and tests/tools/gpu_corrob_timing.py.  The golden case has its own generator in
tests/golden/make_golden_corrob.py."""
import numpy as np

import spatial_cases
from topowx_amd import ncio
from topowx_amd import stationdb as sdb

BIG_SEED = 8               # the regression tests' big case: its regression margins are known to clear 1e-5
N_SHORT, N_FAR = 60, 5


def big_case(n=2000, years=10, seed=BIG_SEED, year0=1991):
    """``spatial_cases.big_case`` plus what the later checks need: every 33rd station (``N_SHORT`` of 2 000) loses its
    first ``years - 5`` years, so it has no normals (and its neighbours see a neighbour without one); the last ``N_FAR``
    stations are moved 40 degrees east, 2 degrees apart (no neighbours: only the mega-inconsistency check runs), each
    with a Tmin above every Tmax and a Tmax below every Tmin of its calendar month; 200 stations get a +-11..14 degC
    spike in Tmax inside a stretch thinned to every third day (too few window days for the regression check)."""
    ids, lon, lat, tmin, tmax, days, spikes = spatial_cases.big_case(n, years, seed, year0)
    rs = np.random.RandomState(seed + 1000)
    nd = days.size
    cut = int(np.nonzero(days.YEAR == days.YEAR[0] + max(years - 5, 0))[0][0]) if years > 5 else 0
    short = np.arange(16, n, 33)[:N_SHORT]
    tmin[:cut, short] = np.nan
    tmax[:cut, short] = np.nan
    far = np.arange(n - N_FAR, n)
    lon[far], lat[far] = -70.0 + 2.0 * np.arange(N_FAR), 45.0
    for s in far:
        d1, d2 = rs.randint(10, nd - 10, 2)
        tmin[d1, s], tmax[d1, s] = 48.0, np.nan
        tmax[d2, s], tmin[d2, s] = -40.0, np.nan
    if nd > 1000:
        for s in rs.choice(np.setdiff1d(np.arange(n - N_FAR), short), min(200, n // 10), replace=False):
            a = int(rs.randint(200, nd - 400))
            thin = np.arange(a, a + 150)
            tmax[thin[thin % 3 != 0], s] = np.nan
            d = a + 75 - (a + 75) % 3
            tmax[d, s] = np.float32(np.round(np.nan_to_num(tmax[d, s], nan=10.0) + rs.choice([-1, 1]) * rs.randint(110, 141) / 10.0, 1))
    return ids, lon, lat, tmin, tmax, days, spikes


def write_db(path, ids, lon, lat, tmin, tmax, days, fmt, qflags=True, prev=()):
    """An all-stations database in the reference's layout; ``qflags``: with ``qflag_tmin`` / ``qflag_tmax`` (``"S1"``,
    empty); ``prev``: ``(variable name, day, station, character)`` entries set beforehand."""
    n = ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = ids, lon, lat, 100.0
    variables = [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                 ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")]
    if qflags:
        variables += [("qflag_tmin", "S1", "", "quality assurance flag tmin", ""),
                      ("qflag_tmax", "S1", "", "quality assurance flag tmax", "")]
    ncio.create_quick_db(path, stns, days, variables, format=fmt)
    ds = ncio.open_dataset(path, "a")
    try:
        for name, a in (("tmin", tmin), ("tmax", tmax)):
            v = ds.variables[name]
            v.missing_value = np.float32(ncio.FILL_F4)
            v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
        for name in sorted(set(p[0] for p in prev)):
            q = np.zeros((days.size, n), "S1")
            for _, d, s, ch in (p for p in prev if p[0] == name):
                q[d, s] = ch
            ds.variables[name][:] = q
    finally:
        ds.close()
    return path
