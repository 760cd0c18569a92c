"""Shared by tests/test_chkperf_host.py and tests/test_gpu_chkperf.py: the golden of make_golden_chkperf.py, the series of
the shape grid and of the degenerate items, the tolerances of DESIGN.md section 19, and the synthetic pool of the facade
test with its numpy restatement of search, check and ladder (no GPU anywhere in this file)."""
import datetime as dt
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_chkperf as RC  # noqa: E402

FACTOR = 100.0                     # section 18's factor for a different but fixed summation order
U = 2.0 ** -52
GRID_N = (4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2139, 8192)
GRID_SEED = 19
STEP = 4.0                         # the factor of the standard deviation across a variance step of the grid


def load_gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_chkperf_v1.npz"))


def tolerances(want, n):
    """(mae, r2, cpt_stat) bounds for a kernel value against the float64 restatement ``want`` (a ``check_pair`` record)."""
    return (max(FACTOR * want["d_mae"], n * U), max(FACTOR * want["d_r2"], n * U), max(FACTOR * want["d_cpt"], n * n * U))


def grid_series():
    """The series of the shape grid: a list of (name, fit, obs).  Per N an iid series and variance steps at tau = 2, N - 2,
    64, 256 and N / 2 (those that lie in 2 .. N - 2, each once): the shorter side of the step has STEP times the standard
    deviation.  obs = fit + noise, a tenth missing (at least two present)."""
    rs = np.random.RandomState(GRID_SEED)
    out = []
    for n in GRID_N:
        taus = []
        for t in (2, n - 2, 64, 256, n // 2):
            if 2 <= t <= n - 2 and t not in taus:
                taus.append(t)
        for t in [None] + taus:
            fit = rs.randn(n)
            if t is not None:
                fit *= np.where((np.arange(n) < t) == (t <= n // 2), STEP, 1.0)
            fit = 3.0 + fit
            obs = fit + 0.5 * rs.randn(n)
            miss = rs.rand(n) < 0.1
            miss[:2] = False
            obs[miss] = np.nan
            out.append(("N %d %s" % (n, "iid" if t is None else "step at %d" % t), fit, obs))
    return out


def mirrored(n=64):
    """A series of integers, mirrored about its middle (n even, a multiple of 8), quiet at both ends and loud in the
    middle: every sum of the check is exact, so tmp(tau) and tmp(n - tau) are the same bytes and the two best splits, at
    n / 4 and 3 n / 4, tie."""
    q = n // 4
    half = np.concatenate([np.tile([1.0, -1.0], q // 2), np.tile([12.0, -12.0], q // 2)])
    return np.concatenate([half, half[::-1]])


def degenerate_series():
    """(name, fit, obs) of the degenerate items, in the order the tests index them."""
    rs = np.random.RandomState(7)
    n = 96
    base = 2.0 + rs.randn(n)
    one = np.full(n, np.nan)
    one[17] = base[17] + 0.25
    bad = base.copy()
    bad[40] = np.nan
    inf = base.copy()
    inf[0] = np.inf
    big = 1.0 + rs.randn(RC.MAX_ROWS + 1)
    nc = 186           # every tmp of a constant series is tau L + (N - tau) L with L = log 1e-10, equal only up to rounding; at
    #                    this N the first tau is the smallest for L and for its two neighbours in fp64
    return [("constant", np.full(nc, 3.0), np.where(np.arange(nc) % 3 == 0, np.nan, 3.5)),
            ("mirrored", mirrored(64), mirrored(64) + 0.5),
            ("nobs 0", base, np.full(n, np.nan)),
            ("nobs 1", base, one),
            ("NaN in fit", bad, base + 0.1),
            ("inf in fit", inf, base + 0.1),
            ("N 3", base[:3].copy(), base[:3] + 0.1),
            ("N 8193", big, big + 0.1),
            ("N 0", np.zeros(0), np.zeros(0)),
            ("constant obs", base, np.full(n, 1.5))]


def flat(series):
    """(off, fit, obs) of a list of (name, fit, obs)."""
    off = np.concatenate([[0], np.cumsum([s[1].size for s in series])]).astype(np.int64)
    return off, np.concatenate([s[1] for s in series]), np.concatenate([s[2] for s in series])


# ---- the pool of the facade test ----
FACADE_SEED = 3
FACADE_NSTN = 16
FACADE_TARGETS = (1, 5, 12)        # ordinary; heavy local noise; in the half whose later years are damped
NOISY, DAMPED_FROM_YEAR, DAMPING = 5, 2004, 0.07


def facade_pool(seed=FACADE_SEED):
    """16 stations x 6 years (186 rows in a 31-day month): two groups of 8 stations 4 degrees apart.  Station NOISY carries
    local noise of 5 degrees; in the second group the regional signal is damped by DAMPING (about tenfold) from DAMPED_FROM_YEAR on.
    Returns (pool, mean, vari)."""
    from topowx_amd.dates import MONTH, YEAR, get_days_metadata
    from topowx_amd.qa import StationObsPool
    rs = np.random.RandomState(seed)
    n = FACADE_NSTN
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2006, 12, 31))
    nd = days.size
    grp = np.arange(n) >= n // 2
    lon = np.where(grp, -106.0, -110.0) + 0.5 * rs.rand(n)
    lat = 45.0 + 0.5 * rs.rand(n)
    fac = np.zeros((nd, 3))
    e = rs.randn(nd, 3) * np.array([3.0, 1.2, 0.8])
    for i in range(1, nd):
        fac[i] = 0.6 * fac[i - 1] + e[i]
    load = np.concatenate([np.ones((1, n)), rs.randn(2, n) * 0.7], axis=0)
    sig = fac @ load
    late = np.asarray(days[YEAR]) >= DAMPED_FROM_YEAR
    sig[np.ix_(late, grp)] *= DAMPING
    noise = np.full(n, 0.2)
    noise[NOISY] = 5.0
    tmin = 2.0 + sig + rs.randn(n)[None, :] * 2.0 + rs.randn(nd, n) * noise[None, :]      # no seasonal cycle: months are alike
    tmin = np.round(tmin, 2)
    tmin[rs.rand(nd, n) < 0.08] = np.nan
    tmin = tmin.astype(np.float32)
    mean, vari = np.full((n, 12), np.nan), np.full((n, 12), np.nan)
    for g in range(12):
        rows = tmin[np.asarray(days[MONTH]) == g + 1].astype(np.float64)
        for s in range(n):
            v = rows[np.isfinite(rows[:, s]), s]
            mean[s, g], vari[s, g] = v.mean(), v.var()
    ids = np.array(["CHK%05d" % i for i in range(n)])
    return StationObsPool(ids, lon, lat, tmin, tmin + 10, days), mean, vari


def facade_items(pool, mean, vari, targets=FACADE_TARGETS):
    """The items of the facade's call from the numpy restatement of the matrix builder: (items, obs, group) as
    ``daily_items`` returns them (``obs`` station-major float32)."""
    import ppca_cases as PC
    from topowx_amd.dates import MONTH
    from topowx_amd.infill import assemble_daily_columns
    from topowx_amd.infill.infill_daily import month_mask_groups
    group = (np.asarray(pool.days[MONTH], np.int64) - 1).astype(np.int8)
    obs = np.ascontiguousarray(pool.tmin.T)
    items = {}
    for mask, months in month_mask_groups(mean, vari):
        m = PC.host_matrices(pool, mask, np.asarray(targets), months)
        for t in range(len(targets)):
            for k, g in enumerate(months):
                cols, extra, norms, stds = assemble_daily_columns(m, t, k, mean[:, g], vari[:, g], None)
                items[(t, g)] = dict(t=t, col=int(targets[t]), g=g, matrix_status=int(m.status[t, k]), cols=cols, extra=extra,
                                     norms=norms, stds=stds, ncomp=0, key=None, nnr=None)
    return [items[k] for k in sorted(items)], obs, group


def restated_ladder(item, obs, group, threshold=1e-5, sig=1e-10, max_r2cum=0.99):
    """Search, check and ladder of one item in numpy, float64 next to longdouble: a dict of ``ladder`` (restate_chkperf's
    record), ``checks`` / ``searches`` per attempt (float64; a repeated attempt is the earlier one's), ``agree`` (the two
    precisions take every decision alike: attempts, reasons, kept, and per search npcs / nfits / iters) and ``d_ref`` per
    attempt."""
    import ppca_cases as PC
    from topowx_amd.infill import item_matrix
    days = np.nonzero(group == item["g"])[0]
    y = item_matrix(obs, days, item)
    o = obs[item["col"], days].astype(np.float64)
    pen = RC.cpt_penalty(days.size, sig)
    thr = (threshold, threshold) + RC.RETRY_THRESHOLDS
    cache, rec = {}, dict(checks={}, searches={}, d_ref={}, agree=True)

    def judge(a):
        if thr[a] not in cache:                                      # no reanalysis columns: attempt 1 repeats attempt 0
            w = PC.want_search(y, threshold=thr[a], max_r2cum=max_r2cum)
            if not np.isfinite(w["d_ref"]) or PC.left_out(w):
                rec["agree"] = False
            fit = w["fit"] * item["stds"][0] + item["norms"][0]
            c = RC.check_pair(fit, o, pen)
            if not np.isfinite(max(c["d_mae"], c["d_r2"], c["d_cpt"])):
                rec["agree"] = False
            cache[thr[a]] = (w, c, fit)
        w, c, fit = cache[thr[a]]
        rec["checks"][a], rec["searches"][a], rec["d_ref"][a] = c, dict(w, fit_c=fit), w["d_ref"]
        return c["reasons"], float(c["mae"]), w["status"] in (0, 20)

    rec["ladder"] = RC.ladder(judge, RC.MIN_NNR_VAR < 0.99)
    return rec
