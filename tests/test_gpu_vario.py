"""The variogram fit on the GPU (twx_vario.h: k_group_dist64, k_vario<0>, k_vario<1>, k_vfit_to_vario behind
twx_fit_vario_points and twx_krigall_points) against the oracle's get_vario_params, fed the neighbours the GPU itself ranked
(ctx.knn with the same exclusions), so that a difference is the fit's and not the selection's.  Bar: rtol 1e-6, atol 1e-9 on
(nugget, psill, range) and equal statuses (test_step22_farm's bar), on every case on which the oracle itself is insensitive
to the order of its neighbours (tests/vario_cases.py: at most 2 % of a test's cases are left out).

(a) every k from 7 to TWX_MAX_NNGHS in one call: the 256-pair stride of the pair loop, the wave boundaries of the residuals;
(b) one station x 16 bandwidths x 12 months in one list, a smaller k reading a prefix of the list's pair table, and the
    three ways two consecutive points must NOT share a list -- the invariant above k_group_dist64;
(c) sparse tables: bins shared by the four waves (more than TWX_VBINS / 4 of them) and pairs past the near / far switch of the
    pair distance;
(d) fallbacks and failures: residuals at rounding level, a co-located twin (bin 0 with mean distance 0), a constant predictor;
(e) twx_krigall_points against orc.krigall end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

import vario_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

NUMERIC = 4                                                  # TWX_CELL_NUMERIC


def _ctx(lib, table):
    ctx = lib.Context()
    ctx.set_stations(lib.TMIN, table, with_obs=False)
    return ctx


def _pts(ctx, cols, js):
    js = np.asarray(js)
    return ctx.make_pts(cols["lon"][js], cols["lat"][js], cols["elev"][js], cols["tdi"][js], cols["lst"][:, js].T)


def _knn(ctx, lib, cols, j, k, excl, rm_zero_dist=True):
    """The ranked neighbours of station j's location, in a call of its own (no list to share)."""
    idx, dist, _, st = ctx.knn(lib.TMIN, cols["lon"][[j]], cols["lat"][[j]], k, excl=np.asarray(excl, np.int32)[None],
                               rm_zero_dist=rm_zero_dist)
    assert st[0] == 0
    return vc.rank_order(idx[0], dist[0])


@pytest.fixture(scope="module")
def gold(golden_case, orc):
    _, tmin, _ = golden_case
    return tmin, orc.Db(tmin).cols


def test_every_k_against_the_oracle(gold, orc):
    """(a) One point per k = 7 .. 152 at stations spread over the golden Tmin table (the station itself excluded,
    rm_zero_dist, months cycling), one twx_fit_vario_points call: statuses and nnghs_used equal, parameters within the bar.
    k = 6 gives TWX_CELL_NUMERIC and NaN (the oracle: its range error), a k larger than the table a non-zero status and NaN.
    Measured on gfx950: largest share of the bar used (nugget, psill, range) = (0.47, 0.04, 0.14); cases left out: 0 of 146."""
    from topowx_amd import _lib as lib
    tmin, cols = gold
    js, ks, m0 = vc.every_k(cols["lon"].size)
    ctx = _ctx(lib, tmin)
    idx, dist, _, kst = ctx.knn(lib.TMIN, cols["lon"][js], cols["lat"][js], 152, excl=js, rm_zero_dist=True)
    assert np.all(kst == 0)
    idx, dist = vc.rank_order(idx, dist)
    jj = np.concatenate([js, js[:2]])
    nn = np.concatenate([ks, [6, cols["lon"].size + 100]]).astype(np.int32)
    mth = np.concatenate([m0 + 1, [1, 2]]).astype(np.int32)
    vario, used, st = ctx.fit_vario_points(lib.TMIN, _pts(ctx, cols, jj), mth, nnghs=nn, excl=jj, rm_zero_dist=True)
    ctx.close()
    cases = [(i, int(m0[i]), idx[i, :k], dist[i, :k]) for i, k in enumerate(ks)]
    worst, left_out, _ = vc.compare(orc, cols, cases, vario, st, "every k")
    print("every k: share of the bar used (nug, psill, range) %s, left out %d of %d" % (worst, left_out, len(cases)))
    ok = st[:ks.size] == 0
    assert ok.mean() > 0.9 and np.array_equal(used[:ks.size][ok], ks[ok])
    assert st[-2] == NUMERIC and np.isnan(vario[-2]).all() and used[-2] == 0
    rc6, _ = orc.get_vario_params(*(cols[c][idx[0, :6]] for c in ("lon", "lat", "elev")), cols["lst"][0, idx[0, :6]],
                                  cols["norm"][0, idx[0, :6]], float(dist[0, :6].max()))
    assert rc6 == 6                                            # ORC_ERR_RANGE
    assert st[-1] != 0 and np.isnan(vario[-1]).all() and used[-1] == 0


STATION = 137                                                # (b)'s station of the golden table


def test_one_list_nested_neighbourhoods_and_lists_that_must_not_be_shared(gold, orc):
    """(b) step21's shape: one station x 16 unsorted bandwidths x 12 months = 192 consecutive points, one list, one pair
    table (k_group_dist64 fills it from the list's first point, whose k is not the largest); every point against the oracle
    on its own.  Then pairs of consecutive points whose neighbour lists differ and must not be shared: the same location
    with another excluded station, the same location with other exclusion LISTS (twx_set_exclusions), two stations back to
    back -- each against the oracle, with the neighbours of each point ranked in a knn call of its own.
    Measured on gfx950: largest share of the bar used (nugget, psill, range) = (0.83, 0.06, 0.08); cases left out: 0 of 204."""
    from topowx_amd import _lib as lib
    tmin, cols = gold
    j = STATION
    ctx = _ctx(lib, tmin)
    idx, dist = _knn(ctx, lib, cols, j, 152, j)
    nn = np.repeat(np.array(vc.LADDER, np.int32), 12)
    mth = np.tile(np.arange(1, 13, dtype=np.int32), len(vc.LADDER))
    assert nn.size == 192 and nn[0] < nn.max()
    jj = np.full(nn.size, j)
    vario, used, st = ctx.fit_vario_points(lib.TMIN, _pts(ctx, cols, jj), mth, nnghs=nn, excl=jj, rm_zero_dist=True)
    cases = [(i, int(mth[i]) - 1, idx[:k], dist[:k]) for i, k in enumerate(nn)]
    worst, left_out, _ = vc.compare(orc, cols, cases, vario, st, "one list", cap=False)
    assert np.all(st == 0) and np.array_equal(used, nn)
    total = len(cases)
    # two (location, exclusion) keys A, B as consecutive points: A k=60, A k=25, B k=60, B k=25, month 5
    a, b, c = int(idx[1]), int(idx[3]), int(idx[2])
    keys = {"another excluded station": ((j, [j]), (j, [int(idx[0])])),
            "other exclusion lists": ((j, [j, a, b]), (j, [j, c, -1])),
            "two stations": ((j, [j]), (j + 1, [j + 1]))}
    for what, (ka, kb) in keys.items():
        ngh = [_knn(ctx, lib, cols, loc, 60, ex) for loc, ex in (ka, kb)]
        assert not np.array_equal(ngh[0][0][:25], ngh[1][0][:25]), what        # the two lists do differ, within k = 25 already
        loc = np.repeat([ka[0], kb[0]], 2)
        ex = np.repeat(np.array([ka[1], kb[1]], np.int32), 2, axis=0)
        k4 = np.array([60, 25, 60, 25], np.int32)
        v4, u4, s4 = ctx.fit_vario_points(lib.TMIN, _pts(ctx, cols, loc), 5, nnghs=k4, excl=ex if ex.shape[1] > 1 else ex[:, 0],
                                          rm_zero_dist=True)
        assert np.all(s4 == 0) and np.array_equal(u4, k4), (what, s4, u4)
        c4 = [(i, 4, ngh[i // 2][0][:k4[i]], ngh[i // 2][1][:k4[i]]) for i in range(4)]
        w, lo, _ = vc.compare(orc, cols, c4, v4, s4, what, cap=False)
        worst, left_out, total = np.maximum(worst, w), left_out + lo, total + 4
    ctx.close()
    print("one list: share of the bar used (nug, psill, range) %s, left out %d of %d" % (worst, left_out, total))
    assert left_out <= vc.MAX_LEFT_OUT * total, (left_out, total)


def test_sparse_tables_shared_bins_and_far_pairs(orc):
    """(c) Synthetic tables of 120 .. 200 stations over boxes 12 .. 30 degrees wide, k in {30, 60, 100}: largest neighbour
    distances from ~200 to ~1 800 km.  At least a quarter of the cases keep the bins per wave (nb <= 128), at least a quarter
    share them among the four waves (128 < nb <= 512), at least 20 hold a pair inside the cutoff past the near / far switch
    of the pair distance (S >= 4e-3, ~807 km: ellip_far_f64); none needs more than TWX_VBINS bins.  The bar is the same.
    Two runs give the same bits where the kernel promises it: the nb <= 128 cases.
    Measured on gfx950: largest share of the bar used (nugget, psill, range) = (0.93, 0.02, 0.06); cases left out: 0 of 160;
    46 cases with nb <= 128, 114 with 128 < nb <= 512, 87 with a far pair.  (The nugget's share is of the bar's absolute
    term: nuggets below 1e-4 that differ by up to 9.3e-10.)"""
    from topowx_amd import _lib as lib
    worst, left_out, total, small, mid, far = np.zeros(3), 0, 0, 0, 0, 0
    for ti in range(len(vc.SPARSE)):
        table = vc.sparse_table(ti)
        cols = orc.Db(table).cols
        pts = vc.sparse_points(ti, cols["lon"].size)
        js = np.array([p[0] for p in pts])
        ks = np.array([p[1] for p in pts], np.int32)
        mth = np.array([p[2] + 1 for p in pts], np.int32)
        ctx = _ctx(lib, table)
        idx, dist, _, kst = ctx.knn(lib.TMIN, cols["lon"][js], cols["lat"][js], int(ks.max()), excl=js, rm_zero_dist=True)
        assert np.all(kst == 0)
        idx, dist = vc.rank_order(idx, dist)
        runs = [ctx.fit_vario_points(lib.TMIN, _pts(ctx, cols, js), mth, nnghs=ks, excl=js, rm_zero_dist=True)
                for _ in range(2)]
        ctx.close()
        vario, used, st = runs[0]
        assert np.array_equal(used, np.where(st == 0, ks, 0))
        S = vc.sin2_half_angle(cols["lon"], cols["lat"])
        cases, per_wave = [], np.zeros(ks.size, bool)
        for i, k in enumerate(ks):
            ii, dd = idx[i, :k], dist[i, :k]
            nb = vc.nbins(dd)
            assert nb <= vc.VBINS, (ti, i, nb)
            per_wave[i] = nb <= vc.VBINS // 4
            h = orc.ellip_dist(cols["lon"][ii][:, None], cols["lat"][ii][:, None], cols["lon"][ii][None, :],
                               cols["lat"][ii][None, :])
            far += bool(((S[np.ix_(ii, ii)] >= 4.05e-3) & (h <= 1.4 * dd.max() * (1 - 1e-9))).any())
            cases.append((i, int(mth[i]) - 1, ii, dd))
        small, mid = small + int(per_wave.sum()), mid + int((~per_wave).sum())
        assert np.array_equal(runs[1][2], st)
        assert np.array_equal(runs[1][0][per_wave].view(np.uint64), vario[per_wave].view(np.uint64)), ti
        w, lo, want = vc.compare(orc, cols, cases, vario, st, "sparse table %d" % ti, cap=False)
        assert all(rc == 0 for rc, _ in want), ti                               # every oracle fit succeeds
        worst, left_out, total = np.maximum(worst, w), left_out + lo, total + len(cases)
    print("sparse: share of the bar used (nug, psill, range) %s, left out %d of %d; nb <= 128: %d, 128 < nb <= 512: %d, far pair: %d"
          % (worst, left_out, total, small, mid, far))
    assert left_out <= vc.MAX_LEFT_OUT * total, (left_out, total)
    assert 4 * small >= total and 4 * mid >= total and far >= 20, (small, mid, far, total)


def _run_points(lib, orc, table, js, ks, mths, rm_zero_dist=True, elev=None):
    """fit_vario_points at stations js (their own station excluded) and each point's ranked neighbours."""
    cols = orc.Db(table).cols
    js, ks, mths = np.asarray(js), np.asarray(ks, np.int32), np.asarray(mths, np.int32)
    ctx = _ctx(lib, table)
    idx, dist, _, kst = ctx.knn(lib.TMIN, cols["lon"][js], cols["lat"][js], int(ks.max()), excl=js, rm_zero_dist=rm_zero_dist)
    assert np.all(kst == 0)
    idx, dist = vc.rank_order(idx, dist)
    pts = _pts(ctx, cols, js)
    if elev is not None:
        pts["elev"] = elev
    vario, used, st = ctx.fit_vario_points(lib.TMIN, pts, mths, nnghs=ks, excl=js, rm_zero_dist=rm_zero_dist)
    ctx.close()
    cases = [(i, int(mths[i]) - 1, idx[i, :k], dist[i, :k]) for i, k in enumerate(ks)]
    return cols, cases, vario, used, st


def test_residuals_at_rounding_level(gold, orc):
    """(d) Normals that are an exact linear trend in the predictors plus 1e-9 noise: residuals of ~1e-9 degC.  Statuses
    equal; the total sill (the residual variance) is below 1e-15 on both sides (test_oracle_vario's bar for the same
    construction: the noise has variance 1e-18, so a residual with 3e-8 degC of rounding error from the kernel's unscaled
    normal equations would break it); where the oracle's two neighbour orders agree on fitted versus pure nugget the kernel
    has that form, (sill, 0, 0) with exact zeros, and where they agree to 1e-8 the parameters meet the bar.
    The oracle's own fitted RANGE on such residuals is not reproducible: it changed by more than 1e-8 with the order of
    the neighbours in all 36 cases (the residuals carry ~1e-6 of their size in rounding error), so the 2 % cap on cases
    left out cannot hold here and is not asserted; the form and the sill are.
    Measured on gfx950: largest total sill 1.27e-18; oracle orders agreeing on the form in 35 of 36 cases, to 1e-8 in 0."""
    from topowx_amd import _lib as lib
    tmin, _ = gold
    n = tmin.stns.size
    js = np.repeat(np.linspace(0, n - 1, 12).astype(int), 3)
    ks = np.tile([20, 60, 110], 12)
    mths = 1 + (js + ks) % 12
    cols, cases, vario, used, st = _run_points(lib, orc, vc.trend_table(tmin), js, ks, mths)
    assert np.all(st == 0) and np.array_equal(used, ks)
    _, unstable, want = vc.compare(orc, cols, cases, vario, st, "trend", cap=False)
    assert float((vario[:, 0] + vario[:, 1]).max()) < 1e-15 and np.all(vario >= 0)
    same_form = 0
    for (i, m0, ii, dd), (rc, v) in zip(cases, want):
        assert rc == 0 and v[0] + v[1] < 1e-15
        a = [cols["lon"][ii], cols["lat"][ii], cols["elev"][ii], cols["lst"][m0, ii], cols["norm"][m0, ii]]
        rc2, v2 = orc.get_vario_params(*[x[::-1] for x in a], float(dd.max()))
        if rc2 == 0 and (v[2] > 0) == (v2[2] > 0):
            same_form += 1
            assert (vario[i, 2] > 0) == (v[2] > 0) and (vario[i, 1] > 0) == (v[1] > 0), (i, vario[i], v)
    print("trend: largest total sill %.3g; oracle orders agree on the form in %d of %d cases, to 1e-8 in %d"
          % ((vario[:, 0] + vario[:, 1]).max(), same_form, len(cases), len(cases) - unstable))


# (point station, k, station that gets the twin): neighbourhoods of the golden table without another pair under 5 km, on
# which the oracle reports the singular GLS system in either neighbour order (found on the CPU, re-checked below)
TWINS = ((66, 10, 244, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)), (61, 14, 227, (1, 2, 3, 4, 5, 6, 7, 9, 10)),
         (12, 20, 238, (3, 4, 8, 9, 10, 11, 12)))


def test_co_located_twin_in_the_neighbourhood(gold, orc):
    """(d) A twin of a neighbour (same place, other elevation and normals), rm_zero_dist off, no other pair of the
    neighbourhood under 5 km: bin 0 of the semivariogram holds the twin pair alone, mean distance 0, weight np / h^2
    infinite -- the range fit of pass 0 is unusable on both sides (the weighted sums are NaN) and falls back to the pure
    nugget.  That model never becomes the result: the GLS trend between the two fits has the twins' identical rows (c(0) =
    the full sill for any two stations at distance 0, in the oracle's cov_model and in the kriging kernels), the system is
    singular, and both sides report it: TWX_CELL_NUMERIC / ORC_ERR_NUMERIC and NaN parameters, not a crash or a finite
    model from an infinite weight.  (Where the oracle's Cholesky lets the exactly singular matrix through on rounding, its
    result depends on the month and the order of the neighbours; the kernels flag coincident neighbours by their distance:
    SelWs.cdup.  Those neighbourhoods are not used here.)"""
    from topowx_amd import _lib as lib
    tmin, cols0 = gold
    n = tmin.stns.size
    for p, k, s, months in TWINS:
        table = vc.twin_table(tmin, s)
        cols, cases, vario, used, st = _run_points(lib, orc, table, [p] * len(months), [k + 1] * len(months), months,
                                                   rm_zero_dist=False)
        ii = cases[0][2]
        assert (ii == n).any() and (ii == s).any()                              # the twin and its original are neighbours
        h = orc.ellip_dist(cols["lon"][ii][:, None], cols["lat"][ii][:, None], cols["lon"][ii][None, :], cols["lat"][ii][None, :])
        iu = np.triu_indices(ii.size, 1)
        assert (h[iu] == 0.0).sum() == 1 and np.sort(h[iu])[1] > 5.0           # bin 0: the twin pair alone
        _, left_out, want = vc.compare(orc, cols, cases, vario, st, "twin %d" % p)
        assert left_out == 0 and all(rc == NUMERIC for rc, _ in want)
        assert np.all(st == NUMERIC) and np.isnan(vario).all() and np.all(used == 0)


def test_constant_predictor_column(gold, orc):
    """(d) A predictor that is constant over the neighbourhood and differs from the point's own value (all stations at one
    elevation, the point elsewhere; one month's LST constant): the column is collinear with the intercept, lm() has no
    unique solution.  The oracle centres its columns and fails in the Cholesky of the normal equations; the kernel must
    report TWX_CELL_NUMERIC with NaN parameters too, not a fit through a pivot that is rounding error."""
    from topowx_amd import _lib as lib
    tmin, _ = gold
    js = np.repeat([5, 100, 200, 333], 2)
    ks = np.tile([20, 60], 4)
    for column in ("elev", "lst"):
        cols, cases, vario, used, st = _run_points(lib, orc, vc.const_table(tmin, column), js, ks,
                                                   np.full(js.size, vc.CONST_LST_MONTH), elev=1500.0 + 10.0 * js)
        _, left_out, want = vc.compare(orc, cols, cases, vario, st, "constant " + column)
        assert left_out == 0 and all(rc == NUMERIC for rc, _ in want)
        assert np.all(st == NUMERIC) and np.isnan(vario).all() and np.all(used == 0), (column, st, vario)


def test_krigall_points_against_the_oracle(gold, orc):
    """(e) twx_krigall_points (fit, then krige with the fitted model, one selection) against orc.krigall, which selects
    its own neighbours: 24 stations of the golden table and 24 of a sparse one (bins shared among the waves), months and
    bandwidths cycling.  Statuses equal, variograms within the bar, means within 1e-5 degC.
    Measured on gfx950: max |mean difference| 4.5e-7 degC; largest share of the bar used (nugget, psill, range) =
    (0.40, 0.06, 0.05); cases left out: 0 of 48."""
    from topowx_amd import _lib as lib
    tmin, _ = gold
    worst, worst_mean, left_out = np.zeros(3), 0.0, 0
    for what, table, kset in (("golden", tmin, (35, 62, 91, 110, 147, 12)), ("sparse", vc.sparse_table(3), (30, 60, 45))):
        db, prm = orc.Db(table), orc.params()
        cols = db.cols
        js = np.linspace(0, cols["lon"].size - 1, 24).astype(int)
        ks = np.array([kset[i % len(kset)] for i in range(24)], np.int32)
        mth = 1 + np.arange(24, dtype=np.int32) % 12
        ctx = _ctx(lib, table)
        idx, dist, _, kst = ctx.knn(lib.TMIN, cols["lon"][js], cols["lat"][js], int(ks.max()), excl=js, rm_zero_dist=True)
        mean, _, vario, used, st = ctx.krigall_points(lib.TMIN, _pts(ctx, cols, js), mth, nnghs=ks, excl=js, rm_zero_dist=True)
        ctx.close()
        assert np.all(kst == 0)
        idx, dist = vc.rank_order(idx, dist)
        for i, j in enumerate(js):
            m0 = int(mth[i]) - 1
            _, _, stable = vc.oracle_fit(orc, cols, idx[i, :ks[i]], dist[i, :ks[i]], m0)
            pt = orc.make_pt(cols["lon"][j], cols["lat"][j], cols["elev"][j], cols["tdi"][j], cols["lst"][:, j])
            rc, norms, v = orc.krigall(db, prm, pt, int(ks[i]), excl=int(j), rm_zero_dist=True)
            if not stable:
                left_out += 1
                continue
            assert st[i] == rc == 0 and used[i] == ks[i], (what, i, st[i], rc)
            assert np.all(np.abs(vario[i] - v[m0]) <= vc.ATOL + vc.RTOL * np.abs(v[m0])), (what, i, vario[i], v[m0])
            assert abs(mean[i] - norms[m0]) <= 1e-5, (what, i, mean[i], norms[m0])
            worst_mean = max(worst_mean, abs(mean[i] - norms[m0]))
            worst = np.maximum(worst, np.abs(vario[i] - v[m0]) / (vc.ATOL + vc.RTOL * np.abs(v[m0])))
    print("krigall: max |d mean| %.3g degC, share of the bar used (nug, psill, range) %s, left out %d of 48" % (worst_mean, worst, left_out))
    assert left_out <= vc.MAX_LEFT_OUT * 48
