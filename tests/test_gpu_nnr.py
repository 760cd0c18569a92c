"""GPU: the reanalysis columns (``twxnr_components``; ``topowx_amd.NNRNghData.batched_components``) against the executed
reference (tests/golden/make_golden_nnr.py) and the numpy restatement (tests/restate_nnr.py): on the seeded case, on the
edge shapes through the raw entry, for byte equality of two calls, and end to end through ``estimate_mean_variance``,
``infill_daily(chk_perf=True)``, ``XvalInfill`` and the three command lines, each against the per-target host route.

``ncomp`` at both cuts is compared exactly.  ``var_explain`` and the sign-aligned scores are compared within the bound of
``restate_nnr.score_bound`` / ``var_explain_bound``: per component the larger of 100 x e_ref and 100 x eps x (lambda_1 /
gap_k) x max |score_k|.  Measured on the case: e_ref (the executed reference against the longdouble evaluation) up to
1.0e-13 for a score and 1.1e-15 for var_explain; e_gram (the restated float64 Gram route against the same) up to 4.8e-14
and 7.6e-16; the GPU against the executed reference (MI355X): 1.0e-13 for a score over the 33 items whose scores the
fixture holds, 2.4e-15 for var_explain over all 132; against the restatement on the other 99 items 1.1e-13 for a score
(DESIGN.md section 22).

End to end the two routes give score columns that differ by the bound above and, for a component, possibly by sign (the host
route's is LAPACK's).  norm's EM starts from the identity and is symmetric under a column's sign, so step14's estimates are
compared as they come, within the 1e-10 of tests/test_gpu_emnorm.py.  The PPCA start C0 is NOT symmetric under a column's
sign, so for step16 / step15 the host route's columns are turned to the kernel's sign rule first; the fits are then
compared within 1e-9 target standard deviations: the columns differ by ~1e-13 relative, and an EM of at most 1000
iterations whose map has a Lipschitz constant near 1 carries that to at most ~1e-10 -- ten times that is allowed.  The
step16 test also runs the host route unpatched and prints how far LAPACK's signs, another start, move the result (up to
0.174 target standard deviations where search and ladder end alike, 0.309 anywhere: reported, not bounded).  Every
comparison prints the largest deviation it saw.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nnr_cases as NC  # noqa: E402
import restate_nnr as RN  # noqa: E402

pytestmark = pytest.mark.gpu
EM_TOL, FIT_TOL = 1e-10, 1e-9


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_nnr_v1.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def case():
    return NC.case()


@pytest.fixture(scope="module")
def batch(case):
    tm = {}
    b = case.reader().batched_components(case.lon, case.lat, "tmax", case.utc, case.day_idx, NC.CUTS, NC.NNGH, timing=tm)
    return b, tm


def test_case_against_the_executed_reference(batch, gold, case):
    from topowx_amd import _qalib
    b, tm = batch
    assert b.set_of.tolist() == gold["stn_set"].tolist() and len(b.sets) == 11 and tm["nr_sets"] == 11
    for k in ("nr_gram_kernel_ms", "nr_eig_kernel_ms", "nr_scores_kernel_ms", "nr_upload_ms", "nr_download_ms", "nr_select_s"):
        assert k in tm and np.isfinite(tm[k]) and tm[k] >= 0, (k, tm)
    assert (b.res.status == _qalib.NR_OK).all() and (b.res.sweeps > 0).all() and (b.res.sweeps < _qalib.NR_MAX_SWEEPS).all()
    worst_sc, worst_ve, nsc, worst_re, nre = 0.0, 0.0, 0, 0.0, 0
    rd = case.reader()
    for x, s in enumerate(gold["set_rep"]):
        t = int(s)
        whole = rd.get_nngh_matrix(case.lon[t], case.lat[t], "tmax", int(case.utc[t]), NC.NNGH)
        for g in range(12):
            assert [b.ncomp(t, g, c) for c in NC.CUTS] == gold["ncomp"][x, g].tolist(), (x, g)
            ve = b.var_explain(t, g)
            dv = np.abs(ve - gold["var_explain"][x, g]).max()
            assert dv <= RN.var_explain_bound(ve, gold["e_ref_ve"][x, g]), (x, g, dv)
            worst_ve = max(worst_ve, dv)
            load = b.loadings(t, g)
            assert (load[np.arange(32), np.abs(load).argmax(axis=1)] > 0).all()
            assert b.scores(t, g, 0.90).shape == (len(case.day_idx[g]), gold["ncomp"][x, g, 1])
            key = "scores_%d_%d" % (x, g)
            if key in gold:
                k = int(gold["ncomp"][x, g, 0])
                sc = b.scores(t, g, 0.99)
                err = RN.column_error(gold[key], sc)
                bound = RN.score_bound(b.res.eigval(int(b.set_of[t]), g), sc, gold["e_ref"][x, g], k)
                assert (err <= bound).all(), (x, g, err, bound)
                worst_sc, nsc = max(worst_sc, float(err.max())), nsc + 1
            else:
                # the fixture holds no scores of this month: the restated float64 Gram route, which the maker pins within
                # e_gram of the longdouble evaluation, stands in; both sides carry an error of their own: twice the bound
                k = int(gold["ncomp"][x, g, 0])
                sc = b.scores(t, g, 0.99)
                re = RN.components(whole[case.day_idx[g]], NC.CUTS)
                err = RN.column_error(re["scores"][:, :k], sc)
                bound = 2 * RN.score_bound(re["eigval"], sc, gold["e_ref"][x, g], k)
                assert (err <= bound).all(), (x, g, err, bound)
                worst_re, nre = max(worst_re, float(err.max())), nre + 1
    # S01 and S02 share one set: the same views
    assert b.key(0) == b.key(1) and b.scores(0, 3, 0.99).tobytes() == b.scores(1, 3, 0.99).tobytes()
    assert nsc + nre == 132
    print("largest deviation from the executed reference: scores %.3g (%d items), var_explain %.3g; from the restatement on "
          "the other %d items: scores %.3g; sweeps %d..%d; kernel ms gram %.3f eig %.3f scores %.3f" % (worst_sc, nsc, worst_ve,
                                                        nre, worst_re, b.res.sweeps.min(), b.res.sweeps.max(),
                                                        tm["nr_gram_kernel_ms"], tm["nr_eig_kernel_ms"], tm["nr_scores_kernel_ms"]))


def test_two_calls_give_the_same_bytes(batch, case):
    b, _ = batch
    c = case.reader().batched_components(case.lon, case.lat, "tmax", case.utc, case.day_idx, NC.CUTS, NC.NNGH)
    for k in ("status", "bad_col", "sweeps", "ncomp", "mean", "sd", "var_explain", "eigval", "loadings", "score_off", "scores"):
        assert b.res._out[k].tobytes() == c.res._out[k].tobytes(), k


def _columns(n, p, seed):
    rng = np.random.default_rng(seed)
    lat = rng.standard_normal((n, 6)) * 0.5 ** np.arange(6)
    a = lat.dot(rng.standard_normal((6, p))) + 0.05 * rng.standard_normal((n, p))
    return (5500.0 + 100.0 * a).astype(np.float32)


def _check_item(res, s, g, a, cuts):
    """Item (s, g) of a raw call against the restatement on its matrix a [n, P]."""
    want = RN.components(a, cuts)
    assert res.status[s, g] == want["status"] and res.bad_col[s, g] == want["bad_col"], (s, g, res.status[s, g], want["status"])
    if want["status"] != RN.OK:
        assert (res.ncomp[s, g] == 0).all() and res.scores(s, g).shape[1] == 0 and np.isnan(res.var_explain(s, g)).all()
        return 0.0
    n, p = a.shape
    ve, lam = res.var_explain(s, g), res.eigval(s, g)
    # two float64 routes, each with an error of its own against the exact value: twice the bound
    assert np.abs(ve - want["var_explain"]).max() <= 2 * RN.var_explain_bound(ve, 0.0), (s, g)
    cum_margin = min(np.abs(np.cumsum(want["var_explain"]) - c).min() for c in cuts)
    if cum_margin > 1e-9:
        assert res.ncomp[s, g].tolist() == list(want["ncomp"]), (s, g, res.ncomp[s, g], want["ncomp"])
    k = int(res.ncomp[s, g].max())
    sc = res.scores(s, g)
    assert sc.shape == (n, k)
    # only the components whose eigenvalue stands clear of its neighbours are comparable column by column
    gaps = np.array([min(abs(lam[c] - lam[j]) for j in (c - 1, c + 1) if 0 <= j < p) if p > 1 else lam[0] for c in range(k)])
    ok = gaps > 1e-6 * lam[0]
    err = RN.column_error(want["scores"][:, :k], sc)
    bound = RN.score_bound(lam, sc, np.zeros(k), k)
    assert (err[ok] <= bound[ok]).all(), (s, g, err, bound)
    assert np.abs(res.mean(s, g) - want["mean"]).max() <= 1e-12 * 5600 and np.abs(res.sd(s, g) / want["sd"] - 1).max() <= 1e-12
    # the loadings are orthonormal
    load = res.loadings(s, g)
    assert np.abs(load.dot(load.T) - np.eye(p)).max() < 1e-12
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("p", [1, 8, 32, 33, 64])
def test_edge_shapes(p):
    """P = 1, 8, 32, 33, 64 with groups of 2, 20, 63, 64, 65 and 257 rows, a group without a day and days in no group."""
    from topowx_amd import _qalib
    rows = (2, 20, 63, 64, 65, 257, 0)
    nd = sum(rows) + 9
    grp = np.full(nd, -1, np.int8)
    rng = np.random.default_rng(p)
    free = rng.permutation(nd)
    at = 0
    for g, r in enumerate(rows):
        grp[free[at:at + r]] = g
        at += r
    a = _columns(nd, p, 100 + p)
    res = _qalib.nnr_components_batched(np.ascontiguousarray(a.T), [0, p], np.arange(p), grp, NC.CUTS, ngroups=len(rows))
    assert res.nrows.tolist() == list(rows)
    assert res.status[0, 6] == _qalib.NR_FEW_ROWS and (res.ncomp[0, 6] == 0).all()
    worst = max(_check_item(res, 0, g, a[grp == g], NC.CUTS) for g in range(6))
    one = _qalib.nnr_components_batched(np.ascontiguousarray(a.T), [0, p], np.arange(p), grp, (0.99,), ngroups=len(rows))
    assert one.ncomp.shape == (1, 7, 1) and np.array_equal(one.ncomp[..., 0], res.ncomp[..., 0])
    assert np.array_equal(one.var_explain(0, 5), res.var_explain(0, 5))
    print("P %d: largest error / bound %.3g; sweeps %s" % (p, worst, res.sweeps[0].tolist()))


def test_shared_columns_and_bad_items():
    """Two sets sharing columns; a planted NaN and a constant column give their items a status and leave the others alone."""
    from topowx_amd import _qalib
    nd = 300
    a = _columns(nd, 12, 9)
    grp = (np.arange(nd) % 3).astype(np.int8)
    set_off, set_col = [0, 8, 16, 20], list(range(8)) + list(range(4, 12)) + [0, 5, 9, 11]
    clean = _qalib.nnr_components_batched(np.ascontiguousarray(a.T), set_off, set_col, grp, NC.CUTS)
    for s, cols in enumerate(([*range(8)], [*range(4, 12)], [0, 5, 9, 11])):
        for g in range(3):
            _check_item(clean, s, g, a[grp == g][:, cols], NC.CUTS)
    b = a.copy()
    b[7, 2] = np.nan                                                 # day 7 is in group 1; column 2 is in set 0 only
    b[grp == 2, 10] = 42.0                                           # column 10 is constant on group 2: set 1 only
    bad = _qalib.nnr_components_batched(np.ascontiguousarray(b.T), set_off, set_col, grp, NC.CUTS)
    want = np.zeros((3, 3), np.int32)
    want[0, 1], want[1, 2] = _qalib.NR_NONFINITE, _qalib.NR_CONSTANT
    assert np.array_equal(bad.status, want) and bad.bad_col[0, 1] == 2 and bad.bad_col[1, 2] == 6
    assert (bad.bad_col[want == 0] == -1).all()
    for s in range(3):
        for g in range(3):
            if want[s, g] == 0:
                assert bad.scores(s, g).tobytes() == clean.scores(s, g).tobytes(), (s, g)
                assert bad.var_explain(s, g).tobytes() == clean.var_explain(s, g).tobytes()
            else:
                assert bad.scores(s, g).shape[1] == 0 and (bad.ncomp[s, g] == 0).all()


def test_reader_names_the_bad_column(case):
    c = NC.NnrCase()
    c.data = dict(c.data)
    a = c.data[("uwnd", "18z")].copy()
    a[case.day_idx[4], 0, 1, 1] = 3.0                                # constant in May at the cell (-112.5, 45)
    c.data[("uwnd", "18z")] = a
    b = c.reader().batched_components([-112.4], [44.9], "tmax", [-6], case.day_idx)
    assert b.scores(0, 3, 0.99).shape[1] == b.ncomp(0, 3, 0.99) > 0      # the other months are served
    with pytest.raises(ValueError, match="uwnd18z.*lon -112.5, lat 45.*zero variance.*group 4"):
        b.scores(0, 4, 0.99)                                         # raised when the item is used, as on the host route


# ---- end to end: the batched route against the per-target host route ----
def _kernel_signed(monkeypatch):
    """Turn the host route's score columns to the kernel's sign rule (the largest-magnitude loading positive)."""
    import importlib
    ID, IN = (importlib.import_module("topowx_amd.infill." + k) for k in ("infill_daily", "infill_normals"))
    orig = IN.nnr_components

    def signed(nnr_tair, max_var=0.99):
        sc = orig(nnr_tair, max_var).copy()
        z = RN.standardise(np.asarray(nnr_tair, np.float32))[0]
        load = z.T.dot(sc)                                           # proportional to the loadings
        for k in range(sc.shape[1]):
            if load[int(np.argmax(np.abs(load[:, k]))), k] < 0:
                sc[:, k] = -sc[:, k]
        return sc
    monkeypatch.setattr(ID, "nnr_components", signed)
    monkeypatch.setattr(IN, "nnr_components", signed)


def test_estimate_mean_variance_both_routes():
    """step14 on the emnorm pool (48 stations x 12 months) with reanalysis columns attached: the batched route against the
    host route.  Statuses, widths, component counts and iterations equal; mean and variance within 1e-10."""
    import make_golden_infillmat as mk
    from topowx_amd import _qalib
    from topowx_amd.infill import build_infill_matrices, estimate_mean_variance
    from topowx_amd.qa import StationObsPool
    ids, lon, lat, tmin, days = mk.case_inputs()
    pool = StationObsPool(ids, lon, lat, tmin, tmin + 10, days)
    c, utc = NC.case_over(pool)
    m = build_infill_matrices(pool, "tmin")
    tb, th = {}, {}
    eb = estimate_mean_variance(m, c.reader(), utc, timing=tb)
    eh = estimate_mean_variance(m, NC.OnlyMatrix(c.reader()), utc, timing=th)
    assert tb["nr_calls"] == 1 and "nr_calls" not in th and tb["nr_sets"] < 48
    for k in ("status", "ncols", "ncomp", "iters"):
        assert np.array_equal(getattr(eb, k), getattr(eh, k)), (k, np.argwhere(getattr(eb, k) != getattr(eh, k))[:5])
    ok = np.isin(eb.status, (_qalib.EM_OK, _qalib.EM_MAXITS))
    assert ok.mean() > 0.9 and (eb.ncomp[ok] > 0).mean() > 0.5      # a matrix of 31 station columns takes no score
    sd = np.sqrt(eh.variance[ok])
    dev = max(float((np.abs(eb.mean[ok] - eh.mean[ok]) / sd).max()), float(np.abs(eb.variance[ok] / eh.variance[ok] - 1).max()))
    print("step14, %d items: largest deviation between the routes %.3g; assemble_s batched %.3f host %.3f" % (
        ok.sum(), dev, tb["assemble_s"], th["assemble_s"]))
    assert dev <= EM_TOL


DAILY_KEYS = ("status", "matrix_status", "ncols", "ncomp", "npcs", "nfits", "iters", "attempt", "nattempts", "nonoptimal",
              "retry_fixed", "reasons", "r2_not_reached")


def _compare_daily(a, b, stds, what):
    for k in DAILY_KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k, np.argwhere(getattr(a, k) != getattr(b, k))[:5])
    assert np.array_equal(np.isnan(a.infill_tair), np.isnan(b.infill_tair))
    dev = np.nanmax(np.abs(a.infill_tair - b.infill_tair) / stds[:, None])
    print("%s: largest deviation of a fit between the routes %.3g target standard deviations" % (what, dev))
    assert dev <= FIT_TOL, (what, dev)


def test_infill_daily_chk_perf_both_routes(monkeypatch):
    import chkperf_cases as CC
    from topowx_amd.infill import infill_daily
    from topowx_amd.infill.infill_daily import month_mask_groups
    pool, mean, vari = CC.facade_pool()
    mean, vari = mean.copy(), vari.copy()
    mean[3, 3] = vari[3, 3] = np.nan                                 # station 3 is no neighbour in April: two groups of months
    assert len(month_mask_groups(mean, vari)) == 2
    c, utc = NC.case_over(pool)
    ids = pool.ids[list(CC.FACADE_TARGETS)]
    utc = utc[list(CC.FACADE_TARGETS)]
    stds = np.sqrt(np.nanmean(vari[list(CC.FACADE_TARGETS)], axis=1))
    # the host route as it is: its columns carry LAPACK's signs, which is another PPCA start for a flipped column
    raw = infill_daily(pool, "tmin", ids, mean, vari, NC.OnlyMatrix(c.reader()), utc, ppca_varyexplain=0.75, chk_perf=True)
    _kernel_signed(monkeypatch)
    tb = {}
    a = infill_daily(pool, "tmin", ids, mean, vari, c.reader(), utc, ppca_varyexplain=0.75, chk_perf=True, timing=tb)
    b = infill_daily(pool, "tmin", ids, mean, vari, NC.OnlyMatrix(c.reader()), utc, ppca_varyexplain=0.75, chk_perf=True)
    assert tb["nr_calls"] == 1 and (a.ncomp[a.matrix_status == 0] > 0).all() and (a.nattempts > 1).any()
    _compare_daily(a, b, stds, "step16 with chk_perf")
    # the unpatched host route: the matrices are the same; the kept attempt (and with it ncols and ncomp, which describe
    # the kept attempt) and the components can move with the start.  Where the search and the ladder end alike, widths are
    # equal.  The distance of the fits is REPORTED, not bounded: measured on an MI355X, 31 of 36 items end alike, the fits
    # differ by up to 0.174 target standard deviations there and 0.309 anywhere (this pool has a target with 5 degrees of
    # local noise and a damped half, and ppca_varyexplain is 0.75).  That is far above the 6.0e-3 of DESIGN.md section 18's
    # 200 x 8 example, whose tenfold (6e-2) was first asserted here and missed: the start moves this pool's fits more.
    assert np.array_equal(a.matrix_status, raw.matrix_status)
    same = (a.npcs == raw.npcs) & (a.attempt == raw.attempt)
    for k in ("status", "ncols", "ncomp"):
        assert np.array_equal(getattr(a, k)[same], getattr(raw, k)[same]), k
    month = np.asarray(pool.days["MONTH"]) - 1
    d = np.abs(a.infill_tair - raw.infill_tair) / stds[:, None]
    per_item = np.array([[np.nanmax(d[t, month == g]) for g in range(12)] for t in range(len(ids))])
    print("step16, host route with LAPACK's signs: %d of %d items end with the same components and attempt; largest "
          "deviation of a fit there %.3g, anywhere %.3g target standard deviations" % (same.sum(), same.size,
                                                                                  per_item[same].max(), per_item.max()))
    assert same.mean() >= 0.5


def test_xval_infill_both_routes(monkeypatch):
    import chkperf_cases as CC
    import xvalinfill_cases as XC
    from topowx_amd.infill import XvalInfill, XvalInfillParams
    _kernel_signed(monkeypatch)
    pool, mean, vari = CC.facade_pool()
    c, utc = NC.case_over(pool)
    ids = pool.ids[list(XC.FACADE_XVAL)][:2]
    res = []
    for nnr in (c.reader(), NC.OnlyMatrix(c.reader())):
        params = XvalInfillParams(nnr, 3, 4, 0.99, True, 0, 0.5, 0.75, False)
        res.append(XvalInfill(pool, "tmin", params, mean, vari, ids, XC.FACADE_NTRAIN_YRS, utc_offset=utc).run_all())
    a, b = res
    assert np.array_equal(a.em_status, b.em_status) and np.array_equal(a.held, b.held) and np.array_equal(a.n, b.n)
    sd = np.sqrt(b.em_variance)
    dev = max(float(np.nanmax(np.abs(a.em_mean - b.em_mean) / sd)), float(np.nanmax(np.abs(a.em_variance / b.em_variance - 1))))
    print("step15: largest deviation of the estimates between the routes %.3g" % dev)
    assert dev <= EM_TOL and (a.daily.ncomp > 0).all()
    _compare_daily(a.daily, b.daily, np.sqrt(np.nanmean(b.em_variance, axis=1)), "step15")


def test_command_lines_with_nnr_dir(tmp_path, capsys):
    """step14 --estimate, step16 and step15 with --nnr-dir on a small database: they run, the reports hold non-zero ncomp, and
    step14's values are those of the library route."""
    import json
    import chkperf_cases as CC
    import xvalinfill_cases as XC
    from topowx_amd import ncio, stationdb as sdb, step14, step15, step16
    from topowx_amd.infill import build_infill_matrices, estimate_mean_variance
    pool, mean, vari = CC.facade_pool()
    c, utc = NC.case_over(pool)
    n = pool.ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = pool.ids, pool.lon, pool.lat, 1000.0
    db = str(tmp_path / "all.nc")
    ncio.create_quick_db(db, stns, pool.days, [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                                               ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")], format="NETCDF3_64BIT")
    ds = ncio.open_dataset(db, "a")
    for name, a in (("tmin", pool.tmin), ("tmax", pool.tmax)):
        v = ds.variables[name]
        v.missing_value = np.float32(ncio.FILL_F4)
        v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
    ds.createVariable("utc_offset", "i2", (sdb.STN_ID,), fill_value=ncio.FILL_I2)[:] = utc
    ds.close()
    nnr_dir = c.write(str(tmp_path / "nnr"), "NETCDF3_64BIT")
    targets = pool.ids[list(CC.FACADE_TARGETS)]
    (tmp_path / "t.txt").write_text("\n".join(targets) + "\n")
    out14 = str(tmp_path / "m.npz")
    assert step14.main(["--db", db, "--var", "tmin", "--out", out14, "--estimate", "--nnr-dir", nnr_dir]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    got = np.load(out14)
    want = estimate_mean_variance(build_infill_matrices(pool, "tmin"), c.reader(), utc)
    assert rep["nr_sets"] >= 1 and "nr_eig_kernel_ms" in rep and (got["ncomp"][got["em_status"] == 0] > 0).any()
    assert got["mean"].tobytes() == want.mean.tobytes() and got["ncomp"].tobytes() == want.ncomp.tobytes()
    out16 = str(tmp_path / "d.npz")
    assert step16.main(["--db", db, "--var", "tmin", "--normals", out14, "--out", out16, "--targets", str(tmp_path / "t.txt"),
                        "--chk-perf", "--nnr-dir", nnr_dir]) == 0
    capsys.readouterr()
    d = np.load(out16)
    assert (d["ncomp"][d["matrix_status"] == 0] > 0).all() and np.isfinite(d["infill_tair"]).any()
    np.savez(str(tmp_path / "normals.npz"), ids=pool.ids, mean_tmin=mean, variance_tmin=vari, mean_tmax=mean + 10.0,
             variance_tmax=vari)
    (tmp_path / "x.txt").write_text(str(pool.ids[XC.FACADE_XVAL[0]]) + "\n")
    assert step15.main(["--db", db, "--normals", str(tmp_path / "normals.npz"), "--xval-stnids", str(tmp_path / "x.txt"),
                        "--out", str(tmp_path / "xv.nc"), "--report", str(tmp_path / "xv.npz"),
                        "--ntrain-yrs", str(XC.FACADE_NTRAIN_YRS), "--ppca-varyexplain", "0.75", "--format", "NETCDF3_64BIT",
                        "--nnr-dir", nnr_dir]) == 0
    capsys.readouterr()
    x = np.load(str(tmp_path / "xv.npz"))
    assert (x["ncomp_tmin"] > 0).all() and (x["ncomp_tmax"] > 0).all()
    # ---- without the flag: the outputs of before.  The key sets are those the command lines' own tests expect
    # (tests/test_gpu_emnorm.py, test_gpu_ppca.py, test_gpu_chkperf.py, test_gpu_xvalinfill.py), the bytes those of the
    # library calls with nnr=None, and nothing of the reanalysis (ncols, ncomp, nr_*) shows in a report or a JSON line
    from topowx_amd.infill import XvalInfill, XvalInfillParams, infill_daily
    plain14 = str(tmp_path / "m_plain.npz")
    assert step14.main(["--db", db, "--var", "tmin", "--out", plain14, "--estimate"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any(k.startswith("nr_") for k in line), sorted(line)
    g14 = np.load(plain14)
    assert set(g14.files) == {"ids", "pool_ids", "ymd", "group", "mean", "variance", "em_iters", "em_status"} | set(step14.COLUMNS)
    w14 = estimate_mean_variance(build_infill_matrices(pool, "tmin"))
    for k, a in (("mean", w14.mean), ("variance", w14.variance), ("em_iters", w14.iters), ("em_status", w14.status)):
        assert g14[k].tobytes() == a.tobytes(), k
    assert g14["mean"].tobytes() != got["mean"].tobytes()           # the flag does change the estimate
    plain16 = str(tmp_path / "d_plain.npz")
    assert step16.main(["--db", db, "--var", "tmin", "--normals", plain14, "--out", plain16, "--targets", str(tmp_path / "t.txt"),
                        "--chk-perf"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any(k.startswith("nr_") for k in line), sorted(line)
    g16 = np.load(plain16)
    assert set(g16.files) == {"ids", "ymd", "fnl_tair", "mask_infill", "infill_tair", "mae", "bias"} | \
        set(step16.ITEM_COLUMNS) | set(step16.CHK_COLUMNS)
    w16 = infill_daily(pool, "tmin", targets, g14["mean"], g14["variance"], chk_perf=True)
    for k in ("fnl_tair", "infill_tair", "mask_infill", "mae", "bias") + step16.ITEM_COLUMNS + step16.CHK_COLUMNS:
        assert g16[k].tobytes() == getattr(w16, k).tobytes(), k
    assert step15.main(["--db", db, "--normals", str(tmp_path / "normals.npz"), "--xval-stnids", str(tmp_path / "x.txt"),
                        "--out", str(tmp_path / "xv_plain.nc"), "--report", str(tmp_path / "xv_plain.npz"),
                        "--ntrain-yrs", str(XC.FACADE_NTRAIN_YRS), "--ppca-varyexplain", "0.75", "--format", "NETCDF3_64BIT"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "nr_" not in json.dumps(line) and "ncomp" not in json.dumps(line)
    g15 = np.load(str(tmp_path / "xv_plain.npz"))
    assert set(g15.files) == {"ids", "ymd"} | {"%s_%s" % (k, v) for v in step15.VARS for k in step15.REPORT + step15.REPORT_DAILY}
    params = XvalInfillParams(None, 3, 4, 0.99, True, 0, 0.5, 0.75, False)
    w15 = XvalInfill(pool, "tmin", params, mean, vari, [pool.ids[XC.FACADE_XVAL[0]]], XC.FACADE_NTRAIN_YRS).run_all()
    for k in step15.REPORT:
        assert np.asarray(g15[k + "_tmin"]).tobytes() == np.asarray(getattr(w15, k)).tobytes(), k
    for k in step15.REPORT_DAILY:
        assert g15[k + "_tmin"].tobytes() == getattr(w15.daily, k).tobytes(), k
