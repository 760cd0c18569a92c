"""GPU: step16's ``chk_perf`` -- the kernel of ``twxck_infill_check`` against the numpy restatement
(tests/restate_chkperf.py) on a shape grid, on degenerate items and on the executed-reference golden, for byte equality,
and the retry ladder through ``infill_daily(chk_perf=True)`` and ``python -m topowx_amd.step16 --chk-perf``.

Tolerances: mae, r2 and cpt_stat within 100 x the float64-to-longdouble distance of the restatement
on that item, with floors of N 2^-52 (mae, r2) and N^2 2^-52 (cpt_stat); nobs, nimpossible, reasons, status and cpt_tau
exact.  Every item's inputs are checked first: the restatement's runner-up tmp lies above its minimum by more than twice the
floor (or ties it exactly, where the first-tau rule decides), and every decision margin is above the tolerance.  Every
comparison prints its largest deviation next to its bound.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chkperf_cases as CC  # noqa: E402
import restate_chkperf as RC  # noqa: E402

pytestmark = pytest.mark.gpu
PPCA_FACTOR, PPCA_FLOOR = 100.0, 1e-12          # section 18's bound of a fit, in target standard deviations
VARYEXPLAIN = 0.75                              # the facade pool's ppca_varyexplain: the noisy target's own noise stays out


def compare(res, k, want, n, what, tie_ok=False):
    """Item ``k`` of a library result against a ``check_pair`` record of the restatement; returns the deviations over their
    bounds."""
    assert np.isfinite(max(want["d_mae"], want["d_r2"], want["d_cpt"])), (what, "float64 and longdouble decide differently")
    tm, tr, tc = CC.tolerances(want, n)
    assert want["tmp_gap"] > 2 * n * n * CC.U or (tie_ok and want["tmp_gap"] == 0.0), (what, want["tmp_gap"])
    for name, tol in (("mae", tm / RC.MAE_MAX), ("r2", tr / RC.R2_MIN), ("cpt", tc / abs(want.get("pen", np.nan)))):
        assert not want["margins"].get(name, np.inf) <= tol, (what, name, want["margins"][name], tol)
    for name in ("nobs", "nimpossible", "reasons", "status", "cpt_tau"):
        assert res[name][k] == want[name], (what, name, res[name][k], want[name])
    ratios = []
    for name, tol in (("mae", tm), ("r2", tr), ("cpt_stat", tc)):
        got, ref = float(res[name][k]), float(want[name])
        if np.isnan(ref) or np.isinf(ref):
            assert (np.isnan(got) and np.isnan(ref)) or got == ref, (what, name, got, ref)
            continue
        dev = abs(got - ref)
        print("%s %s: deviation %.3g, bound %.3g" % (what, name, dev, tol))
        assert dev <= tol, (what, name, got, ref, dev, tol)
        ratios.append(dev / tol)
    return ratios


def m_cpt(c):
    return c["margins"].get("cpt", np.inf)


def wants_of(series, pens):
    out = []
    for (name, fit, obs), pen in zip(series, pens):
        with np.errstate(all="ignore"):
            w = RC.check_pair(fit, obs, pen)
        w["pen"] = pen
        out.append(w)
    return out


@pytest.fixture(scope="module")
def grid():
    series = CC.grid_series()
    off, fit, obs = CC.flat(series)
    default = np.array([RC.cpt_penalty(s[1].size) for s in series])
    return series, off, fit, obs, default, wants_of(series, [10.0] * len(series)), wants_of(series, default)


def test_shape_grid(grid):
    """(a) N = 4 .. 8192, iid and with a variance step at tau = 2, N - 2, 64, 256 and N / 2, at pen = 10 and at the default
    penalty (NaN below N = 63), one call each."""
    from topowx_amd import _qalib
    series, off, fit, obs, default, want10, wantd = grid
    tm = {}
    res10 = _qalib.infill_check(off, fit, obs, pen=10.0, timing=tm)
    resd = _qalib.infill_check(off, fit, obs)
    assert np.array_equal(resd["pen"], default, equal_nan=True) and np.isnan(default[0]) and tm["ck_check_kernel_ms"] > 0
    worst = 0.0
    for k, (name, f, o) in enumerate(series):
        worst = max([worst] + compare(res10, k, want10[k], f.size, name + " pen 10") + compare(resd, k, wantd[k], f.size, name))
    nchg = sum(bool(w["reasons"] & RC.VAR_CHGPT) for w in want10), sum(bool(w["reasons"] & RC.VAR_CHGPT) for w in wantd)
    assert len(series) == 60 and 0 < nchg[1] < nchg[0] < len(series)
    hits = [k for k, (name, f, o) in enumerate(series) if "step at" in name and f.size >= 511
            and want10[k]["cpt_tau"] == int(name.split()[-1])]
    assert len(hits) >= 10                                            # the steps are found where they were put
    print("shape grid: %d items, %d / %d change points at pen 10 / default, largest deviation / bound %.3g, kernel %.3f ms"
          % (len(series), nchg[0], nchg[1], worst, tm["ck_check_kernel_ms"]))


def test_degenerate_items():
    """(b) a constant series, two equal minima, nobs 0 and 1, a NaN and an infinity in fit, N = 3, 8193 and 0."""
    from topowx_amd import _qalib
    series = CC.degenerate_series()
    off, fit, obs = CC.flat(series)
    res = _qalib.infill_check(off, fit, obs, pen=10.0)
    want = wants_of(series, [10.0] * len(series))
    for k, (name, f, o) in enumerate(series):
        compare(res, k, want[k], f.size, name, tie_ok=name in ("constant", "mirrored"))
    idx = {s[0]: k for k, s in enumerate(series)}
    k = idx["constant"]
    assert res["cpt_stat"][k] == -np.inf and res["cpt_tau"][k] == 2 and not res["reasons"][k] & RC.VAR_CHGPT
    k = idx["mirrored"]
    assert res["cpt_tau"][k] == 16 and res["reasons"][k] & RC.VAR_CHGPT and res["cpt_stat"][k] == want[k]["cpt_stat"]
    assert res["nobs"][idx["nobs 0"]] == 0 and np.isnan(res["mae"][idx["nobs 0"]]) and np.isnan(res["r2"][idx["nobs 0"]])
    assert res["nobs"][idx["nobs 1"]] == 1 and res["mae"][idx["nobs 1"]] == 0.25 and res["r2"][idx["nobs 1"]] == 0.0
    for name in ("NaN in fit", "inf in fit"):
        assert res["status"][idx[name]] == RC.NOT_FITTED and res["reasons"][idx[name]] == RC.UNFITTED
    assert res["status"][idx["N 3"]] == RC.FEW_ROWS and res["nobs"][idx["N 3"]] == 3 and np.isnan(res["cpt_stat"][idx["N 3"]])
    assert res["status"][idx["N 8193"]] == RC.ROW_CAP and res["reasons"][idx["N 8193"]] == RC.UNFITTED
    assert res["status"][idx["N 0"]] == RC.FEW_ROWS and res["nobs"][idx["N 0"]] == 0 and res["reasons"][idx["N 0"]] == 0
    # a NaN penalty: no change point, the statistic is still reported
    nan = _qalib.infill_check(off, fit, obs, pen=np.nan)
    assert not (nan["reasons"] & RC.VAR_CHGPT).any() and nan["cpt_stat"].tobytes() == res["cpt_stat"].tobytes()
    assert nan["cpt_tau"].tobytes() == res["cpt_tau"].tobytes()


def test_golden_series_through_the_kernel():
    """(c) every attempt the executed reference judged: its reasons exact, its mae and r2 (scipy's) within the bound."""
    from topowx_amd import _qalib
    gold = CC.load_gold()
    run = [(i, a) for i in range(gold["names"].size) for a in range(4) if gold["reasons"][i, a] >= 0]
    series = [("%s attempt %d" % (gold["names"][i], a), gold["series"][i, a], gold["obs"][i]) for i, a in run]
    off, fit, obs = CC.flat(series)
    res = _qalib.infill_check(off, fit, obs)
    assert (res["pen"] == float(gold["pen"])).all()
    want = wants_of(series, res["pen"])
    for k, (i, a) in enumerate(run):
        compare(res, k, want[k], series[k][1].size, series[k][0])
        assert res["reasons"][k] == gold["reasons"][i, a], series[k][0]
        assert abs(res["mae"][k] - gold["mae"][i, a]) <= 1e-12 and abs(res["r2"][k] - gold["r2"][i, a]) <= 1e-12, series[k][0]
    assert len(run) == gold["nattempts"].sum()


def test_bytes_repeat_and_across_batches(grid):
    """(d) a repeated call and a call split into three workspace batches give the same bytes."""
    from topowx_amd import _qalib
    series, off, fit, obs = grid[:4]
    a = _qalib.infill_check(off, fit, obs, pen=10.0)
    b = _qalib.infill_check(off, fit, obs, pen=10.0)
    c = _qalib.infill_check(off, fit, obs, pen=10.0, workspace_bytes=int(off[-1]) * 16 // 3 + 8192 * 16)
    assert a["batches"] == 1 and c["batches"] == 3
    for name in ("nobs", "mae", "r2", "nimpossible", "cpt_stat", "cpt_tau", "reasons", "status"):
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes(), name


# ---- the facade ----
@pytest.fixture(scope="module")
def facade():
    """The pool, the restatement of search, check and ladder per item (CPU, once) and the three facade results."""
    from topowx_amd.infill import infill_daily
    pool, mean, vari = CC.facade_pool()
    items, obs, group = CC.facade_items(pool, mean, vari)
    with np.errstate(all="ignore"):
        wants = [CC.restated_ladder(it, obs, group, max_r2cum=VARYEXPLAIN) for it in items]
    ids = pool.ids[list(CC.FACADE_TARGETS)]
    tmp, tm0, tm1 = {}, {}, {}
    plain = infill_daily(pool, "tmin", ids, mean, vari, ppca_varyexplain=VARYEXPLAIN, timing=tmp)
    off = infill_daily(pool, "tmin", ids, mean, vari, ppca_varyexplain=VARYEXPLAIN, timing=tm0, chk_perf=False)
    on = infill_daily(pool, "tmin", ids, mean, vari, ppca_varyexplain=VARYEXPLAIN, timing=tm1, chk_perf=True)
    return dict(pool=pool, mean=mean, vari=vari, items=items, obs=obs, group=group, wants=wants, plain=plain, off=off, on=on,
                tmp=tmp, tm0=tm0, tm1=tm1)


RESULT_ARRAYS = ("fnl_tair", "infill_tair", "mask_infill", "mae", "bias", "status", "matrix_status", "npcs", "nfits", "iters",
                 "ncols", "ncomp", "item_impossible", "rel", "item_mae", "item_r2", "r2_not_reached")


def test_facade_without_chk_perf_is_unchanged(facade):
    """(e) ``chk_perf=False`` against the same call without the argument: the same bytes, the same timing keys."""
    for name in RESULT_ARRAYS:
        assert getattr(facade["off"], name).tobytes() == getattr(facade["plain"], name).tobytes(), name
    assert facade["off"].calls == facade["plain"].calls and (facade["off"].attempt == -1).all()
    assert (facade["off"].nattempts == 0).all() and (facade["off"].reasons == -1).all()
    assert sorted(facade["tm0"]) == sorted(facade["tmp"]) and not any(k.startswith("ck_") for k in facade["tm0"])
    assert {"pp_fits", "pp_items", "pp_calls", "search_s"} <= set(facade["tm0"]) and "attempt_items" not in facade["tm0"]


def test_facade_with_chk_perf(facade):
    """(f) an ordinary target (done at attempt 0, byte-equal to (e)), one with heavy local noise (low performance at every
    rung: the least-MAE attempt is kept) and one in the half whose later years are damped (a change point at every rung),
    each item against the numpy restatement of search, check and ladder: attempts, reasons and kept attempt exact, the fit
    within section 18's bound, mae / r2 / cpt_stat within this file's.  None is left out."""
    from topowx_amd import _qalib
    r, plain, group, obs = facade["on"], facade["plain"], facade["group"], facade["obs"]
    kinds = {0: [0], 1: [1, 1, 1, 1], 2: [4, 4, 4, 4]}
    seen, worst = 0, 0.0
    for it, w in zip(facade["items"], facade["wants"]):
        t, g = it["t"], it["g"]
        what = "target %d month %d" % (t, g + 1)
        lad = w["ladder"]
        assert w["agree"], (what, "float64 and longdouble decide differently: choose another seed")
        assert lad["reasons"] == kinds[t], (what, lad["reasons"])
        days = np.nonzero(group == g)[0]
        # the decisions are safe: the MAE of the kept attempt lies below the next candidate's by more than the tolerance
        tol_fit = max(PPCA_FACTOR * max(w["d_ref"].values()), PPCA_FLOOR) * it["stds"][0]
        if lad["nonoptimal"]:
            maes = sorted({float(w["checks"][a]["mae"]) for a in lad["attempts"]})
            assert len(maes) == 1 or maes[1] - maes[0] > 2 * tol_fit, (what, maes, tol_fit)
        for a in lad["attempts"]:
            m = w["checks"][a]["margins"]
            assert min(m["mae"] * RC.MAE_MAX, m["r2"] * RC.R2_MIN, m["impossible"] * 50.0) > 10 * tol_fit, (what, a, m)
        assert r.nattempts[t, g] == len(lad["attempts"]) and r.attempt[t, g] == lad["kept"], (what, r.attempt[t, g], lad["kept"])
        assert r.nonoptimal[t, g] == lad["nonoptimal"] and r.retry_fixed[t, g] == lad["retry_fixed"], what
        for a in range(4):
            if a in lad["attempts"]:
                c = w["checks"][a]
                assert r.reasons[t, g, a] == c["reasons"], (what, a, r.reasons[t, g, a], c["reasons"])
                # a mean of absolute values moves by at most the largest deviation of the fit; to first order r2 moves by
                # at most 4 deviations over the smaller standard deviation of the two series (above 0.2 here): 20 deviations
                assert abs(r.attempt_mae[t, g, a] - float(c["mae"])) <= tol_fit, (what, a)
                assert abs(r.attempt_r2[t, g, a] - float(c["r2"])) <= 20 * tol_fit, (what, a)
                assert m_cpt(c) * RC.cpt_penalty(days.size) > 1e-3, (what, a)
            else:
                assert r.reasons[t, g, a] == -1 and np.isnan(r.attempt_mae[t, g, a]), (what, a)
        s = w["searches"][lad["kept"]]
        assert (r.status[t, g], r.npcs[t, g], r.iters[t, g]) == (s["status"], s["npcs"], s["iters"]), (what, r.npcs[t, g], r.iters[t, g], s["npcs"], s["iters"])
        dev = float(np.abs(r.infill_tair[t, days] - s["fit_c"]).max())
        assert dev <= tol_fit, (what, dev, tol_fit)
        worst = max(worst, dev / tol_fit)
        # the check's values of the kept attempt are the kernel's on the facade's own fit
        o = obs[it["col"], days].astype(np.float64)
        mine = RC.check_pair(r.infill_tair[t, days], o, RC.cpt_penalty(days.size))
        k = _qalib.infill_check([0, days.size], r.infill_tair[t, days], o)
        for name, got in (("mae", r.item_mae[t, g]), ("r2", r.item_r2[t, g]), ("cpt_stat", r.cpt_stat[t, g])):
            assert got == k[name][0], (what, name)
        compare(k, 0, dict(mine, pen=RC.cpt_penalty(days.size)), days.size, what + " kept")
        assert r.cpt_tau[t, g] == mine["cpt_tau"] and r.cpt_pen[t, g] == RC.cpt_penalty(days.size) and r.item_impossible[t, g] == 0
        if t == 0:
            assert r.infill_tair[t, days].tobytes() == plain.infill_tair[t, days].tobytes() and r.nfits[t, g] == plain.nfits[t, g]
        elif t == 2:
            assert 0.3 * days.size < r.cpt_tau[t, g] < 0.7 * days.size and r.cpt_stat[t, g] >= r.cpt_pen[t, g]
        seen += 1
    assert seen == 36 == len(facade["items"])
    assert r.fnl_tair[0].tobytes() == plain.fnl_tair[0].tobytes() and r.mae[0] == plain.mae[0]
    assert np.array_equal(r.mask_infill, plain.mask_infill) and (r.nfits[1:] > plain.nfits[1:]).all()
    tm = facade["tm1"]
    assert tm["attempt_items"] == [36, 24, 24, 24] and tm["nonoptimal"] == 24 and tm["retry_fixed"] == 0
    assert tm["ck_calls"] == 3 and tm["ck_check_kernel_ms"] > 0 and tm["pp_fits"] == r.nfits.sum() and r.calls > plain.calls
    print("facade: largest fit deviation / bound %.3g; check kernel %.3f ms over %d calls, pp_upload %.3f ms over %d calls"
          % (worst, tm["ck_check_kernel_ms"], tm["ck_calls"], tm["pp_upload_ms"], tm["pp_calls"]))


def test_step16_chk_perf(tmp_path, capsys, facade):
    """(g) ``step16 --chk-perf`` writes the new columns and report keys; without the flag the keys are what they were."""
    import corrob_cases
    from topowx_amd import step16
    pool, mean, vari = facade["pool"], facade["mean"], facade["vari"]
    db = corrob_cases.write_db(str(tmp_path / "all.nc"), pool.ids, pool.lon, pool.lat, pool.tmin, pool.tmax, pool.days,
                               "NETCDF3_64BIT")
    targets = pool.ids[[CC.FACADE_TARGETS[2]]]
    (tmp_path / "t.txt").write_text("\n".join(targets) + "\n")
    np.savez(str(tmp_path / "normals.npz"), ids=pool.ids, mean=mean, variance=vari)
    args = ["--db", db, "--var", "tmin", "--normals", str(tmp_path / "normals.npz"), "--targets", str(tmp_path / "t.txt")]
    assert step16.main(args + ["--out", str(tmp_path / "plain.npz")]) == 0
    rep0 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert step16.main(args + ["--out", str(tmp_path / "chk.npz"), "--chk-perf"]) == 0
    rep1 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert step16.main(args + ["--out", str(tmp_path / "loose.npz"), "--chk-perf", "--cpt-sig", "0.5"]) == 0
    capsys.readouterr()
    plain, chk, loose = np.load(str(tmp_path / "plain.npz")), np.load(str(tmp_path / "chk.npz")), np.load(str(tmp_path / "loose.npz"))
    base = ["ids", "ymd", "fnl_tair", "mask_infill", "infill_tair", "mae", "bias"] + list(step16.ITEM_COLUMNS)
    assert sorted(plain.files) == sorted(base) and sorted(chk.files) == sorted(base + list(step16.CHK_COLUMNS))
    assert sorted(rep0) == sorted(["var", "stations", "pool", "days", "items", "status", "fits", "calls", "r2_not_reached",
                                   "seconds"] + list(facade["tm0"]))
    assert set(rep1) - set(rep0) == {"attempt_items", "nonoptimal", "retry_fixed", "ck_check_kernel_ms", "ck_upload_ms",
                                     "ck_download_ms", "ck_batches", "ck_calls"}
    assert rep1["items"] == 12 and rep1["attempt_items"] == [int((chk["reasons"][..., a] >= 0).sum()) for a in range(4)]
    assert rep1["attempt_items"][0] == 12 and rep1["nonoptimal"] == int(chk["nonoptimal"].sum())
    assert (chk["nattempts"] >= 1).all() and chk["reasons"].shape == (1, 12, 4) and (chk["cpt_pen"] > 180).all()
    if rep1["nonoptimal"] == 0:
        assert chk["infill_tair"].tobytes() == plain["infill_tair"].tobytes()
    assert (loose["cpt_pen"] < chk["cpt_pen"]).all()
