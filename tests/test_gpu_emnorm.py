"""GPU: step14's mean / variance estimator (``twxem_mean_variance``; ``topowx_amd.infill.infill_normals``) against the numpy
restatement (tests/restate_emnorm.py): on the executed-reference golden matrices (576 items in one call), on the
constructed column-cap pool, on a random pool, on the smallest shapes that can still go wrong, for determinism, and
through the facade and the command line.

``status`` and ``iters`` are compared exactly; mean and variance within 1e-10 (the mean in standard deviations of the target
column, the variance relative): the project's bar for long sums in another order.  An item is left out if ``d_ref`` -- the
distance of the float64 restatement from the ``np.longdouble`` one -- is above 1e-12 or an iteration's delta lies within
1e-6 (relative) of the criterion; none may be left out on the golden, at most 5 % on a random pool.  Every comparison
prints the largest deviation it saw.

Measured (MI355X): see DESIGN.md section 17.
"""
import datetime as dt
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd.dates import MONTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_emnorm as RE  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
D_REF_MAX, MARGIN_MIN = 1e-12, 1e-6


def em_call(x, extra=None, **kw):
    """The library on ONE matrix: ``x`` [n, P] float32 as a target and P - 1 station columns, ``extra`` [n, k] float64."""
    from topowx_amd import _qalib
    x = np.asarray(x, np.float32)
    n, p = x.shape
    sets = [] if extra is None else [(0, extra)]
    return _qalib.em_mean_variance(np.ascontiguousarray(x.T), np.zeros(n, np.int8), [0], [0], [0, p - 1], np.arange(1, p), sets,
                                   None if extra is None else [0], **kw)


def whole(x, extra=None):
    x = np.asarray(x, np.float32).astype(np.float64)
    return x if extra is None else np.concatenate([x, np.asarray(extra, np.float64)], axis=1)


def want_of(x, criterion=1e-4, maxits=1000, longdouble=True):
    """The restatement's record of a matrix: mean, variance, iters, status, sd0, d_ref (the larger of the two), margin."""
    with np.errstate(all="ignore"):
        a = RE.run(x, criterion, maxits)
        d_ref = 0.0
        if longdouble and a["status"] in (RE.OK, RE.MAXITS):
            b = RE.run(x, criterion, maxits, dtype=np.longdouble)
            d_ref = np.inf
            if b["status"] == a["status"] and b["iters"] == a["iters"]:
                d_ref = max(float(abs(a["mean"] - b["mean_ld"]) / a["sd0"]), float(abs(a["variance"] / b["variance_ld"] - 1)))
    a["d_ref"], a["margin"] = d_ref, RE.margin(a["deltas"], criterion)
    return a


def compare(got, i, want, what):
    """Item ``i`` of a library result against a restatement record (or a golden row with the same keys).  Returns
    (deviation, d_ref), or None if the item is left out."""
    if want["margin"] < MARGIN_MIN or not np.isfinite(want["d_ref"]):
        return None
    if want["d_ref"] > D_REF_MAX:                                   # the stop is still comparable, the values are not at 1e-10
        assert got["status"][i] == want["status"] and got["iters"][i] == want["iters"], (what, got["iters"][i], want["iters"])
        print("%s left out: d_ref %.3g; deviation of the mean %.3g, of the variance %.3g" % (
            what, want["d_ref"], abs(got["mean"][i] - want["mean"]) / want["sd0"], abs(got["variance"][i] / want["variance"] - 1)))
        return None
    assert got["status"][i] == want["status"], (what, got["status"][i], want["status"])
    assert got["iters"][i] == want["iters"], (what, got["iters"][i], want["iters"])
    if want["status"] not in (RE.OK, RE.MAXITS):
        assert np.isnan(got["mean"][i]) and np.isnan(got["variance"][i]), what
        return 0.0, 0.0
    dev = max(abs(got["mean"][i] - want["mean"]) / want["sd0"], abs(got["variance"][i] / want["variance"] - 1))
    assert dev <= TOL, (what, dev, want["d_ref"], got["mean"][i], want["mean"], got["variance"][i], want["variance"])
    return float(dev), float(want["d_ref"])


def report(name, devs, nleft=0):
    devs = [d for d in devs if d is not None]
    print("%s: largest deviation %.3g (d_ref there %.3g; largest d_ref %.3g) over %d items, %d left out" % (
        name, max(d[0] for d in devs), max(devs)[1], max(d[1] for d in devs), len(devs), nleft))


def as_items(e):
    return {k: getattr(e, k).ravel() for k in ("mean", "variance", "iters", "delta", "status")}


# ---- the golden: the matrices the executed reference assembled ----
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_emnorm_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_infillmat as mk
    ids, lon, lat, tmin, days = mk.case_inputs()
    assert mk.input_hash(ids, lon, lat, tmin, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    from topowx_amd.qa import StationObsPool
    return StationObsPool(ids, lon, lat, tmin, tmin + 10, days)


@pytest.fixture(scope="module")
def built(case):
    from topowx_amd.infill import build_infill_matrices
    return build_infill_matrices(case, "tmin")


def test_golden(gold, case, built):
    import make_golden_infillmat as mk
    from topowx_amd.infill import estimate_mean_variance
    tm = {}
    e = estimate_mean_variance(built, mk._Nnr(case.days.size), timing=tm)
    assert np.array_equal(e.ncols, gold["width"]) and np.array_equal(e.ncomp, gold["ncomp"])
    assert e.batches == 1 and e.rounds == -(-int(gold["iters"].max()) // 16)
    for k in ("em_prep_kernel_ms", "em_iter_kernel_ms", "em_upload_ms", "em_download_ms", "em_rounds", "em_batches",
              "assemble_s", "em_library_s"):
        assert k in tm and np.isfinite(tm[k]) and tm[k] >= 0, (k, tm)
    got, devs = as_items(e), []
    for i in range(576):
        want = {k: gold[k].ravel()[i] for k in ("mean", "variance", "iters", "status", "sd0", "margin")}
        want["d_ref"] = max(gold["d_ref_mean"].ravel()[i], gold["d_ref_var"].ravel()[i])
        devs.append(compare(got, i, want, divmod(i, 12)))
    assert None not in devs, "no golden item may be left out"
    report("golden", devs)
    print("kernel ms: prep %.3f, iter %.3f, %d launches" % (tm["em_prep_kernel_ms"], tm["em_iter_kernel_ms"], tm["em_rounds"]))


@pytest.mark.parametrize("variant", [0, 1])
def test_column_cap_pool(gold, variant):
    """More than 31 columns: cut to 31 without a reanalysis column (variant 0); a day left without any observation: the
    last column is the first score (variant 1)."""
    import make_golden_emnorm as me
    import make_golden_infillmat as mk
    from topowx_amd.infill import assemble_columns, build_infill_matrices, estimate_mean_variance
    from topowx_amd.qa import StationObsPool
    ids, lon, lat, tmin, days = me.cap_inputs(variant)
    assert mk.input_hash(ids, lon, lat, tmin, days) == str(gold["cap%d_input_hash" % variant])
    pool = StationObsPool(ids, lon, lat, tmin, tmin + 10, days)
    m = build_infill_matrices(pool, "tmin", [ids[0]], None, "all")
    assert m.status[0, 0] == 0 and int(m.keep.sum()) == me.CAP_NNGH
    e = estimate_mean_variance(m, mk._Nnr(days.size))
    used = bool(gold["cap%d_used_score" % variant])
    assert used == (variant == 1) and e.ncols[0, 0] == 31 and e.ncomp[0, 0] == int(used)
    cols, _ = assemble_columns(m, 0, 0, None if not used else np.zeros((days.size, 2)))
    assert np.array_equal(mk.matrix_hash(tmin[:, np.concatenate([[0], cols])].astype(np.float64)), gold["cap%d_hash" % variant])
    want = {k: gold["cap%d_%s" % (variant, k)][()] for k in ("mean", "variance", "iters", "status", "sd0", "margin")}
    want["d_ref"] = max(gold["cap%d_d_ref_mean" % variant][()], gold["cap%d_d_ref_var" % variant][()])
    dev = compare(as_items(e), 0, want, variant)
    assert dev is not None
    report("cap pool, variant %d" % variant, [dev])


# ---- a random pool ----
@pytest.fixture(scope="module")
def random_case():
    from test_gpu_infillmat import random_pool
    from topowx_amd.infill import build_infill_matrices
    pool, rs = random_pool(31, 80, dt.date(2001, 1, 1), dt.date(2003, 12, 31))
    targets = np.sort(rs.choice(80, 16, replace=False))
    return pool, build_infill_matrices(pool, "tmin", pool.ids[targets])


def test_restatement_on_a_random_pool(random_case):
    from topowx_amd.infill import estimate_mean_variance
    pool, m = random_case
    e = estimate_mean_variance(m)
    got, devs, nok = as_items(e), [], 0
    for t in range(len(m.target_ids)):
        for g in range(12):
            i = t * 12 + g
            if m.status[t, g] != 0:
                assert e.status[t, g] == RE.NO_MATRIX and np.isnan(e.mean[t, g]) and e.ncols[t, g] == 0
                continue
            nok += 1
            x = m.matrix(t, g)
            assert e.ncols[t, g] == x.shape[1] and e.ncomp[t, g] == 0
            devs.append(compare(got, i, want_of(x), (t, g)))
    left = sum(d is None for d in devs)
    assert nok > 150 and left <= 0.05 * nok
    report("random pool 80 x 3 years", devs, left)


def test_same_bytes_whatever_the_launches_and_batches(random_case):
    from topowx_amd.infill import estimate_mean_variance
    pool, m = random_case
    first = estimate_mean_variance(m)
    rows = sum(int((m.group == g).sum()) for g in range(12)) * len(m.target_ids)
    budget = (rows * 8 + m.status.size * 9000) // 3 + 9000
    runs = {"again": estimate_mean_variance(m), "one iteration per launch": estimate_mean_variance(m, iters_per_launch=1),
            "three batches": estimate_mean_variance(m, workspace_bytes=budget)}
    assert first.batches == 1 and runs["three batches"].batches >= 3
    assert runs["one iteration per launch"].rounds == int(first.iters.max()) > first.rounds
    for name, e in runs.items():
        for k in ("mean", "variance", "iters", "delta", "status"):
            assert getattr(e, k).tobytes() == getattr(first, k).tobytes(), (name, k)


# ---- the smallest shapes ----
def shape_matrix(n, p, seed, missing=0.12):
    rs = np.random.RandomState(seed)
    x = np.round(rs.randn(n, 1) * 3.0 + rs.randn(n, p) * 2.0 + 10.0 * rs.rand(p)[None, :], 1)
    x[rs.rand(n, p) < missing] = np.nan
    return x.astype(np.float32)


@pytest.mark.parametrize("p", [1, 2, 31])
def test_smallest_shapes(p):
    devs, statuses = [], set()
    for n in (1, 63, 64, 65, 255, 256, 257):
        x = shape_matrix(n, p, 100 * p + n, missing=0.03 if p == 31 and n < 100 else 0.12)   # (few rows: well conditioned)
        got = em_call(x)
        want = want_of(whole(x))
        statuses.add(want["status"])
        devs.append(compare(got, 0, want, (n, p)))
    left = sum(d is None for d in devs)
    print("P = %d: statuses %s" % (p, sorted(statuses)))
    assert left <= 1 and RE.OK in statuses
    report("rows 1 .. 257, P = %d" % p, devs, left)


def test_more_than_31_columns_fail_the_call():
    from topowx_amd import _qalib
    x = shape_matrix(64, 32, 1)
    with pytest.raises(_qalib.QaError, match="TWXEM_MAX_COLS"):
        em_call(x)
    with pytest.raises(_qalib.QaError, match="TWXEM_MAX_COLS"):
        em_call(x[:, :30], extra=np.ones((64, 2)))


def test_complete_rows_take_two_iterations():
    rs = np.random.RandomState(2)
    x = np.round(rs.randn(257, 7) @ rs.randn(7, 7) + 3.0, 2).astype(np.float32)
    got = em_call(x, full=True)
    x = x.astype(np.float64)
    assert got["status"][0] == RE.OK and got["iters"][0] == 2
    assert abs(got["mean"][0] - x[:, 0].mean()) <= 1e-12 * x[:, 0].std() * 100
    assert abs(got["variance"][0] / x[:, 0].var() - 1) <= 1e-12
    assert np.abs(got["mu"][0, :7] - x.mean(axis=0)).max() <= 1e-12 and np.isnan(got["mu"][0, 7:]).all()
    cov = np.cov(x.T, bias=True)
    assert np.abs(got["sigma"][0, :7, :7] - cov).max() <= 1e-10 * np.abs(cov).max() and np.isnan(got["sigma"][0, 7:]).all()
    assert np.isnan(got["sigma"][0, :, 7:]).all()


def pattern_cases():
    out = {"a_single_pattern": shape_matrix(200, 5, 7, missing=0.0)}
    two = shape_matrix(200, 5, 8, missing=0.0)
    two[1::2, 0] = np.nan                                          # the target is missing on every other row
    out["two_patterns"] = two
    own = shape_matrix(31, 6, 9, missing=0.0)                      # 31 rows, 31 different masks of 5 columns
    for r in range(31):
        for c in range(5):
            if not (r + 1) >> c & 1:
                own[r, 1 + c] = np.nan
    out["every_row_its_own_pattern"] = own
    empty = shape_matrix(120, 4, 10)
    empty[[5, 77, 119]] = np.nan
    out["rows_with_nothing_observed"] = empty
    out["forty_rows_31_columns"] = shape_matrix(40, 31, 12, missing=0.2)
    return out


PATTERNS = pattern_cases()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_patterns(name):
    x = PATTERNS[name]
    got = em_call(x)
    want = want_of(whole(x))
    print("%s: status %d, %d iterations (restated %d), d_ref %.3g, margin %.3g" % (
        name, got["status"][0], got["iters"][0], want["iters"], want["d_ref"], want["margin"]))
    assert want["status"] == RE.OK
    if name == "forty_rows_31_columns":
        assert want["iters"] > 100
    if name == "every_row_its_own_pattern":
        assert np.unique(RE.patterns(np.isfinite(x))[0]).size == 31
    dev = compare(got, 0, want, name)
    # rows close to columns: the float64 restatement itself is 3e-11 from the longdouble one, so the values are not
    # comparable at 1e-10 (compare() has checked status and iterations and printed the deviation)
    assert (dev is None) == (name == "forty_rows_31_columns")
    if dev is not None:
        report(name, [dev])


def test_monotone_closed_form():
    import make_golden_emnorm as me
    x = me.monotone_case().astype(np.float32)
    mean, var = me.monotone_closed_form(x.astype(np.float64))
    got = em_call(x, criterion=1e-12, maxits=100000)
    assert got["status"][0] == RE.OK
    print("monotone: %d iterations, mean off by %.3g, variance by %.3g (relative)" % (
        got["iters"][0], abs(got["mean"][0] - mean), abs(got["variance"][0] / var - 1)))
    assert abs(got["mean"][0] - mean) <= 1e-10 * np.sqrt(var) and abs(got["variance"][0] / var - 1) <= 1e-10


def test_statuses():
    from topowx_amd import _qalib
    x = shape_matrix(100, 4, 12, missing=0.0)
    const = x.copy()
    const[:, 2] = 5.0
    got = em_call(const)
    want = want_of(whole(const))
    assert want["status"] == RE.NUMERIC and got["status"][0] == RE.NUMERIC and got["iters"][0] == want["iters"] == 1
    assert np.isnan(got["mean"][0]) and np.isnan(got["variance"][0]) and np.isnan(got["delta"][0])
    nan = x.copy()
    nan[:, 3] = np.nan
    got = em_call(nan)
    assert got["status"][0] == RE.EMPTY_COLUMN and np.isnan(got["mean"][0]) and got["iters"][0] == 0
    gaps = shape_matrix(100, 4, 13)
    got = em_call(gaps, maxits=3)
    want = want_of(whole(gaps), maxits=3)
    assert got["status"][0] == RE.MAXITS == want["status"] and got["iters"][0] == 3
    dev = compare(got, 0, want, "maxits")
    assert dev is not None
    report("maxits = 3", [dev])
    assert abs(got["delta"][0] / want["delta"] - 1) <= 1e-8
    # a non-OK matrix item among good ones
    obs = np.ascontiguousarray(gaps.T)
    r = _qalib.em_mean_variance(obs, np.zeros(100, np.int8), [0, 0, 0], [0, 0, 0], [0, 3, 6, 9], [1, 2, 3] * 3,
                                matrix_status=[0, 19, 0])
    assert r["status"].tolist() == [RE.OK, RE.NO_MATRIX, RE.OK] and np.isnan(r["mean"][1]) and r["iters"][1] == 0
    assert r["mean"][0] == r["mean"][2] and r["variance"][0] == r["variance"][2]
    for kw in (dict(criterion=0.0), dict(criterion=-1.0), dict(maxits=0)):
        with pytest.raises(_qalib.QaError, match="criterion and maxits"):
            em_call(gaps, **kw)
    with pytest.raises(_qalib.QaError, match="column index"):
        _qalib.em_mean_variance(obs, np.zeros(100, np.int8), [0], [0], [0, 1], [4])


def test_row_cap():
    from topowx_amd import _qalib
    n = _qalib.EM_MAX_ROWS + 1
    rs = np.random.RandomState(3)
    x = np.round(rs.randn(n, 1) * 3 + rs.randn(n, 3), 1).astype(np.float32)
    x[rs.rand(n, 3) < 0.1] = np.nan
    got = em_call(x)
    assert got["status"][0] == RE.ROW_CAP and np.isnan(got["mean"][0]) and np.isnan(got["variance"][0])
    got = em_call(x[:-1])                                          # exactly the cap: estimated
    dev = compare(got, 0, want_of(whole(x[:-1])), "rows = cap")
    assert dev is not None
    report("rows = TWXEM_MAX_ROWS", [dev])


def test_an_extra_column_set_shared_by_two_items():
    from topowx_amd import _qalib
    rs = np.random.RandomState(4)
    x = shape_matrix(90, 5, 14)
    extra = rs.randn(90, 2) + np.nan_to_num(x[:, 1:3].astype(np.float64)) * 0.2
    obs = np.ascontiguousarray(x.T)
    # item 0: target 0 with stations 1, 2; item 1: target 3 with station 4; both with the set; item 2: as item 0, no set
    r = _qalib.em_mean_variance(obs, np.zeros(90, np.int8), [0, 3, 0], [0, 0, 0], [0, 2, 3, 5], [1, 2, 4, 1, 2],
                                [(0, extra)], [0, 0, -1])
    x64 = x.astype(np.float64)
    devs = [compare(r, 0, want_of(np.concatenate([x64[:, :3], extra], axis=1)), "item 0"),
            compare(r, 1, want_of(np.concatenate([x64[:, 3:5], extra], axis=1)), "item 1"),
            compare(r, 2, want_of(x64[:, :3]), "item 2")]
    assert None not in devs and r["mean"][0] != r["mean"][2]
    report("a shared extra-column set", devs)


# ---- facade and command line ----
def test_facade(case, built):
    from topowx_amd.infill import build_infill_matrices, estimate_mean_variance, infill_mean_variance
    t = 30
    m = build_infill_matrices(case, "tmin", [case.ids[t], case.ids[2]])
    e = estimate_mean_variance(m)
    masks = [case.days[MONTH] == g + 1 for g in range(12)]
    mean, var = infill_mean_variance(case.ids[t], case, np.ones(48, bool), "tmin", day_masks=masks)
    assert mean.tobytes() == e.mean[0].tobytes() and var.tobytes() == e.variance[0].tobytes()
    mean1, var1 = infill_mean_variance(case.ids[t], case, np.ones(48, bool), "tmin", day_masks=[masks[6], masks[6] | masks[7]])
    assert mean1[0] == e.mean[0, 6] and var1[0] == e.variance[0, 6] and np.isfinite(mean1[1])
    a, b = infill_mean_variance(case.ids[2], case, None, "tmin")
    assert isinstance(a, float) and np.isfinite(a) and b > 0
    with pytest.raises(NotImplementedError):
        infill_mean_variance(case.ids[t], case, None, "tmin", tair_mask=np.zeros(case.days.size, bool))


def test_step14_estimate(tmp_path, capsys):
    import corrob_cases
    from test_gpu_infillmat import random_pool
    from topowx_amd import step14
    from topowx_amd.infill import build_infill_matrices, estimate_mean_variance
    pool, rs = random_pool(21, 30, dt.date(2001, 1, 1), dt.date(2002, 12, 31), box=(1.0, 0.7))
    db = corrob_cases.write_db(str(tmp_path / "all.nc"), pool.ids, pool.lon, pool.lat, pool.tmin, pool.tmax, pool.days,
                               "NETCDF3_64BIT")
    targets = pool.ids[[0, 1, 7, 29]]
    (tmp_path / "t.txt").write_text("\n".join(targets) + "\n")
    out = str(tmp_path / "m.npz")
    assert step14.main(["--db", db, "--var", "tmin", "--out", out, "--targets", str(tmp_path / "t.txt"), "--estimate"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = estimate_mean_variance(build_infill_matrices(pool, "tmin", targets))
    got = np.load(out)
    for k, a in (("mean", want.mean), ("variance", want.variance), ("em_iters", want.iters), ("em_status", want.status)):
        assert got[k].tobytes() == a.tobytes(), k
    assert sum(rep["em_status"].values()) == 48 and rep["em_status"].get("ok", 0) == int((want.status == 0).sum()) > 0
    assert "em_iter_kernel_ms" in rep and "em_prep_kernel_ms" in rep and rep["em_rounds"] >= 1
    assert step14.main(["--db", db, "--var", "tmin", "--out", out, "--targets", str(tmp_path / "t.txt")]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any(k.startswith("em_") for k in plain) and "mean" not in np.load(out).files
