"""CPU: step14's mean / variance estimator without a GPU -- the header, the binding and the status numbers, the host-side
column assembly (``assemble_columns``, ``nnr_components``) against the executed-reference golden
(tests/golden/make_golden_emnorm.py), argument validation, and the numpy restatement (tests/restate_emnorm.py) itself: a
slice of the golden, its known answers, and the monotone observed-data log-likelihood."""
import os
import re
import sys

import numpy as np
import pytest

from topowx_amd.dates import MONTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_emnorm as RE  # noqa: E402

NEW_KERNELS = ("k_em_prep", "k_em_iter")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_emnorm_v1.npz"))


@pytest.fixture(scope="module")
def gold_mat():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_infillmat_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_infillmat as mk
    ids, lon, lat, tmin, days = mk.case_inputs()
    assert mk.input_hash(ids, lon, lat, tmin, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    from topowx_amd.qa import StationObsPool
    return StationObsPool(ids, lon, lat, tmin, tmin + 10, days)


def matrices_of(pool, res, targets, group, ngroups):
    """An ``InfillMatrices`` from recorded ranked lists (no GPU)."""
    from topowx_amd.infill import InfillMatrices
    nt = len(targets)
    full = dict(status=np.zeros((nt, ngroups), np.int32), nnghs=np.zeros((nt, ngroups), np.int32),
                max_dist=np.full((nt, ngroups), 75.0), ioa=np.zeros(res["idx"].size), dist=np.zeros(res["idx"].size),
                nlap=np.zeros(res["idx"].size, np.int32), nlap_stn=np.zeros(res["idx"].size, np.int32), rounds=1)
    full.update(res)
    return InfillMatrices(pool, "tmin", pool.ids[targets], np.asarray(targets, np.int32), group, ngroups, full,
                          np.zeros(ngroups, np.int32), np.zeros((nt, ngroups), np.int32), 3)


def test_golden_file(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_emnorm_v1.npz")) < 1024 * 1024
    assert gold["mean"].shape == (48, 12) and (gold["status"] == 0).all()
    assert max(gold["d_ref_mean"].max(), gold["d_ref_var"].max()) <= 1e-12 and gold["margin"].min() >= 1e-6
    assert gold["iters"].min() >= 2 and (gold["iters_conv"] >= gold["iters"]).all()
    # what stays unpinned: where criterion 1e-4 stops against the fixed point
    dm = np.abs(gold["mean"] - gold["mean_conv"]) / gold["sd0"]
    dv = np.abs(gold["variance"] / gold["variance_conv"] - 1)
    assert dm.max() < 1e-3 and dv.max() < 1e-3 and np.median(dm) < 1e-5


def test_header_and_binding():
    from topowx_amd import _qalib, infill
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxem_\w+)\s*\(", h))) == sorted(_qalib.EM_EXPORTS) == ["twxem_mean_variance"]
    for macro, val in (("TWXEM_MAXITS", _qalib.EM_MAXITS), ("TWXEM_NO_MATRIX", _qalib.EM_NO_MATRIX),
                       ("TWXEM_EMPTY_COLUMN", _qalib.EM_EMPTY_COLUMN), ("TWXEM_ROW_CAP", _qalib.EM_ROW_CAP),
                       ("TWXEM_MAX_ROWS", _qalib.EM_MAX_ROWS), ("TWXEM_NKERNELS", len(_qalib.EM_KERNELS)),
                       ("TWXEM_NTIMES", len(_qalib.EM_KERNELS) + len(_qalib.EM_HOST_TIMES))):
        m = re.search(r"#define %s (\d+)" % macro, h)
        assert m and int(m.group(1)) == val, macro
    assert "#define TWXEM_NUMERIC TWX_CELL_NUMERIC" in h and "#define TWXEM_OK TWX_CELL_OK" in h
    assert "#define TWXEM_MAX_COLS TWXIF_MAX_COLS_NORM_IMPUTE" in h and _qalib.EM_MAX_COLS == _qalib.IF_MAX_COLS_NORM_IMPUTE
    assert _qalib.EM_MAX_ROWS >= 4216
    assert (_qalib.EM_OK, _qalib.EM_NUMERIC, _qalib.EM_MAXITS, _qalib.EM_NO_MATRIX, _qalib.EM_EMPTY_COLUMN,
            _qalib.EM_ROW_CAP) == (0, 4, 20, 21, 22, 23) == (RE.OK, RE.NUMERIC, RE.MAXITS, RE.NO_MATRIX, RE.EMPTY_COLUMN,
                                                            RE.ROW_CAP)
    assert sorted(infill.EM_STATUS) == [0, 4, 20, 21, 22, 23] and sorted(infill.ITEM_STATUS) == [0, 4, 7, 18, 19]
    assert infill.InfillEstimates.EM_STATUS is infill.EM_STATUS
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_emnorm.hip" in build
    # every unit of topowx_amd/qa is named in the build script exactly once, and nothing that is not there
    named = re.findall(r"topowx_amd/qa/(twx_\w+\.hip)", build)
    on_disk = [f for f in os.listdir(os.path.join(ROOT, "topowx_amd", "qa")) if re.fullmatch(r"twx_\w+\.hip", f)]
    assert sorted(named) == sorted(on_disk) and len(set(named)) == len(named)
    assert build.count("topowx_amd/csrc/twx_hip.hip") == 1
    for name in ("assemble_columns", "nnr_components", "estimate_mean_variance", "infill_mean_variance", "InfillEstimates"):
        assert name in infill.__all__ and hasattr(infill, name)


def test_assembly_reproduces_the_golden(gold, gold_mat, case):
    """Widths, the number of score columns and the score columns themselves (up to sign) of all 576 reference matrices."""
    import make_golden_infillmat as mk
    from topowx_amd.infill import assemble_columns, nnr_components
    grp = (case.days[MONTH] - 1).astype(np.int8)
    m = matrices_of(case, dict(off=gold_mat["off"], idx=gold_mat["idx"], keep=gold_mat["keep"], nnghs=gold_mat["nnghs"]),
                    np.arange(48), grp, 12)
    nnr = mk._Nnr(case.days.size).m
    scores = [nnr_components(nnr[grp == g]) for g in range(12)]
    for t in range(48):
        for g in range(12):
            cols, extra = assemble_columns(m, t, g, scores[g])
            assert 1 + cols.size + extra.shape[1] == gold["width"][t, g] and extra.shape[1] == gold["ncomp"][t, g], (t, g)
            assert cols.size == gold_mat["matrix_ncols"][t, g] and np.array_equal(cols, m.columns(t, g))
            nost, none = assemble_columns(m, t, g)
            assert np.array_equal(nost, cols) and none.shape == (extra.shape[0], 0)
    for t, g in gold_mat["full_items"]:
        want = gold["scores_%d_%d" % (t, g)]
        _, extra = assemble_columns(m, t, g, scores[g])
        assert extra.shape == want.shape
        for c in range(want.shape[1]):
            scale = np.abs(want[:, c]).max()
            assert min(np.abs(extra[:, c] - want[:, c]).max(), np.abs(extra[:, c] + want[:, c]).max()) <= 1e-9 * scale


@pytest.mark.parametrize("variant", [0, 1])
def test_assembly_cap_branches(gold, variant):
    """36 kept stations: the matrix is cut to 31 columns without a score; where that leaves a day without any
    observation the last column becomes the first score (the ranking of the constructed pool follows the column number,
    which the maker asserted on the executed reference)."""
    import make_golden_emnorm as me
    import make_golden_infillmat as mk
    from topowx_amd.infill import assemble_columns, nnr_components
    from topowx_amd.qa import StationObsPool
    ids, lon, lat, tmin, days = me.cap_inputs(variant)
    assert mk.input_hash(ids, lon, lat, tmin, days) == str(gold["cap%d_input_hash" % variant])
    pool = StationObsPool(ids, lon, lat, tmin, tmin + 10, days)
    n = me.CAP_NNGH
    m = matrices_of(pool, dict(off=np.array([0, n], np.int64), idx=np.arange(1, n + 1, dtype=np.int32),
                               keep=np.ones(n, np.uint8), nnghs=np.full((1, 1), n, np.int32)), [0],
                    np.zeros(days.size, np.int8), 1)
    scores = nnr_components(mk._Nnr(days.size).m)
    cols, extra = assemble_columns(m, 0, 0, scores)
    used = bool(gold["cap%d_used_score" % variant])
    assert used == (variant == 1)
    assert 1 + cols.size + extra.shape[1] == int(gold["cap%d_width" % variant]) == 31
    assert extra.shape[1] == int(used) and cols.tolist() == list(range(1, 30 if used else 31))
    assert np.array_equal(mk.matrix_hash(tmin[:, np.concatenate([[0], cols])].astype(np.float64)), gold["cap%d_hash" % variant])
    if used:
        assert np.array_equal(extra[:, 0], scores[:, 0])
        x = np.concatenate([tmin[:, :31].astype(np.float64)], axis=1)
        assert np.isfinite(x).sum(axis=1).min() == 0
    cols, extra = assemble_columns(m, 0, 0)                          # no reanalysis source: cut to 31 columns, nothing else
    assert cols.tolist() == list(range(1, 31)) and extra.shape[1] == 0
    # the restatement on the matrix as assembled here reproduces the recorded estimate
    cols, extra = assemble_columns(m, 0, 0, scores)
    r = RE.run(np.concatenate([tmin[:, np.concatenate([[0], cols])].astype(np.float64), extra], axis=1))
    assert r["iters"] == int(gold["cap%d_iters" % variant]) and abs(r["mean"] - gold["cap%d_mean" % variant]) <= 1e-9


def test_nnr_components():
    from topowx_amd.infill import nnr_components
    rs = np.random.RandomState(3)
    base = rs.randn(200, 1)
    a = np.concatenate([base + 0.01 * rs.randn(200, 1) for _ in range(4)], axis=1) * np.array([1.0, 5.0, 0.1, 2.0]) + 270.0
    s = nnr_components(a)
    assert s.shape == (200, 1)                                       # four near copies: one component explains 99 %
    assert nnr_components(rs.randn(200, 4)).shape == (200, 4) and nnr_components(rs.randn(200, 4), 0.2).shape[1] <= 2
    assert abs(s[:, 0].mean()) < 1e-9
    for bad in (np.zeros(5), np.zeros((1, 4)), np.zeros((5, 0))):
        with pytest.raises(ValueError):
            nnr_components(bad)


def test_argument_validation(case, gold_mat):
    from topowx_amd import _qalib
    from topowx_amd.infill import assemble_columns, infill_mean_variance
    grp = (case.days[MONTH] - 1).astype(np.int8)
    m = matrices_of(case, dict(off=gold_mat["off"], idx=gold_mat["idx"], keep=gold_mat["keep"], nnghs=gold_mat["nnghs"]),
                    np.arange(48), grp, 12)
    with pytest.raises(ValueError, match="nnr_scores"):
        assemble_columns(m, 0, 0, np.zeros((5, 2)))
    with pytest.raises(IndexError):
        assemble_columns(m, 0, 12)
    with pytest.raises(NotImplementedError, match="step15"):
        infill_mean_variance(case.ids[0], case, None, "tmin", tair_mask=np.zeros(case.days.size, bool))
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    with pytest.raises(ValueError, match="day_masks"):
        infill_mean_variance(case.ids[0], case, None, "tmin", day_masks=[np.ones(5, bool)])
    obs = np.zeros((3, 10), np.float32)
    g = np.zeros(10, np.int8)
    for kw in (dict(obs=obs[0]), dict(group=g[:9]), dict(item_group=[0, 0]), dict(col_off=[0, 2]), dict(col_off=[1, 2]),
               dict(item_set=[0, 0]), dict(matrix_status=[0, 0]), dict(sets=[(0, np.zeros((9, 1)))]),
               dict(sets=[(1, np.zeros((10, 1)))]), dict(sets=[(0, np.zeros(10))])):
        with pytest.raises(ValueError):
            _qalib.em_mean_variance(**dict(dict(obs=obs, group=g, item_target=[0], item_group=[0], col_off=[0, 1], col_idx=[1]),
                                           **kw))


def test_entry_rejects_bad_arguments_before_any_device_work():
    """Call-level failures (the library is needed, a GPU is not)."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    obs = np.zeros((40, 10), np.float32)
    g = np.zeros(10, np.int8)
    ok = dict(obs=obs, group=g, item_target=[0], item_group=[0], col_off=[0, 2], col_idx=[1, 2])
    with pytest.raises(_qalib.QaError, match="TWXEM_MAX_COLS"):
        _qalib.em_mean_variance(**dict(ok, col_off=[0, 31], col_idx=np.arange(1, 32)))
    with pytest.raises(_qalib.QaError, match="TWXEM_MAX_COLS"):
        _qalib.em_mean_variance(**dict(ok, col_off=[0, 29], col_idx=np.arange(1, 30), sets=[(0, np.zeros((10, 2)))], item_set=[0]))
    with pytest.raises(_qalib.QaError, match="column index"):
        _qalib.em_mean_variance(**dict(ok, col_idx=[1, 40]))
    with pytest.raises(_qalib.QaError, match="target"):
        _qalib.em_mean_variance(**dict(ok, item_target=[40]))
    with pytest.raises(_qalib.QaError, match="extra-column set"):
        _qalib.em_mean_variance(**dict(ok, item_set=[0]))
    for kw in (dict(criterion=0.0), dict(criterion=float("nan")), dict(maxits=0), dict(maxits=-3)):
        with pytest.raises(_qalib.QaError, match="criterion and maxits"):
            _qalib.em_mean_variance(**dict(ok, **kw))


def test_restatement_reproduces_a_slice_of_the_golden(gold, gold_mat, case):
    """48 items (every station, one month each) from the matrices assembled here."""
    import make_golden_infillmat as mk
    from topowx_amd.infill import assemble_columns, nnr_components
    grp = (case.days[MONTH] - 1).astype(np.int8)
    m = matrices_of(case, dict(off=gold_mat["off"], idx=gold_mat["idx"], keep=gold_mat["keep"], nnghs=gold_mat["nnghs"]),
                    np.arange(48), grp, 12)
    nnr = mk._Nnr(case.days.size).m
    worst = 0.0
    for t in range(48):
        g = (5 * t) % 12
        cols, extra = assemble_columns(m, t, g, nnr_components(nnr[grp == g]))
        x = np.concatenate([case.tmin[np.ix_(grp == g, np.concatenate([[t], cols]))].astype(np.float64), extra], axis=1)
        r = RE.run(x)
        assert r["status"] == gold["status"][t, g] and r["iters"] == gold["iters"][t, g], (t, g)
        worst = max(worst, abs(r["mean"] - gold["mean"][t, g]) / gold["sd0"][t, g], abs(r["variance"] / gold["variance"][t, g] - 1))
    assert worst <= 1e-10, worst


def test_restatement_known_answers():
    import make_golden_emnorm as me
    rs = np.random.RandomState(1)
    x = rs.randn(100, 5) @ rs.randn(5, 5) + 3.0
    r = RE.run(x, full=True)
    assert r["iters"] == 2 and abs(r["mean"] - x[:, 0].mean()) < 1e-12 and abs(r["variance"] - x[:, 0].var()) < 1e-12
    assert np.abs(r["sigma"] - np.cov(x.T, bias=True)).max() < 1e-11
    one = x[:, :1].copy()
    one[::3] = np.nan
    r = RE.run(one)
    assert r["iters"] == 1 and abs(r["mean"] - np.nanmean(one)) < 1e-12 and abs(r["variance"] - np.nanvar(one)) < 1e-12
    const = x.copy()
    const[:, 2] = 5.0
    r = RE.run(const)
    assert r["status"] == RE.NUMERIC and r["iters"] == 1 and np.isnan(r["mean"])       # a pivot of exactly 0 in iteration 2
    x[:, 4] = np.nan
    assert RE.run(x)["status"] == RE.EMPTY_COLUMN
    m = me.monotone_case()
    mean, var = me.monotone_closed_form(m)
    r = RE.run(m, 1e-12, 100000)
    assert r["status"] == RE.OK and abs(r["mean"] - mean) < 1e-10 and abs(r["variance"] / var - 1) < 1e-10
    assert RE.run(m, maxits=3)["status"] == RE.MAXITS
    for kw in (dict(criterion=0), dict(maxits=0)):
        with pytest.raises(ValueError):
            RE.run(m, **kw)
    with pytest.raises(ValueError):
        RE.run(np.zeros((5, 32)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_observed_data_likelihood_never_decreases(seed):
    rs = np.random.RandomState(seed)
    n, p = 150, 6
    x = rs.randn(n, 1) * 2.0 + rs.randn(n, p) @ rs.randn(p, p) + 4.0
    x[rs.rand(n, p) < 0.3] = np.nan
    x[0] = np.nan                                                   # a row with nothing observed
    last, steps = -np.inf, 0
    for its in range(1, 40):
        r = RE.run(x, 1e-300, its, full=True)
        assert r["iters"] == its
        ll = RE.loglik(x, r["mu"], r["sigma"])
        assert ll >= last - 1e-9 * abs(ll), (its, ll, last)
        steps += ll > last
        last = ll
    assert steps >= 5


def test_resource_table_lists_the_new_kernels():
    """No scratch, no spills, LDS at most 80 KiB and what the header's arithmetic says (no build in this checkout: skipped,
    as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    assert hasattr(ctypes.CDLL(_qalib.LIB_PATH), "twxem_mean_variance")
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
        assert table[k]["lds"] <= 80 * 1024, (k, table[k])
    keys = 8 * _qalib.EM_MAX_ROWS
    assert keys + 3 * 32 * 8 <= table["k_em_prep"]["lds"] <= keys + 3 * 32 * 8 + 256
    it = 8192 + 4 * 8192 + 4 * 256 + 2 * 256
    assert it <= table["k_em_iter"]["lds"] <= it + 256
