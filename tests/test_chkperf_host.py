"""CPU: the host side of step16's ``chk_perf`` -- ``RetryLadder`` and the numpy restatement of the check
(tests/restate_chkperf.py) against the executed-reference golden (tests/golden/make_golden_chkperf.py), the penalty, the
header / binding / build naming, the resource table of a build and the call-level failures of ``twxck_infill_check`` (they
need the library, not a GPU).  The kernel is checked against the restatement in tests/test_gpu_chkperf.py.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chkperf_cases as CC  # noqa: E402
import restate_chkperf as RC  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return CC.load_gold()


def attempts_of(gold, i):
    return [a for a in range(4) if gold["reasons"][i, a] >= 0]


def test_golden_file(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_chkperf_v1.npz")) < 1024 * 1024
    assert gold["min_margin"] >= 1e-6 and gold["names"].size >= 24
    n = [len(attempts_of(gold, i)) for i in range(gold["names"].size)]
    assert np.array_equal(n, gold["nattempts"]) and set(n) == {1, 2, 3, 4}
    assert (~gold["has_attempt1"]).sum() >= 4 and (gold["reasons"][~gold["has_attempt1"], 1] == -1).all()
    assert {1, 2, 3, 4, 5}.issubset(set(gold["reasons"].ravel().tolist()))
    fixed = [i for i in range(len(n)) if gold["reasons"][i, gold["kept"][i]] == 0 and gold["kept"][i] > 0]
    assert {int(gold["kept"][i]) for i in fixed} == {1, 2, 3}          # fixed at each rung
    print("golden: %d items, smallest margin %.3g" % (len(n), gold["min_margin"]))


def test_ladder_class_reproduces_the_golden(gold):
    """``RetryLadder`` fed the golden's reasons and MAE: the attempts it asks for, the kept attempt and the flags, exact; the
    functional restatement says the same."""
    from topowx_amd.infill import RetryLadder
    for i, name in enumerate(gold["names"]):
        inputs = [("a", 1e-5), ("b", 1e-5) if gold["has_attempt1"][i] else None, ("a", 1e-6), ("a", 1e-7)]
        lad, asked = RetryLadder(inputs), []
        while lad.request is not None:
            a = lad.request
            assert lad.duplicate is None
            asked.append(a)
            lad.feed(gold["reasons"][i, a], gold["mae"][i, a])
        assert asked == attempts_of(gold, i) == lad.attempts, name
        assert lad.kept == gold["kept"][i], (name, lad.kept, gold["kept"][i])
        assert lad.nonoptimal == (gold["reasons"][i, lad.kept] != 0) and lad.retry_fixed == (not lad.nonoptimal and lad.kept > 0), name
        rec = RC.ladder(lambda a: (gold["reasons"][i, a], gold["mae"][i, a], True), bool(gold["has_attempt1"][i]))
        assert (rec["kept"], rec["attempts"], rec["nonoptimal"], rec["retry_fixed"]) == (lad.kept, asked, lad.nonoptimal, lad.retry_fixed), name
        assert np.array_equal(gold["series"][i, lad.kept], gold["kept_series"][i]), name
        with pytest.raises(ValueError):
            lad.feed(0, 0.0)


def test_ladder_rules_of_ours():
    from topowx_amd.infill import RetryLadder
    # equal inputs: attempt 1 repeats attempt 0 (no reanalysis columns), attempt 2 repeats it when the call's threshold is 1e-6
    lad = RetryLadder([(0, 1e-6), (0, 1e-6), (0, 1e-6), (0, 1e-7)])
    lad.feed(1, 3.0)
    assert lad.request == 1 and lad.duplicate == 0
    lad.feed(1, 3.0)
    assert lad.request == 2 and lad.duplicate == 0
    lad.feed(1, 3.0)
    assert lad.request == 3 and lad.duplicate is None
    lad.feed(1, 3.0)
    assert lad.request is None and lad.kept == 0 and lad.attempts == [0, 1, 2, 3] and lad.nonoptimal and not lad.retry_fixed
    # an attempt that is not fitted is never kept while a fitted one exists, whatever its MAE
    lad = RetryLadder([(3, 1e-5), (2, 1e-5), (3, 1e-6), (3, 1e-7)])
    for reasons, mae, fitted in ((8, np.nan, False), (5, 4.0, True), (8, np.nan, False), (2, 0.5, True)):
        lad.feed(reasons, mae, fitted)
    assert lad.kept == 3 and lad.nonoptimal
    lad = RetryLadder([(3, 1e-5), None, (3, 1e-6), (3, 1e-7)])
    for _ in range(3):
        lad.feed(8, np.nan, False)
    assert lad.attempts == [0, 2, 3] and lad.kept == 0 and lad.nonoptimal      # nothing fitted: the first
    lad = RetryLadder([(3, 1e-5), (2, 1e-5), (3, 1e-6), (3, 1e-7)])
    lad.feed(8, np.nan, False)
    lad.feed(0, 0.3)
    assert lad.request is None and lad.kept == 1 and lad.retry_fixed and not lad.nonoptimal
    with pytest.raises(ValueError):
        RetryLadder([(0, 1e-5), (0, 1e-5), None, (0, 1e-7)])


def test_restated_check_against_the_golden(gold):
    """mae and r2 of the restatement against the values scipy and numpy gave the executed reference (1e-12), the reasons
    exact, on every attempt that ran."""
    pen, seen = float(gold["pen"]), 0
    assert pen == RC.cpt_penalty(gold["obs"].shape[1])
    for i, name in enumerate(gold["names"]):
        for a in attempts_of(gold, i):
            c = RC.check(gold["series"][i, a], gold["obs"][i], pen)
            assert abs(c["mae"] - gold["mae"][i, a]) <= 1e-12 and abs(c["r2"] - gold["r2"][i, a]) <= 1e-12, (name, a)
            assert c["reasons"] == gold["reasons"][i, a] and c["status"] == RC.OK, (name, a)
            seen += 1
    assert seen == gold["nattempts"].sum()


def test_restated_check_known_answers():
    s = dict((name, (fit, obs)) for name, fit, obs in CC.degenerate_series())
    c = RC.check(*s["constant"], pen=10.0)
    assert c["cpt_stat"] == -np.inf and c["cpt_tau"] == 2 and c["reasons"] == RC.LOW_PERF and c["mae"] == 0.5 and c["r2"] == 0.0
    c = RC.check(*s["mirrored"], pen=10.0)
    assert c["cpt_tau"] == 16 and c["tmp_gap"] == 0.0 and c["reasons"] == RC.VAR_CHGPT      # the lower of two equal minima
    c = RC.check(*s["nobs 0"], pen=10.0)
    assert c["nobs"] == 0 and np.isnan(c["mae"]) and np.isnan(c["r2"]) and c["reasons"] == 0 and c["status"] == RC.OK
    c = RC.check(*s["nobs 1"], pen=10.0)
    assert c["nobs"] == 1 and c["mae"] == 0.25 and c["r2"] == 0.0 and c["reasons"] == RC.LOW_PERF
    for name in ("NaN in fit", "inf in fit"):
        c = RC.check(*s[name], pen=10.0)
        assert c["status"] == RC.NOT_FITTED and c["reasons"] == RC.UNFITTED and np.isnan(c["cpt_stat"]) and c["nobs"] == 0
    c = RC.check(*s["N 3"], pen=10.0)
    assert c["status"] == RC.FEW_ROWS and c["nobs"] == 3 and np.isnan(c["cpt_stat"]) and c["cpt_tau"] == 0 and abs(c["mae"] - 0.1) < 1e-15
    assert RC.check(*s["N 8193"], pen=10.0)["status"] == RC.ROW_CAP
    c = RC.check(*s["constant obs"], pen=10.0)
    assert c["r2"] == 0.0 and c["reasons"] & RC.LOW_PERF
    # a NaN penalty means "no change point"; cpt_stat and cpt_tau are still reported
    fit = np.concatenate([np.tile([0.01, -0.01], 15), np.tile([9.0, -9.0], 15)])
    a, b = RC.check(fit, fit, np.nan), RC.check(fit, fit, 10.0)
    assert a["reasons"] == 0 and b["reasons"] == RC.VAR_CHGPT and a["cpt_tau"] == b["cpt_tau"] == 30 and a["cpt_stat"] == b["cpt_stat"] > 10
    assert RC.check(fit, fit, float(b["cpt_stat"]))["reasons"] == RC.VAR_CHGPT      # >= in the decision
    # impossible values count on every row, observed or not
    fit = np.array([1.0, 58.0, -90.0, 2.0, 57.7, -89.4, 3.0, 0.0])
    assert RC.check(fit, np.full(8, np.nan), np.nan)["nimpossible"] == 2


def test_cpt_penalty():
    from topowx_amd import _qalib
    assert RC.cpt_penalty is _qalib.cpt_penalty                       # one function for the restatement and the facade
    assert all(np.isnan(_qalib.cpt_penalty(n)) for n in range(1, 63)) and np.isfinite(_qalib.cpt_penalty(63))
    for n, want in ((63, 293.8), (186, 215.6), (2139, 186.7)):
        assert abs(_qalib.cpt_penalty(n) - want) < 0.05, (n, _qalib.cpt_penalty(n))
    # the formula, spelled out once more with numpy (1e-9 relative)
    for n in (63, 186, 2139, 8192):
        ll = np.log(np.log(n))
        a, b = np.sqrt(2 * ll), 2 * ll + np.log(ll) / 2 - np.log(np.sqrt(np.pi))
        want = (-(np.log(np.log((1 - 1e-10 + np.exp(-2 * np.exp(b))) ** -0.5)) / a) + b / a) ** 2
        assert abs(_qalib.cpt_penalty(n) / want - 1) < 1e-9
    assert _qalib.cpt_penalty(186, 0.05) < _qalib.cpt_penalty(186, 1e-10)


def test_header_binding_and_build_naming():
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxck_\w+)\s*\(", h))) == sorted(_qalib.CK_EXPORTS) == ["twxck_infill_check"]
    for name, val in (("TWXCK_MAX_ROWS", _qalib.CK_MAX_ROWS), ("TWXCK_NOT_FITTED", _qalib.CK_NOT_FITTED),
                      ("TWXCK_FEW_ROWS", _qalib.CK_FEW_ROWS), ("TWXCK_ROW_CAP", _qalib.CK_ROW_CAP),
                      ("TWXCK_LOW_PERF", _qalib.CK_LOW_PERF), ("TWXCK_IMPOSSIBLE", _qalib.CK_IMPOSSIBLE),
                      ("TWXCK_VAR_CHGPT", _qalib.CK_VAR_CHGPT), ("TWXCK_UNFITTED", _qalib.CK_UNFITTED),
                      ("TWXCK_NTIMES", len(_qalib.CK_KERNELS) + len(_qalib.CK_HOST_TIMES))):
        assert re.search(r"#define %s %d\b" % (name, val), h), name
    assert _qalib.CK_MAX_ROWS == _qalib.PP_MAX_ROWS
    assert (RC.OK, RC.NOT_FITTED, RC.FEW_ROWS, RC.ROW_CAP) == (_qalib.CK_OK, _qalib.CK_NOT_FITTED, _qalib.CK_FEW_ROWS, _qalib.CK_ROW_CAP)
    assert (RC.LOW_PERF, RC.IMPOSSIBLE, RC.VAR_CHGPT, RC.UNFITTED) == (_qalib.CK_LOW_PERF, _qalib.CK_IMPOSSIBLE, _qalib.CK_VAR_CHGPT, _qalib.CK_UNFITTED)
    statuses = [int(v) for v in re.findall(r"#define TWX(?:EM|PP|CK)_[A-Z_]+ (\d+) +/\*", h)]
    assert len({_qalib.CK_NOT_FITTED, _qalib.CK_FEW_ROWS, _qalib.CK_ROW_CAP} & {20, 21, 22, 23, 24, 25}) == 0 and statuses
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "topowx_amd/qa/twx_infillchk.hip" in build and os.path.exists(os.path.join(ROOT, "topowx_amd", "qa", "twx_infillchk.hip"))
    from topowx_amd.infill import infill_daily as facade
    import inspect
    sig = inspect.signature(facade)
    assert sig.parameters["chk_perf"].default is False and sig.parameters["cpt_sig"].default == 1e-10


def test_resource_table_lists_the_new_kernel():
    """No scratch, no spill, and the 32 doubles of LDS the reductions use (no build in this checkout: skipped, as
    test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_resources
    assert hasattr(ctypes.CDLL(_qalib.LIB_PATH), "twxck_infill_check")
    table = isa_resources.parse(res)
    assert "k_ck_check" in table
    k = table["k_ck_check"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 4 * 8 * 8, k


def test_call_level_failures():
    """``off`` not non-decreasing from 0 and a non-finite scalar fail the call before the device is touched."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    fit = np.arange(8.0)
    for off, text in (([1, 4, 8], "off[0]"), ([0, 5, 4], "decreases"), ([0, 4, 2, 8], "decreases")):
        with pytest.raises(_qalib.QaError) as e:
            _qalib.infill_check(off, fit, fit, pen=10.0)
        assert text in str(e.value), str(e.value)
    for kw in (dict(mae_max=np.nan), dict(r2_min=np.inf), dict(impossible_high=np.nan), dict(impossible_low=-np.inf)):
        with pytest.raises(_qalib.QaError) as e:
            _qalib.infill_check([0, 8], fit, fit, pen=10.0, **kw)
        assert "finite" in str(e.value)
    with pytest.raises(ValueError):
        _qalib.infill_check([0, 7], fit, fit)
    with pytest.raises(ValueError):
        _qalib.infill_check([0], fit[:0], fit[:0])
