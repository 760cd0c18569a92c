"""Generate tests/golden/golden_chkperf_v1.npz by EXECUTING the reference's judgement of a fit and its retry ladder on
scripted series.  Needs the reference checkout (``make_golden.REF``); the tests only read the fixture.

    python tests/golden/make_golden_chkperf.py

Executed (read at run time, nothing of the text is stored): twx/infill/infill_daily.py:44-51 (the constants), :563-595
(``_is_nonoptimal_infill``) and :436-524 (the ``chk_perf`` block of ``InfillMatrixPPCA.infill`` up to its return, placed
under a method header of ours; its Python-2 ``print`` statements are converted in memory by ``lib2to3``).
``scipy.stats.linregress`` is the real one.  Stubs: ``self.infill`` (the recursive refits) returns the scripted series of
the attempt its arguments name; ``r.hasVarChgPt`` is the numpy restatement (tests/restate_chkperf.py) -- R's
``changepoint`` cannot be run, so THE CHANGE-POINT DECISION IS THE ONLY PART OF THE FIXTURE THAT IS NOT EXECUTED REFERENCE.

Per scripted item and attempt the fixture records mae, r2 and the reasons the reference computed, the attempts it ran, and
the index and the series ``infill`` returned.  The maker refuses a fixture in which a decision margin (mae against 2.0, r2
against 0.7, a fitted value against 57.7 / -89.4, cpt_stat against pen) is below 1e-6 relative, or in which the float64
and the longdouble restatement decide differently.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_chkperf as RC  # noqa: E402

OUT = os.path.join(HERE, "golden_chkperf_v1.npz")
N = 120
MARGIN_MIN = 1e-6
REASON_BITS = {"low infill performance": RC.LOW_PERF, "impossible infill values": RC.IMPOSSIBLE,
               "variance change point": RC.VAR_CHGPT}

# (name, max_nnr_var, the kind of the series of the attempts 0 .. 3).  O: optimal; L<x>: the truth + noise of mean absolute
# size about x; R: r2 alone low; I: one value above 57.7 (i: below -89.4); C: a variance change point (see make_series);
# combinations by concatenation; =k: the series of attempt k again (an MAE tie).
SCRIPTS = [
    ("optimal at once", 0.99, ["O", "L3", "L3", "L3"]),
    ("optimal at once b", 0.99, ["O", "I", "C", "L3"]),
    ("fixed at rung 1 from L", 0.99, ["L3", "O", "L3", "L3"]),
    ("fixed at rung 1 from C", 0.99, ["C", "O", "L3", "L3"]),
    ("fixed at rung 1 from I", 0.99, ["I", "O", "L3", "L3"]),
    ("fixed at rung 1 from i", 0.99, ["i", "O", "L3", "L3"]),
    ("fixed at rung 2 from L", 0.99, ["L3", "L4", "O", "L3"]),
    ("fixed at rung 2 from CI", 0.99, ["C", "I", "O", "L3"]),
    ("fixed at rung 2 from LC", 0.99, ["L3C", "L3I", "O", "O"]),
    ("fixed at rung 3 from L", 0.99, ["L3", "L4", "L5", "O"]),
    ("fixed at rung 3 mixed", 0.99, ["I", "C", "L3C", "O"]),
    ("never, pure low everywhere", 0.99, ["L3", "L2.5", "L4", "L3.5"]),
    ("never, pure low last", 0.99, ["C", "L3", "I", "L2.5"]),
    ("never, one pure low", 0.99, ["L2.5I", "L4", "C", "I"]),
    ("never, pure low first", 0.99, ["L2.5", "L3", "L4", "L5"]),
    ("never, no pure low", 0.99, ["C", "I", "L3C", "L3I"]),
    ("never, no pure low b", 0.99, ["L3I", "L2.5C", "I", "C"]),
    ("never, no pure low c", 0.99, ["L4C", "L3C", "L2.5I", "L5I"]),
    ("tie, all equal", 0.99, ["L3", "=0", "=0", "=0"]),
    ("tie, least twice", 0.99, ["L4", "L2.5", "L3", "=1"]),
    ("tie, least twice late", 0.99, ["L4", "L3", "L2.5", "=2"]),
    ("tie, no pure low", 0.99, ["C", "=0", "I", "=0"]),
    ("tie, impure smaller", 0.99, ["L2.5I", "L3", "=1", "L4"]),
    ("no attempt 1, optimal", 0.90, ["O", "O", "L3", "L3"]),
    ("no attempt 1, fixed at 2", 0.90, ["L3", "O", "O", "L3"]),
    ("no attempt 1, fixed at 3", 0.90, ["C", "O", "I", "O"]),
    ("no attempt 1, never", 0.90, ["L3", "L2.1", "L4", "L2.5"]),
    ("no attempt 1, never mixed", 0.85, ["L3C", "L2.1", "I", "L2.5"]),
    ("no attempt 1, tie", 0.90, ["L3", "O", "=0", "=0"]),
    ("r2 alone low", 0.99, ["R", "O", "L3", "L3"]),
    ("r2 alone low, never", 0.99, ["R", "R", "L3", "R"]),
]


NBLOCK = 48                # a C item has no observation on its first NBLOCK days: the fit is free there


def expected_bits(kind):
    return (RC.LOW_PERF if kind[0] in "LR" else 0) | (RC.IMPOSSIBLE if "I" in kind or "i" in kind else 0) | \
        (RC.VAR_CHGPT if "C" in kind else 0)


def make_series(rs, kind, truth, flat, free):
    """One scripted series around the complete ``truth``.  C flattens the series on the first NBLOCK days, where the item has
    no observation: mae and r2 do not see it, the change-point check does.  An impossible value sits on one of the days
    ``free`` (without an observation, after the block) for the same reason."""
    k = kind
    if k[0] == "L":
        num, k = "", k[1:]
        while k and (k[0].isdigit() or k[0] == "."):
            num, k = num + k[0], k[1:]
        fit = truth + rs.randn(N) * float(num) * 1.2533              # E|z| = sqrt(2 / pi)
    elif k[0] == "R":                                                # errors as large as the nearly constant truth's spread
        fit = truth + rs.randn(N) * 0.3
    else:
        fit = truth + rs.randn(N) * (0.02 if flat else 0.3)
    if "C" in k:
        fit[:NBLOCK] = fit[NBLOCK:].mean() + (fit[:NBLOCK] - fit[:NBLOCK].mean()) * 0.01       # about the series' mean
    if "I" in k:
        fit[free[int(rs.randint(free.size))]] = 60.0 + rs.rand()
    if "i" in k:
        fit[free[int(rs.randint(free.size))]] = -95.0 - rs.rand()
    return fit


def build_items():
    rs = np.random.RandomState(1605)
    items = []
    for name, max_var, kinds in SCRIPTS:
        flat = any(k[0] == "R" for k in kinds)
        truth = 5.0 + rs.randn(N) * 0.2 if flat else 5.0 + 6.0 * np.sin(np.arange(N) / 7.0) + rs.randn(N) * 3.0
        obs = truth.copy()
        obs[rs.rand(N) < 0.15] = np.nan
        free = NBLOCK + np.nonzero(np.isnan(obs[NBLOCK:]))[0]
        if any("C" in k for k in kinds):
            obs[:NBLOCK] = np.nan
        series = []
        for k in kinds:
            series.append(series[int(k[1:])].copy() if k[0] == "=" else make_series(rs, k, truth, flat, free))
        want = [expected_bits(kinds[int(k[1:])] if k[0] == "=" else k) for k in kinds]
        items.append(dict(name=name, max_nnr_var=max_var, kinds=kinds, obs=obs, series=series, want=want))
    return items


def load_slice():
    """The namespace with the reference's ``_is_nonoptimal_infill`` and the ``chk_perf`` block as ``_Block.run``."""
    import make_golden as mg
    from lib2to3 import refactor
    from scipy import stats
    for name, val in (("bool", bool), ("int", int), ("float", float), ("object", object)):
        if name not in vars(np):
            setattr(np, name, val)
    warnings.filterwarnings("ignore", category=DeprecationWarning)

    class _R(object):
        @staticmethod
        def hasVarChgPt(vals):                                       # NOT executed reference: the numpy restatement
            v = np.asarray(vals, np.float64)
            c = RC.check(v, np.full(v.size, np.nan), RC.cpt_penalty(v.size))
            return [bool(c["reasons"] & RC.VAR_CHGPT)]

    class _Robjects(object):
        FloatVector = staticmethod(lambda a: np.asarray(a, np.float64))

    ns = dict(np=np, stats=stats, r=_R, robjects=_Robjects)
    exec(compile("\n" * 43 + mg._slice("twx/infill/infill_daily.py", 44, 51), "infill_daily.py", "exec"), ns)
    exec(compile("\n" * 562 + mg._slice("twx/infill/infill_daily.py", 563, 595), "infill_daily.py", "exec"), ns)
    head = ("class _Block(object):\n"
            "    def run(self, infill_tair, trim_pca_tair, min_daily_nnghs, nnghs_nnr, max_nnr_var, chk_perf, npcs,\n"
            "            frac_obs_initnpcs, ppca_varyexplain, ppcaConThres, verbose):\n")
    body = mg._slice("twx/infill/infill_daily.py", 436, 524)
    tool = refactor.RefactoringTool(["lib2to3.fixes.fix_print"])
    src = str(tool.refactor_string(head + body, "infill_daily.py"))
    assert "print(" in src and "print \"" not in src
    exec(compile(src, "infill_daily.py", "exec"), ns)
    return ns


def run_reference(ns, item, conv_thres=1e-5):
    """The reference's block on one scripted item: a dict of attempts, mae, r2, reasons (bit masks), kept, series."""
    import contextlib
    import io
    judge = ns["_is_nonoptimal_infill"]
    min_var = ns["MIN_NNR_VAR"]
    log = []

    class Matrix(ns["_Block"]):
        stn_id, tair_var, vname_mean = "SCRIPTED", "tmin", "norm01"
        pca_tair = item["obs"][:, None].copy()
        valid_pca_mask = np.isfinite(item["obs"])[:, None]

        def attempt_of(self, nnr_var, thres):
            if thres == conv_thres:
                return 0 if nnr_var == item["max_nnr_var"] else 1
            return 2 if thres == 1e-6 else 3

        def infill(self, min_daily_nnghs, nnghs_nnr, max_nnr_var, chk_perf, npcs, frac, vary, thres, verbose):
            assert chk_perf is False and thres in (conv_thres, 1e-6, 1e-7) and max_nnr_var in (item["max_nnr_var"], min_var)
            a = self.attempt_of(max_nnr_var, thres)
            assert a >= 1 and (a != 1 or max_nnr_var == min_var)
            log.append(a)
            return None, None, item["series"][a].copy()

    m = Matrix()
    orig = ns["_is_nonoptimal_infill"]
    judged = []

    def spy(infill_tair, matrix):
        res = orig(infill_tair, matrix)
        judged.append((res[1][:], float(res[2]), float(res[3])))
        return res

    ns["_is_nonoptimal_infill"] = spy
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fnl, mask, kept_series = m.run(item["series"][0].copy(), item["obs"][:, None].copy(), 3, 4, item["max_nnr_var"], True,
                                           0, 0.5, 0.99, conv_thres, False)
    finally:
        ns["_is_nonoptimal_infill"] = orig
    attempts = [0] + log
    assert len(judged) == len(attempts)
    assert np.array_equal(mask, np.isnan(item["obs"])) and np.array_equal(fnl[~mask], item["obs"][~mask])
    kept = [a for a in attempts if np.array_equal(item["series"][a], kept_series)][0]
    return dict(attempts=attempts, mae=[j[1] for j in judged], r2=[j[2] for j in judged],
                reasons=[sum(REASON_BITS[x] for x in j[0]) for j in judged], kept=kept, series=np.asarray(kept_series))


def main():
    ns = load_slice()
    items = build_items()
    pen = RC.cpt_penalty(N)
    rec = dict(mae=np.full((len(items), 4), np.nan), r2=np.full((len(items), 4), np.nan),
               reasons=np.full((len(items), 4), -1, np.int32), nattempts=np.zeros(len(items), np.int32),
               kept=np.zeros(len(items), np.int32), has_attempt1=np.zeros(len(items), bool),
               max_nnr_var=np.array([it["max_nnr_var"] for it in items]), names=np.array([it["name"] for it in items]),
               obs=np.array([it["obs"] for it in items]), series=np.array([it["series"] for it in items]),
               kept_series=np.zeros((len(items), N)), pen=np.float64(pen))
    worst = np.inf
    for i, it in enumerate(items):
        ref = run_reference(ns, it)
        rec["has_attempt1"][i] = ns["MIN_NNR_VAR"] < it["max_nnr_var"]
        rec["nattempts"][i], rec["kept"][i], rec["kept_series"][i] = len(ref["attempts"]), ref["kept"], ref["series"]
        for a, mae, r2, reasons in zip(ref["attempts"], ref["mae"], ref["r2"], ref["reasons"]):
            rec["mae"][i, a], rec["r2"][i, a], rec["reasons"][i, a] = mae, r2, reasons
            c = RC.check_pair(it["series"][a], it["obs"], pen)
            if not np.isfinite(max(c["d_mae"], c["d_r2"], c["d_cpt"])):
                raise SystemExit("refused: float64 and longdouble decide differently on %r attempt %d" % (it["name"], a))
            if reasons != it["want"][a]:
                raise SystemExit("refused: %r attempt %d was scripted as %d and judged %d (mae %.3g, r2 %.3g)" % (
                    it["name"], a, it["want"][a], reasons, mae, r2))
            if c["reasons"] != reasons:
                raise SystemExit("refused: the restatement disagrees with the reference on %r attempt %d" % (it["name"], a))
            m = min(c["margins"].values())
            if m < MARGIN_MIN:
                raise SystemExit("refused: %r attempt %d has a margin of %.3g" % (it["name"], a, m))
            worst = min(worst, m)
        print("%-28s attempts %s reasons %s kept %d" % (it["name"], ref["attempts"], ref["reasons"], ref["kept"]))
    rec["min_margin"] = np.float64(worst)
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d items, %d bytes), smallest margin %.3g, pen(%d) = %.6g" % (OUT, len(items), os.path.getsize(OUT), worst, N, pen))


if __name__ == "__main__":
    main()
