"""The check of step16's fits and the retry ladder in numpy, the same text as include/twx_qa.h (``twxck_infill_check``) and
``topowx_amd.infill.RetryLadder``: what the GPU kernel and the host state machine are compared with.  Every sum is
sequential in row order (``np.cumsum`` / a Python loop are avoided only where a sequential ``np.add.accumulate`` says the
same); ``dtype=np.longdouble`` runs the same text in extended precision, and the distance between the two is the yardstick
of the tolerances.  The penalty is the binding's ``cpt_penalty``: one function for both sides.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from topowx_amd._qalib import cpt_penalty  # noqa: E402,F401

OK, NOT_FITTED, FEW_ROWS, ROW_CAP = 0, 26, 27, 28
LOW_PERF, IMPOSSIBLE, VAR_CHGPT, UNFITTED = 1, 2, 4, 8
MAX_ROWS = 8192
MAE_MAX, R2_MIN, IMPOSSIBLE_HIGH, IMPOSSIBLE_LOW = 2.0, 0.7, 57.7, -89.4
VAR_FLOOR = 1e-10
MIN_NNR_VAR, RETRY_THRESHOLDS = 0.90, (1e-6, 1e-7)


def seq_sum(v, dtype):
    """The sum of v in order, in ``dtype``."""
    v = np.asarray(v, dtype)
    return np.add.accumulate(v, dtype=dtype)[-1] if v.size else dtype(0)


def check(fit, obs, pen, dtype=np.float64, mae_max=MAE_MAX, r2_min=R2_MIN, impossible_high=IMPOSSIBLE_HIGH,
          impossible_low=IMPOSSIBLE_LOW):
    """The check of one item: a dict of nobs, mae, r2, nimpossible, cpt_stat, cpt_tau, reasons, status (the outputs of
    ``twxck_infill_check``, mae / r2 / cpt_stat in ``dtype``), and for the tests ``tmp_gap`` (the runner-up tmp over the
    minimum among the other taus; inf if there is none) and ``margins`` (the relative distance of every decision from its
    bound)."""
    fit64, obs64 = np.asarray(fit, np.float64), np.asarray(obs, np.float64)
    n = fit64.size
    nan = dtype(np.nan)
    out = dict(nobs=0, mae=nan, r2=nan, nimpossible=0, cpt_stat=nan, cpt_tau=0, reasons=UNFITTED, status=ROW_CAP,
               tmp_gap=np.inf, margins={})
    if n > MAX_ROWS:
        return out
    if not np.isfinite(fit64).all():
        out["status"] = NOT_FITTED
        return out
    f, o = fit64.astype(dtype), obs64.astype(dtype)
    v = np.isfinite(obs64)
    nobs = int(v.sum())
    margins = {}
    with np.errstate(all="ignore"):
        mae, r2 = nan, nan
        if nobs:
            fv, ov = f[v], o[v]
            mae = seq_sum(np.abs(fv - ov), dtype) / dtype(nobs)
            xbar, ybar = seq_sum(ov, dtype) / dtype(nobs), seq_sum(fv, dtype) / dtype(nobs)
            dx, dy = ov - xbar, fv - ybar
            ssxm, ssym, ssxym = seq_sum(dx * dx, dtype), seq_sum(dy * dy, dtype), seq_sum(dx * dy, dtype)
            if ssxm == 0 or ssym == 0:
                r = dtype(0)
            else:
                r = min(max(ssxym / np.sqrt(ssxm * ssym), dtype(-1)), dtype(1))
            r2 = r * r
            margins["mae"] = abs(float(mae) - mae_max) / mae_max
            margins["r2"] = abs(float(r2) - r2_min) / r2_min
        nimp = int((fit64 > impossible_high).sum() + (fit64 < impossible_low).sum())
        if n:
            margins["impossible"] = float(min(np.abs(fit64 - impossible_high).min() / abs(impossible_high),
                                              np.abs(fit64 - impossible_low).min() / abs(impossible_low)))
        reasons = 0
        if mae > mae_max or r2 < r2_min:
            reasons |= LOW_PERF
        if nimp:
            reasons |= IMPOSSIBLE
        out.update(nobs=nobs, mae=mae, r2=r2, nimpossible=nimp, status=OK if n >= 4 else FEW_ROWS)
        if n >= 4:
            mu = seq_sum(f, dtype) / dtype(n)
            d = f - mu
            y2 = np.add.accumulate(d * d, dtype=dtype)
            null = dtype(n) * np.log(y2[-1] / dtype(n))
            tau = np.arange(2, n - 1)
            s1 = y2[tau - 1] / tau.astype(dtype)
            sn = (y2[-1] - y2[tau - 1]) / (n - tau).astype(dtype)
            s1 = np.where(s1 <= 0, dtype(VAR_FLOOR), s1)
            sn = np.where(sn <= 0, dtype(VAR_FLOOR), sn)
            tmp = tau.astype(dtype) * np.log(s1) + (n - tau).astype(dtype) * np.log(sn)
            ok = ~np.isnan(tmp)
            if ok.any():
                k = int(np.argmin(np.where(ok, tmp, dtype(np.inf))))      # the first of the smallest
                out["cpt_tau"], out["cpt_stat"] = int(tau[k]), null - tmp[k]
                rest = np.delete(tmp, k)[np.delete(ok, k)]
                if rest.size:
                    out["tmp_gap"] = float(rest.min() - tmp[k])
                if pen == pen:
                    margins["cpt"] = abs(float(out["cpt_stat"]) - pen) / abs(pen) if np.isfinite(out["cpt_stat"]) else np.inf
                    if out["cpt_stat"] >= pen:
                        reasons |= VAR_CHGPT
        out["reasons"], out["margins"] = reasons, margins
    return out


def check_pair(fit, obs, pen, **kw):
    """The float64 check with ``d_mae``, ``d_r2``, ``d_cpt``: its distances from the longdouble one (inf where the two decide
    differently: reasons, status or cpt_tau)."""
    a, b = check(fit, obs, pen, np.float64, **kw), check(fit, obs, pen, np.longdouble, **kw)
    same = (a["reasons"], a["status"], a["cpt_tau"], a["nobs"]) == (b["reasons"], b["status"], b["cpt_tau"], b["nobs"])
    for k, name in (("mae", "d_mae"), ("r2", "d_r2"), ("cpt_stat", "d_cpt")):
        x, y = float(a[k]), float(b[k])
        if not same:
            a[name] = np.inf
        elif np.isnan(x) and np.isnan(y) or x == y:
            a[name] = 0.0
        else:
            with np.errstate(all="ignore"):
                a[name] = float(abs(np.longdouble(a[k]) - b[k]))
    return a


def ladder(judge, has_attempt1=True):
    """The chk_perf block of ``InfillMatrixPPCA.infill`` (:438-518) with our two stated rules.  ``judge(attempt)`` returns
    (reasons, mae, fitted) of that attempt (a repeated attempt's result is the earlier one's: the caller's business).
    Returns a dict of kept, attempts, reasons, mae, nonoptimal, retry_fixed."""
    attempts, reasons, maes, fitted = [], [], [], []

    def run(a):
        r, m, f = judge(a)
        attempts.append(a); reasons.append(int(r)); maes.append(float(m)); fitted.append(bool(f))
        return not (f and r == 0)

    non_optimal = run(0)
    if non_optimal:
        if has_attempt1:
            non_optimal = run(1)
        if non_optimal:
            for a in (2, 3):
                non_optimal = run(a)
                if not non_optimal:
                    break
    if not non_optimal:
        return dict(kept=attempts[-1], attempts=attempts, reasons=reasons, mae=maes, nonoptimal=False,
                    retry_fixed=attempts[-1] > 0)
    idx = [k for k in range(len(attempts)) if fitted[k]] or list(range(len(attempts)))
    pure = [k for k in idx if reasons[k] == LOW_PERF]
    idx = pure or idx
    k = idx[int(np.argmin(np.array([maes[j] for j in idx])))]
    return dict(kept=attempts[k], attempts=attempts, reasons=reasons, mae=maes, nonoptimal=True, retry_fixed=False)
