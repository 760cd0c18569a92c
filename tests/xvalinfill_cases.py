"""Shared by tests/test_xvalinfill_host.py and tests/test_gpu_xvalinfill.py: the literal lines of the reference's hold-out
(twx/infill/xval_infill.py:73-86) in numpy, the rows and series of the shape grids, the float64 restatement of the score
with its longdouble twin, and the parent's chain run one station at a time on a masked pool copy (no GPU call is made
when this file is imported)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOLD_NDAYS = (1, 63, 64, 65, 128, 129, 1000)
HOLD_SEED = 15
FACADE_XVAL = (1, 2, 5, 12)        # 1 and 2 are each other's neighbours; 5 is the noisy station; 12 lies in the other group
FACADE_NTRAIN_YRS = 2


def nmask_of(ntrain_yrs):
    return int(np.round(ntrain_yrs * 365.25))                      # :73


def literal_holdout(row, nmask):
    """Lines 78-86 for one station's observations, as they are written."""
    idxs = np.arange(row.size)
    fin_obs = np.isfinite(row)
    last_idxs = np.nonzero(fin_obs)[0][-nmask:]
    return np.logical_and(np.logical_not(np.isin(idxs, last_idxs, assume_unique=True)), fin_obs)


def closed_form(row, nkeep):
    """What include/twx_qa.h states: finite, and (nkeep > 0) at least nkeep finite days after it."""
    fin = np.isfinite(row)
    after = fin[::-1].cumsum()[::-1] - fin
    return fin & (nkeep > 0) & (after >= nkeep)


def holdout_rows(ndays, seed=HOLD_SEED):
    """[nrows, ndays] float32: all NaN, all finite, finite only in the last chunk of 64, finite only in the first chunk,
    one holding +-inf among finite values, and two random rows (one sparse)."""
    rs = np.random.RandomState(seed + ndays)
    base = np.round(rs.randn(7, ndays) * 5, 1).astype(np.float32)
    rows = base.copy()
    rows[0] = np.nan
    last0 = ((ndays - 1) // 64) * 64
    rows[2, :last0] = np.nan
    rows[3, 64:] = np.nan
    rows[4, ::3] = np.inf
    rows[4, 1::5] = -np.inf
    rows[5, rs.rand(ndays) < 0.3] = np.nan
    rows[6, rs.rand(ndays) < 0.9] = np.nan
    return rows


def holdout_nkeeps(rows):
    out = {0, 1, 64}
    for r in rows:
        nf = int(np.isfinite(r).sum())
        out.update(k for k in (nf - 1, nf, nf + 1) if k >= 0)
    return sorted(out)


def want_holdout(rows, nkeep):
    held = np.array([literal_holdout(r, nkeep) for r in rows])
    train = np.where(held, np.float32(np.nan), rows)
    return held, train, held.sum(axis=1).astype(np.int32), np.isfinite(rows).sum(axis=1).astype(np.int32)


# ---- the score ----
def score_series(n, seed=4):
    """(infill [4, n] float64, obs [4, n] float32, held [4, n] bool, group [n] int8): an ordinary series; one with no held
    day; one with an unfitted month (NaN in infill over group 3); one with held days in group 7 only."""
    rs = np.random.RandomState(seed + n)
    group = (np.arange(n) // 3 % 13 - 1).astype(np.int8)            # -1, 0 .. 11 in runs of three days
    obs = np.round(2.0 + 4.0 * rs.randn(4, n), 2).astype(np.float32)
    infill = obs.astype(np.float64) + 0.3 + 0.5 * rs.randn(4, n)
    held = rs.rand(4, n) < 0.6
    obs[~held & (rs.rand(4, n) < 0.5)] = np.nan                     # what is not held may be missing
    held[1] = False
    infill[2, group == 3] = np.nan
    held[3] &= group == 7
    return infill, obs, held, group


def want_score(infill, obs, held, group, dtype=np.float64):
    """n, bias, mae [ns, 13] (entry 12: the whole series) as numpy means in ``dtype``, and the two float32 rows."""
    ns, nd = infill.shape
    n = np.zeros((ns, 13), np.int32)
    bias, mae = np.full((ns, 13), np.nan, dtype), np.full((ns, 13), np.nan, dtype)
    scored = held & np.isfinite(infill)
    for s in range(ns):
        for p in range(13):
            m = scored[s] if p == 12 else scored[s] & (group == p)
            n[s, p] = m.sum()
            if n[s, p]:
                d = infill[s, m].astype(dtype) - obs[s, m].astype(dtype)
                bias[s, p], mae[s, p] = np.mean(d), np.mean(np.abs(d))
    oo = np.where(scored, obs, np.float32(np.nan)).astype(np.float32)
    io = np.where(scored, infill, np.nan).astype(np.float32)
    return n, bias, mae, oo, io


# ---- the chain of the parent code, one station at a time on a masked pool copy ----
def masked_copy(pool, var, col, held_row):
    """A copy of ``pool`` in which the held observations of column ``col`` are NaN."""
    from topowx_amd.qa import StationObsPool
    a = {v: getattr(pool, v).copy() for v in ("tmin", "tmax")}
    a[var][held_row, col] = np.nan
    return StationObsPool(pool.ids, pool.lon, pool.lat, a["tmin"], a["tmax"], pool.days)


def held_masks(pool, var, cols, nkeep):
    obs = getattr(pool, var)
    return np.array([literal_holdout(obs[:, c], nkeep) for c in cols])


def ranked_equal(a, ta, b, tb):
    """Status, nnghs, max_dist and every CSR column of target ta of ``a`` and target tb of ``b`` (two ``InfillMatrices``
    over the same day groups), byte for byte."""
    for k in ("status", "nnghs", "max_dist"):
        if getattr(a, k)[ta].tobytes() != getattr(b, k)[tb].tobytes():
            return False, k
    for g in range(a.ngroups):
        ra, rb = a.ranked(ta, g), b.ranked(tb, g)
        for k in ra:
            if ra[k].tobytes() != rb[k].tobytes():
                return False, (k, g)
    return True, None


# ---- the golden of make_golden_xvalinfill.py ----
def load_gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_xvalinfill_v1.npz"))


def gold_case(gold):
    """(ids, lon, lat, tmin, days) of the golden, checked against its input hash."""
    import make_golden_infillmat as mk
    import make_golden_xvalinfill as mx
    case = mx.case_inputs()
    assert mk.input_hash(*case) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return case


def gold_held(gold):
    return np.unpackbits(gold["held"], axis=1)[:, :int(gold["ndays"])].astype(bool)


def gold_lists(gold, stage, t):
    """(off [13], idx, ioa, dist, nnghs [12], max_dist [12]) of cross-validation station t in stage 1 or 2."""
    return tuple(gold["s%d_%s_%d" % (stage, k, t)] for k in ("off", "idx", "ioa", "dist", "nnghs", "max_dist"))
