"""The numpy restatement of step16's estimator (EM for probabilistic PCA with missing values: Tipping and Bishop 1999,
Verbeek's ``ppca_mv`` which ``pcaMethods::ppca`` follows) as include/twx_qa.h, ``twxpp_ppca_fit``, states it, and of the
component search of ``run_ppca`` (twx/infill/rpy/pca_infill.R:112-303): the checker of the GPU kernels.  ``dtype`` is
``np.float64`` or ``np.longdouble``.

    Y [N, D] standardised, non-finite = missing; d components; C0 [D, d]
    set-up   M_j = mean of column j over its observed values; Ye = Y - M, hidden positions 0; C = C0; CtC = C'C;
             X = (Ye C) CtC^-1; ss = sum over observed positions of (X C' - Ye)^2 / (N D - missing); count = 1; old = inf
    iterate  Sx = (I + CtC / ss)^-1; ss_old = ss; Ye[hidden] = (X C')[hidden]; X = ((Ye C) Sx) / ss; S = X'X;
             C = (Ye'X) (S + N Sx)^-1; CtC = C'C;
             ss = (sum (C X' - Ye')^2 + N sum(CtC o Sx) + missing ss_old) / (N D);
             objective = N (D log ss + tr Sx - log det Sx) + tr S - missing log ss_old;
             rel = |1 - objective / old|; old = objective; count += 1;
             stop at rel < threshold and count > 5 (OK), else at count > maxits (MAXITS)
    after    Q = the columns of C orthonormalised in order (modified Gram-Schmidt, every column twice); T = Ye Q;
             cov = (T'T - s s' / N) / (N - 1), s the column sums of T; eigenvectors V of cov, eigenvalues descending;
             C = Q V; X = Ye C (Ye with its last fill)
    out      R2cum[i] = 1 - sum_obs (Ye - X[:, :i] C[:, :i]')^2 / sum_obs Ye^2; fit = X C[0]' + M_0

An inverse is Gauss-Jordan without pivoting (the matrices are symmetric positive definite): a pivot <= 0 or not finite,
ss <= 0 or not finite, or a column of C without norm in the orthonormalisation: NUMERIC, NaN results.  log det Sx is minus the
sum of the logs of the pivots of I + CtC / ss.  ``iters`` = count - 1.
"""
import numpy as np

OK, NUMERIC, MAXITS, NO_MATRIX, EMPTY_COLUMN, ROW_CAP, COL_CAP, PCS_CAP = 0, 4, 20, 21, 22, 23, 24, 25
MAX_COLS, MAX_PCS, MAX_ROWS = 64, 32, 8192
SEED = 4324


def default_c0(D, d, seed=SEED):
    """The facade's start: ``RandomState(seed).standard_normal(D * d)`` laid out column-major as [D, d]."""
    return np.random.RandomState(seed).standard_normal(D * d).reshape(d, D).T.copy()


def gj_inverse(a):
    """(inverse, sum of the logs of the pivots, bad): in-place Gauss-Jordan without pivoting, the pivot row divided by the
    pivot."""
    w = np.array(a)
    n = w.shape[0]
    one = w.dtype.type(1)
    logdet = w.dtype.type(0)
    for p in range(n):
        piv = w[p, p]
        if not (np.isfinite(piv) and piv > 0):
            return w, logdet, True
        logdet = logdet + np.log(piv)
        row = w[p] / piv
        row[p] = one / piv
        f = w[:, p].copy()
        f[p] = 0
        w = w - f[:, None] * row[None, :]
        w[:, p] = -f / piv
        w[p] = row
    return w, logdet, False


def orthonormalise(c):
    """Modified Gram-Schmidt on the columns in order, every column against the earlier ones twice; (Q, bad)."""
    q = np.array(c)
    for k in range(q.shape[1]):
        for _ in range(2):
            for m in range(k):
                q[:, k] = q[:, k] - (q[:, m] * q[:, k]).sum() * q[:, m]
        nrm = np.sqrt((q[:, k] * q[:, k]).sum())
        if not (np.isfinite(nrm) and nrm > 0):
            return q, True
        q[:, k] = q[:, k] / nrm
    return q, False


def fit(y, d, c0=None, threshold=1e-5, maxits=1000, dtype=np.float64, trace=False):
    """One PPCA fit.  Returns a dict: status, iters, rel (the last), rels and objectives (every iteration's), r2cum [d],
    fit [N] (standardised scale: X C[0]' + M_0), C [D, d], M [D], ss."""
    y = np.asarray(y, dtype)
    N, D = y.shape
    if d < 1 or d > D or N <= d:
        raise ValueError("need 1 <= d <= D and N > d")
    if not threshold > 0 or maxits < 1:
        raise ValueError("threshold and maxits must be positive")
    c0 = default_c0(D, d) if c0 is None else c0
    nan = float("nan")
    out = dict(status=OK, iters=0, rel=nan, rels=[], objectives=[], r2cum=np.full(d, nan), fit=np.full(N, nan),
               C=np.full((D, d), nan), M=np.full(D, nan), ss=nan)
    obs = np.isfinite(y)
    cnt = obs.sum(axis=0)
    if (cnt == 0).any():
        out["status"] = EMPTY_COLUMN
        return out
    hidden = ~obs
    missing = dtype(int(hidden.sum()))
    n_, d_ = dtype(N), dtype(D)
    with np.errstate(all="ignore"):
        M = np.where(obs, y, dtype(0)).sum(axis=0) / cnt.astype(dtype)
        ye = np.where(obs, y - M, dtype(0))
        C = np.asarray(c0, dtype).copy()
        ctc = C.T @ C
        inv, _, bad = gj_inverse(ctc)
        if bad:
            out["status"] = NUMERIC
            return out
        X = (ye @ C) @ inv
        r = X @ C.T - ye
        ss = (np.where(obs, r, dtype(0)) ** 2).sum() / (n_ * d_ - missing)
        count, old = 1, dtype(np.inf)
        status = None
        eye = np.eye(d, dtype=dtype)
        while status is None:
            if not (np.isfinite(ss) and ss > 0):
                status = NUMERIC
                break
            sx, logpiv, bad = gj_inverse(eye + ctc / ss)
            if bad:
                status = NUMERIC
                break
            ss_old = ss
            ye_prev_fill = (X, C)
            ye = np.where(hidden, X @ C.T, ye)
            X = ((ye @ C) @ sx) / ss
            S = X.T @ X
            inv, _, bad = gj_inverse(S + n_ * sx)
            if bad:
                status = NUMERIC
                break
            C = (ye.T @ X) @ inv
            ctc = C.T @ C
            r = X @ C.T - ye
            ss = ((r * r).sum() + n_ * (ctc * sx).sum() + missing * ss_old) / (n_ * d_)
            if not (np.isfinite(ss) and ss > 0):
                status = NUMERIC
                break
            objective = n_ * (d_ * np.log(ss) + np.trace(sx) + logpiv) + np.trace(S) - missing * np.log(ss_old)
            rel = abs(dtype(1) - objective / old)
            old = objective
            count += 1
            out["rels"].append(float(rel))
            out["objectives"].append(float(objective))
            if rel < threshold and count > 5:
                status = OK
            elif count > maxits:
                status = MAXITS
        out["iters"] = count - 1
        out["status"] = status
        if status == NUMERIC:
            return out
        out["rel"] = out["rels"][-1]
        q, bad = orthonormalise(C)
        if bad:
            out["status"] = NUMERIC
            return out
        t = ye @ q
        s = t.sum(axis=0)
        cov = (t.T @ t - s[:, None] * s[None, :] / n_) / (n_ - dtype(1))
        if dtype is np.float64:
            vals, vecs = np.linalg.eigh(cov)
        else:
            vals, vecs = jacobi_eigh(cov)
        order = np.argsort(-vals, kind="stable")
        C = q @ vecs[:, order]
        X = ye @ C
        den = (np.where(obs, ye, dtype(0)) ** 2).sum()
        r2 = np.empty(d, dtype)
        for i in range(1, d + 1):
            e = np.where(obs, ye - X[:, :i] @ C[:, :i].T, dtype(0))
            r2[i - 1] = dtype(1) - (e * e).sum() / den
        f = X @ C[0] + M[0]
    out.update(r2cum=np.asarray(r2, np.float64), fit=np.asarray(f, np.float64), fit_ld=f, C=np.asarray(C, np.float64),
               M=np.asarray(M, np.float64), ss=float(ss))
    if trace:
        out["last_fill"] = ye_prev_fill
    return out


def jacobi_eigh(a, sweeps=30):
    """Cyclic Jacobi in the matrix' own dtype (numpy's eigh has no longdouble): (eigenvalues, eigenvectors in columns)."""
    a = np.array(a)
    n = a.shape[0]
    v = np.eye(n, dtype=a.dtype)
    for _ in range(sweeps):
        off = np.sqrt((np.tril(a, -1) ** 2).sum())
        if off == 0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if a[p, q] == 0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
                t = np.sign(theta) / (abs(theta) + np.sqrt(theta * theta + 1)) if theta != 0 else a.dtype.type(1)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                ap, aq = a[:, p].copy(), a[:, q].copy()
                a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
                ap, aq = a[p].copy(), a[q].copy()
                a[p], a[q] = c * ap - s * aq, s * ap + c * aq
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(a).copy(), v


def round_half_even(x):
    return int(round(float(x)))


def first_npcs(D, frac_obs, bound):
    return min(max(2, round_half_even((D - 1) * frac_obs)), bound)


def add_npcs(r2cum, max_r2cum):
    """The components ``run_ppca`` adds after a fit that misses ``max_r2cum`` (:276-277)."""
    last = r2cum[-1]
    r2last = r2cum[-1] - r2cum[-2] if len(r2cum) > 1 else r2cum[-1]
    with np.errstate(all="ignore"):
        q = np.float64(max_r2cum - last) / np.float64(r2last)
    if q >= 10:
        return 10
    if not q >= 1:                                                  # below 1, negative or NaN
        return 1
    return max(1, min(10, round_half_even(q)))


def search(y, c0_of=None, npcs=0, frac_obs=0.5, max_r2cum=0.99, threshold=1e-5, maxits=1000, dtype=np.float64,
           max_pcs=MAX_PCS):
    """``run_ppca`` on one standardised matrix: a dict of the final fit's record plus npcs, nfits, r2_not_reached, r2max
    (the largest R2cum of every fit) and every fit's rels.  ``c0_of(D, d)`` gives the start (default ``default_c0``)."""
    N, D = y.shape
    c0_of = default_c0 if c0_of is None else c0_of
    log = dict(nfits=0, r2max=[], rels=[])

    def run(k):
        log["nfits"] += 1
        r = fit(y, k, c0_of(D, k), threshold, maxits, dtype)
        log["rels"].extend(r["rels"])
        if r["status"] in (OK, MAXITS):
            log["r2max"].append(float(np.max(r["r2cum"])))
        return r

    def done(r, k, flag=False):
        return dict(r, npcs=k, nfits=log["nfits"], r2_not_reached=flag, r2max=log["r2max"], all_rels=log["rels"])

    if npcs != 0:
        return done(run(npcs), npcs)
    bound = min(D - 1, max_pcs)
    k = first_npcs(D, frac_obs, bound)
    cache = {}
    flag = False
    while True:
        r = cache[k] if k in cache else run(k)
        if r["status"] not in (OK, MAXITS):
            return done(r, k)
        if np.max(r["r2cum"]) >= max_r2cum:
            n = int(np.nonzero(r["r2cum"] >= max_r2cum)[0][0]) + 1
            if n != k:
                k = n
                r = cache[k] if k in cache else run(k)
            break
        if k >= bound:
            flag = True
            break
        cache[k] = r
        k = min(k + add_npcs(r["r2cum"], max_r2cum), bound)
    if k == 1 and cache and max(cache) > 1:                          # the "bogus PC1" rule (:286-298)
        k = max(cache)
        r = cache[k]
    return done(r, k, flag)


def closed_form(y, d):
    """Tipping and Bishop's fixed point for complete data: (ss, fit of column 0): ss = the mean of the discarded eigenvalues
    of the divisor-N covariance; the fit is the projection on the leading d eigenvectors."""
    y = np.asarray(y, np.float64)
    m = y.mean(axis=0)
    yc = y - m
    vals, vecs = np.linalg.eigh(yc.T @ yc / y.shape[0])
    order = np.argsort(-vals)
    u = vecs[:, order[:d]]
    return float(vals[order[d:]].mean()), (yc @ u) @ u[0] + m[0]


def margin(values, bound):
    """The smallest relative distance of a value from ``bound``."""
    v = np.asarray(values, np.float64)
    return float(np.min(np.abs(v - bound) / abs(bound))) if v.size else np.inf
