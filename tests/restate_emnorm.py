"""The numpy restatement of the mean / variance estimator of step14 (``norm``'s EM as include/twx_qa.h, ``twxem_mean_variance``,
states it; Schafer 1997, section 5.3): the checker of the GPU kernels.  ``dtype`` is ``np.float64`` or ``np.longdouble``.

    x [n, P], column 0 the target, NaN (any non-finite value) = missing, P <= 31
    1. per column over its finite values: cnt, xbar = sum / cnt, sdv = sqrt((sum x^2 - (sum x)^2 / cnt) / cnt), 0 -> 1;
       z = (x - xbar) / sdv
    2. theta [(P + 1), (P + 1)]: theta[0][0] = -1, theta[0][j] = mu_j = 0, theta[j][k] = sigma_jk = I
    3. one iteration: rows grouped by their mask of finite columns; for every pattern W = theta swept on every observed k
       in ascending k from a fresh copy of theta (sweep on k: r = 1 / W[k][k], c = W[:, k]; W -= (c c') r;
       W[:, k] = W[k, :] = c r; W[k][k] = -r); the completed row is z on the observed columns and W[0][m] + sum_o W[o][m] z_o
       on a missing m; T = sum of [1, zhat]' [1, zhat], plus W[j][k] for j, k missing, per row; mu = T[0] / n,
       sigma = T / n - mu mu'; delta = the largest absolute change of an element of theta
    4. stop at delta <= criterion (OK) or after maxits iterations (MAXITS); a pivot <= 0 or not finite: NUMERIC, NaN
    5. mean = mu_0 sdv_0 + xbar_0, variance = sigma_00 sdv_0^2

``iters`` counts completed iterations (the one a pivot failed in is not counted).  ``run`` returns every iteration's delta.
"""
import numpy as np

OK, NUMERIC, MAXITS, NO_MATRIX, EMPTY_COLUMN, ROW_CAP = 0, 4, 20, 21, 22, 23
MAX_COLS = 31


def standardise(x, dtype=np.float64):
    """(z [n, P] with NaN where missing, finite mask, cnt, xbar, sdv)."""
    x = np.asarray(x, dtype)
    fin = np.isfinite(x)
    x0 = np.where(fin, x, dtype(0))
    cnt = fin.sum(axis=0)
    with np.errstate(all="ignore"):
        c = cnt.astype(dtype)
        s1, s2 = x0.sum(axis=0), (x0 * x0).sum(axis=0)
        xbar = s1 / c
        sdv = np.sqrt((s2 - s1 * s1 / c) / c)
        sdv = np.where(sdv == 0, dtype(1), sdv)
        z = np.where(fin, (x0 - xbar) / sdv, dtype(0))
    return z, fin, cnt, xbar, sdv


def patterns(fin):
    """(masks [npat] ascending, pattern index of every row, rows per pattern, observed flags [npat, P])."""
    P = fin.shape[1]
    mask = (fin.astype(np.uint64) << np.arange(P, dtype=np.uint64)).sum(axis=1)
    masks, pidx, cnt = np.unique(mask, return_inverse=True, return_counts=True)
    obs = ((masks[:, None] >> np.arange(P, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return masks, pidx.ravel(), cnt, obs


def sweep_patterns(theta, obs):
    """W [npat, D, D]: theta swept on the observed columns of each pattern, ascending, from a fresh copy; ``bad`` is True if a
    pivot was <= 0 or not finite."""
    npat, P = obs.shape
    W = np.repeat(theta[None], npat, axis=0)
    for k in range(1, P + 1):
        sel = np.nonzero(obs[:, k - 1])[0]
        if sel.size == 0:
            continue
        Wk = W[sel]
        d = Wk[:, k, k]
        if not np.all(np.isfinite(d) & (d > 0)):
            return W, True
        r = 1 / d
        c = Wk[:, :, k].copy()
        Wk = Wk - (c[:, :, None] * c[:, None, :]) * r[:, None, None]
        Wk[:, :, k] = c * r[:, None]
        Wk[:, k, :] = c * r[:, None]
        Wk[:, k, k] = -r
        W[sel] = Wk
    return W, False


def iterate(theta, z, fin, pidx, pcnt, obs):
    """One EM iteration: (new theta, bad)."""
    dtype = theta.dtype.type
    n, P = z.shape
    W, bad = sweep_patterns(theta, obs)
    if bad:
        return theta, True
    Wr = W[pidx]                                                  # [n, D, D]
    pred = Wr[:, 0, 1:] + np.einsum("ro,rom->rm", z, Wr[:, 1:, 1:] * fin[:, :, None])
    zhat = np.where(fin, z, pred)
    y = np.concatenate([np.ones((n, 1), dtype), zhat], axis=1)
    T = np.einsum("ri,rj->ij", y, y)
    mis = np.concatenate([np.zeros((obs.shape[0], 1), bool), ~obs], axis=1)
    T = T + ((W * (mis[:, :, None] & mis[:, None, :])) * pcnt.astype(dtype)[:, None, None]).sum(axis=0)
    new = np.empty_like(theta)
    mu = T[0, 1:] / dtype(n)
    new[0, 0] = -1
    new[0, 1:] = new[1:, 0] = mu
    new[1:, 1:] = T[1:, 1:] / dtype(n) - mu[:, None] * mu[None, :]
    return new, False


def run(x, criterion=1e-4, maxits=1000, dtype=np.float64, full=False):
    """The estimator on one matrix.  Returns a dict: mean, variance, iters, status, delta (the last), deltas (every
    iteration's), sd0 (the target column's sdv: the unit of the mean's tolerance) and, with ``full``, mu [P] and sigma [P, P]
    on the original scale and theta."""
    x = np.asarray(x, np.float64)
    n, P = x.shape
    if not 1 <= P <= MAX_COLS:
        raise ValueError("1 .. %d columns" % MAX_COLS)
    if criterion <= 0 or maxits <= 0:
        raise ValueError("criterion and maxits must be positive")
    nan = float("nan")
    out = dict(mean=nan, variance=nan, iters=0, status=OK, delta=nan, deltas=[], sd0=nan)
    z, fin, cnt, xbar, sdv = standardise(x, dtype)
    if (cnt == 0).any():
        out["status"] = EMPTY_COLUMN
        return out
    out["sd0"] = float(sdv[0])
    _, pidx, pcnt, obs = patterns(fin)
    theta = np.zeros((P + 1, P + 1), dtype)
    theta[0, 0] = -1
    theta[1:, 1:] = np.eye(P, dtype=dtype)
    status = MAXITS
    with np.errstate(all="ignore"):
        for it in range(1, maxits + 1):
            new, bad = iterate(theta, z, fin, pidx, pcnt, obs)
            if bad:
                status = NUMERIC
                break
            delta = np.abs(new - theta).max()
            theta = new
            out["iters"] = it
            out["deltas"].append(float(delta))
            if delta <= criterion:
                status = OK
                break
    out["status"] = status
    if status == NUMERIC:
        return out
    out["delta"] = out["deltas"][-1]
    out["mean"] = float(theta[0, 1] * sdv[0] + xbar[0])
    out["variance"] = float(theta[1, 1] * sdv[0] * sdv[0])
    out["mean_ld"], out["variance_ld"] = theta[0, 1] * sdv[0] + xbar[0], theta[1, 1] * sdv[0] * sdv[0]
    if full:
        out["mu"] = np.asarray(theta[0, 1:] * sdv + xbar, np.float64)
        out["sigma"] = np.asarray(theta[1:, 1:] * sdv[:, None] * sdv[None, :], np.float64)
        out["theta"] = theta
    return out


def loglik(x, mu, sigma):
    """The observed-data log-likelihood of N(mu, sigma) on x (NaN = missing), up to its constant."""
    x = np.asarray(x, np.float64)
    fin = np.isfinite(x)
    _, pidx, _, obs = patterns(fin)
    ll = 0.0
    for p in range(obs.shape[0]):
        o = np.nonzero(obs[p])[0]
        if o.size == 0:
            continue
        rows = x[pidx == p][:, o] - mu[o]
        S = sigma[np.ix_(o, o)]
        _, logdet = np.linalg.slogdet(S)
        ll += -0.5 * (rows.shape[0] * logdet + np.einsum("ri,ij,rj->", rows, np.linalg.inv(S), rows))
    return ll


def margin(deltas, criterion):
    """The smallest relative distance of an iteration's delta from the criterion."""
    d = np.asarray(deltas, np.float64)
    return float(np.min(np.abs(d - criterion) / criterion)) if d.size else np.inf
