"""A numpy restatement of the route ``twxnr_components`` takes (include/twx_qa.h): standardise, Gram matrix, symmetric
eigen-decomposition, sign rule, cuts, scores -- in float64 with ``np.linalg.eigh`` (``components``), and the same route in
``np.longdouble`` with a Jacobi iteration of its own (``components_longdouble``), which is the yardstick both the executed
reference and the float64 routes are measured against.  Also the error bound of the tests (``score_bound``).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
OK, NOCONV, NONFINITE, CONSTANT, FEW_ROWS = 0, 29, 30, 31, 32


def _sign_and_sort(lam, vec):
    """Eigenvalues descending (ties by index), every eigenvector's largest-magnitude entry (the first of equal ones) made
    positive.  vec: columns."""
    order = np.lexsort((np.arange(lam.size), -lam))
    lam, vec = lam[order], vec[:, order].copy()
    for k in range(lam.size):
        j = int(np.argmax(np.abs(vec[:, k])))
        if vec[j, k] < 0:
            vec[:, k] = -vec[:, k]
    return lam, vec


def cut(var_explain, max_var):
    cum = np.cumsum(var_explain)
    hit = np.nonzero(cum >= max_var)[0]
    return int(hit[0]) + 1 if hit.size else int(var_explain.size)


def standardise(a, dtype=np.float64):
    a = np.asarray(a, np.float32).astype(dtype)
    n = a.shape[0]
    mean = a.sum(axis=0) / dtype(n)
    d = a - mean
    sd = np.sqrt((d * d).sum(axis=0) / dtype(n - 1))
    with np.errstate(all="ignore"):
        return d / sd, mean, sd


def components(a, max_vars=(0.99, 0.90)):
    """a [n, P] float32.  Returns a dict of status, bad_col, ncomp (per cut), var_explain [P], eigval [P], loadings [P, P]
    (component k is row k) and scores [n, P]."""
    a = np.asarray(a, np.float32)
    n, P = a.shape
    if n < 2:
        return dict(status=FEW_ROWS, bad_col=-1)
    fin = np.isfinite(a).all(axis=0)
    if not fin.all():
        return dict(status=NONFINITE, bad_col=int(np.nonzero(~fin)[0][0]))
    z, mean, sd = standardise(a)
    if (sd == 0).any():
        return dict(status=CONSTANT, bad_col=int(np.nonzero(sd == 0)[0][0]))
    g = z.T.dot(z) / (n - 1)
    lam, vec = _sign_and_sort(*np.linalg.eigh(g))
    total = 0.0
    for x in lam:
        total = total + x
    ve = lam / total
    return dict(status=OK, bad_col=-1, ncomp=[cut(ve, v) for v in max_vars], var_explain=ve, eigval=lam, loadings=vec.T.copy(),
                scores=z.dot(vec), mean=mean, sd=sd)


def _jacobi_longdouble(g, v0):
    """The eigen-decomposition of the symmetric longdouble matrix g, started from the float64 eigenvectors v0: cyclic Jacobi
    on v0' g v0 until no off-diagonal entry is above eps(longdouble) x the trace."""
    ld = np.longdouble
    v = v0.astype(ld)
    a = v.T.dot(g).dot(v)
    P = a.shape[0]
    tol = np.finfo(ld).eps * np.trace(a)
    for _ in range(60):
        off = a - np.diag(np.diag(a))
        if np.abs(off).max() <= tol:
            break
        for p in range(P - 1):
            for q in range(p + 1, P):
                if a[p, q] == 0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
                t = (ld(-1) if theta < 0 else ld(1)) / (abs(theta) + np.sqrt(theta * theta + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                for m in (a, v):
                    x, y = m[:, p].copy(), m[:, q].copy()
                    m[:, p], m[:, q] = c * x - s * y, s * x + c * y
                x, y = a[p, :].copy(), a[q, :].copy()
                a[p, :], a[q, :] = c * x - s * y, s * x + c * y
                a[p, q] = a[q, p] = 0
    else:
        raise RuntimeError("the longdouble Jacobi iteration did not converge")
    return np.diag(a).copy(), v


def components_longdouble(a):
    """The same route in ``np.longdouble``: (var_explain [P], eigval [P], scores [n, P]) as longdouble arrays."""
    ld = np.longdouble
    z, _, _ = standardise(a, ld)
    n = z.shape[0]
    g = z.T.dot(z) / ld(n - 1)
    g = (g + g.T) / 2
    _, v0 = np.linalg.eigh(g.astype(np.float64))
    lam, vec = _sign_and_sort(*_jacobi_longdouble(g, v0))
    return lam / lam.sum(), lam, z.dot(vec)


def align(ref, got):
    """``ref`` with every column's sign turned to that of ``got``'s (the sign of a component is arbitrary)."""
    sgn = np.sign(np.sum(np.asarray(ref, np.longdouble) * np.asarray(got, np.longdouble), axis=0))
    sgn[sgn == 0] = 1
    return ref * sgn.astype(ref.dtype)


def column_error(ref, got):
    """max |ref - got| per column after the sign alignment, float64."""
    ref = np.asarray(ref, np.longdouble)
    got = np.asarray(got, np.longdouble)
    return np.abs(align(ref, got) - got).max(axis=0).astype(np.float64)


def score_bound(eigval, scores, e_ref, k):
    """The allowed error of the first k score columns: per component the larger of 100 x e_ref and 100 x eps x (lambda_1 /
    gap) x max |score|, gap the distance of the component's eigenvalue to its nearest neighbour.  The Gram route loses about
    lambda_1 / gap of relative accuracy in a component; the factor 100 covers the constants of the summations (n <= 279 days,
    P = 32 columns) that the first-order estimate leaves out."""
    lam = np.asarray(eigval, np.float64)
    out = np.empty(k)
    for c in range(k):
        gap = min(abs(lam[c] - lam[j]) for j in (c - 1, c + 1) if 0 <= j < lam.size) if lam.size > 1 else lam[0]
        out[c] = max(100.0 * e_ref[c], 100.0 * EPS * (lam[0] / gap) * np.abs(scores[:, c]).max())
    return out


def var_explain_bound(var_explain, e_ref_ve):
    """The allowed error of var_explain: the larger of 100 x e_ref and 100 x eps x var_explain[0] (an eigenvalue of a
    symmetric matrix is perfectly conditioned: its error is that of the matrix, eps x lambda_1 times a constant)."""
    return max(100.0 * float(e_ref_ve), 100.0 * EPS * float(var_explain[0]))
