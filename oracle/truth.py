"""ctypes wrapper for oracle/gp_truth_ld.c (extended-precision arbiter; test infrastructure only)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libgp_truth_ld.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _HERE, "libgp_truth_ld.so"])
        lib = ctypes.CDLL(path)
        P = ctypes.POINTER(ctypes.c_double)
        lib.gp_truth_predict.restype = ctypes.c_int
        lib.gp_truth_predict.argtypes = [ctypes.c_long, ctypes.c_int, P, P, P, P, ctypes.c_double, P,
                                         ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_long,
                                         P, P, P, ctypes.c_int, P, P, P]
        _LIB = lib
    return _LIB


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def truth_predict(X, y, Xs, mX=None, vX=None, mXs=None, vXs=None, variance=1.0, lengthscale=1.0,
                  diag_add=1e-10 + 1e-8, noise_var=1e-10, include_noise=True):
    """Posterior mean/var (M,1) and alpha (N,) computed in 80-bit long double."""
    c = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    X = np.ascontiguousarray(X, dtype=np.float64)
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    n, d = X.shape
    m = Xs.shape[0]
    ls = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)).copy()
    ard = int(ls.size > 1)
    y_, mX_, vX_, mXs_, vXs_ = c(y), c(mX), c(vX), c(mXs), c(vXs)
    mean = np.empty(m)
    var = np.empty(m)
    alpha = np.empty(n)
    rc = _lib().gp_truth_predict(n, d, _p(X), _p(y_), _p(mX_), _p(vX_), variance, _p(ls), ard, diag_add,
                                 noise_var, m, _p(Xs), _p(mXs_), _p(vXs_), int(include_noise),
                                 _p(mean), _p(var), _p(alpha))
    if rc != 0:
        raise np.linalg.LinAlgError(f"truth cholesky failed at pivot {rc}")
    return mean[:, None], var[:, None], alpha


def _exact_rbf(X, X2, variance, lengthscale):
    """sigma^2 exp(-r^2/2) with r^2 from DIRECT coordinate differences (accurate to a few eps; GPy's
    |x|^2 + |x'|^2 - 2 x.x' loses eps * |x|^2 absolutely, 1e-9 at the coral graph's T ~ 2475)."""
    ls = np.broadcast_to(np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)), (X.shape[1],))
    r2 = np.zeros((X.shape[0], X2.shape[0]))
    for k in range(X.shape[1]):
        d = (X[:, k][:, None] - X2[:, k][None, :]) / ls[k]
        d *= d
        r2 += d
    r2 *= -0.5
    np.exp(r2, out=r2)
    r2 *= variance
    return r2


def refined_mean(post, Xs, mXs=None, vXs=None, iterations=4, exact_entries=False):
    """Posterior mean K*^T alpha + m(X*) with alpha from ITERATIVE REFINEMENT of Ky alpha = y - m(X): an fp64 Cholesky
    factor is the solver, the residuals are formed in long double (x87 80-bit) against the matrix entries.  Converges
    while eps * cond(Ky) < 1; the refined alpha carries a relative error of a few eps, so the mean no longer carries the
    eps * cond(Ky) * |k*| |alpha| of a plain fp64 solve.  ``exact_entries=False``: the very entries the oracle's fit
    factored (GPy's distance formula) -- arbitrates the SOLVE.  ``exact_entries=True``: entries from direct coordinate
    differences, refactored with the fit's diagonal add and jitter -- the mean of the exact-arithmetic kernel on the same
    inputs, what the all-long-double restatement (gp_truth_predict, O(n^3) scalar work) computes; the arbiter at sizes
    where that one is not affordable (plain models only: no causal rank-1 term).  Test infrastructure only (tests/)."""
    from scipy.linalg import lapack
    from . import gp_oracle as O
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    if exact_entries:
        assert post.vX is None, "exact_entries: plain RBF models only"
        K = _exact_rbf(post.X, post.X, post.variance, post.lengthscale)
        K[np.diag_indices_from(K)] += post.noise_var + O.GPY_DIAG_JITTER + post.jitter
        L, info = lapack.dpotrf(K, lower=1, clean=0, overwrite_a=0)
        assert info == 0, info
        Kx = _exact_rbf(post.X, Xs, post.variance, post.lengthscale)
    else:
        K = O.causal_K(post.X, post.X, post.vX, post.vX, post.variance, post.lengthscale, post.zero_diag)
        K[np.diag_indices_from(K)] += post.noise_var + O.GPY_DIAG_JITTER + post.jitter
        L = post.L
        Kx = O.causal_K(post.X, Xs, post.vX, vXs, post.variance, post.lengthscale, False)
    r = post.y if post.mX is None else post.y - np.asarray(post.mX, dtype=np.float64).reshape(-1, 1)
    rl = r.astype(np.longdouble)
    a0, info = lapack.dpotrs(L, r, lower=1)
    assert info == 0
    alpha = a0.astype(np.longdouble)
    block = 2048                                            # long-double copies of K one row block at a time
    for _ in range(iterations):
        res = np.empty_like(rl)
        for i in range(0, K.shape[0], block):
            res[i:i + block] = rl[i:i + block] - K[i:i + block].astype(np.longdouble) @ alpha
        d, info = lapack.dpotrs(L, np.asarray(res, dtype=np.float64), lower=1)
        assert info == 0
        alpha = alpha + d.astype(np.longdouble)
    mean = np.asarray(Kx.astype(np.longdouble).T @ alpha, dtype=np.float64)
    if mXs is not None:
        mean = mean + np.asarray(mXs, dtype=np.float64).reshape(-1, 1)
    return mean, np.asarray(alpha, dtype=np.float64)


def refined_variance(post, Xs, vXs=None, iterations=4, include_noise=True):
    """Posterior variance at a FEW points for the exact-arithmetic kernel on the oracle's inputs (entries from direct
    coordinate differences, the fit's diagonal add and jitter): kss - k*^T Ky^-1 k* with Ky w = k* solved by iterative
    refinement (fp64 Cholesky factor as the solver, long-double residuals) and the final inner product in long double.
    The arbiter of the variance at sizes where the all-long-double restatement (gp_truth_predict) is not affordable;
    O(n^2 m) long-double work per iteration, so keep m small (tens).  Plain RBF models only.  Test infrastructure only."""
    from scipy.linalg import lapack
    from . import gp_oracle as O
    assert post.vX is None, "plain RBF models only"
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    K = _exact_rbf(post.X, post.X, post.variance, post.lengthscale)
    K[np.diag_indices_from(K)] += post.noise_var + O.GPY_DIAG_JITTER + post.jitter
    L, info = lapack.dpotrf(K, lower=1, clean=0, overwrite_a=0)
    assert info == 0, info
    Kx = _exact_rbf(post.X, Xs, post.variance, post.lengthscale)
    kl = Kx.astype(np.longdouble)
    w0, info = lapack.dpotrs(L, Kx, lower=1)
    assert info == 0
    w = w0.astype(np.longdouble)
    block = 1024
    for _ in range(iterations):
        res = np.empty_like(kl)
        for i in range(0, K.shape[0], block):
            res[i:i + block] = kl[i:i + block] - K[i:i + block].astype(np.longdouble) @ w
        d, info = lapack.dpotrs(L, np.asarray(res, dtype=np.float64), lower=1)
        assert info == 0
        w = w + d.astype(np.longdouble)
    var = np.longdouble(post.variance) - np.sum(kl * w, axis=0)
    var = np.maximum(var, np.longdouble(O.GPY_VAR_CLIP))
    if include_noise:
        var = var + np.longdouble(post.noise_var)
    return np.asarray(var, dtype=np.float64)[:, None]


# ------------------------------------------------------------------ long-double linear algebra on GIVEN fp64 factors
# (oracle/gp_linalg_ld.c): the device's own L, alpha go in, so that a test measures one stage of the device at a time.
_LINALG = None


def _linalg():
    global _LINALG
    if _LINALG is None:
        path = os.path.join(_HERE, "libgp_linalg_ld.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _HERE, "libgp_linalg_ld.so"])
        lib = ctypes.CDLL(path)
        P = ctypes.POINTER(ctypes.c_double)
        PL = ctypes.POINTER(ctypes.c_longdouble)
        PI = ctypes.POINTER(ctypes.c_long)
        lib.ld_backward_error_rows.restype = ctypes.c_int
        lib.ld_backward_error_rows.argtypes = [ctypes.c_long, P, P, PI, ctypes.c_long, PL, PI, PI]
        lib.ld_solve_many.restype = ctypes.c_int
        lib.ld_solve_many.argtypes = [ctypes.c_long, P, ctypes.c_long, P, P, P, PL, PL, PL, P]
        lib.ld_lml_gradients.restype = ctypes.c_int
        lib.ld_lml_gradients.argtypes = [ctypes.c_long, ctypes.c_int, P, P, P, P, ctypes.c_double, P, ctypes.c_int,
                                         PL, PL, PL]
        lib.ld_prediction_gradients.restype = ctypes.c_int
        lib.ld_prediction_gradients.argtypes = [ctypes.c_long, ctypes.c_int, P, P, P, ctypes.c_long, P, P, P,
                                                ctypes.c_double, P, ctypes.c_int, PL, PL, PL, PL]
        _LINALG = lib
    return _LINALG


def _c64(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a if shape is None else a.reshape(shape)


def _pl(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_longdouble))


def _check_rc(rc, what):
    if rc != 0:
        raise np.linalg.LinAlgError(f"{what}: non-positive pivot or diagonal at row {rc - 1}" if rc > 0 else
                                    f"{what}: invalid argument or out of memory")


def _hyper(X, lengthscale):
    X = _c64(X)
    if X.ndim == 1:
        X = X[:, None]
    ls = np.atleast_1d(_c64(lengthscale)).copy()
    return X, ls, int(ls.size > 1)


def backward_error_rows(L, A, rows):
    """max over the sampled rows i and all j of |(L L^T - A)_ij| / sqrt(A_ii A_jj), in long double (only the lower
    triangle of L is read).  Returns (value as numpy.longdouble, (i, j) where it is reached).  O(n^2 |rows|)."""
    L, A = _c64(L), _c64(A)
    n = L.shape[0]
    assert L.shape == A.shape == (n, n)
    rows = np.ascontiguousarray(np.unique(np.asarray(rows, dtype=np.int64)), dtype=np.int64)
    out = np.zeros(1, dtype=np.longdouble)
    bi, bj = ctypes.c_long(-1), ctypes.c_long(-1)
    rc = _linalg().ld_backward_error_rows(n, _p(L), _p(A), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_long)),
                                          rows.size, _pl(out), ctypes.byref(bi), ctypes.byref(bj))
    _check_rc(rc, "backward_error_rows")
    return out[0], (bi.value, bj.value)


def solve_many(L, B, z=None, r=None, return_v=False):
    """v_k = L^-1 b_k for every column of B (n, m), in long double: returns (q, mu) with q_k = sum v_k^2 and
    mu_k = v_k^T z (numpy.longdouble arrays; mu is None without z or r) -- the two reductions of the sweep
    (kernels_trsm.hip).  ``z`` is taken as given; ``r`` instead: z = L^-1 r in long double.  ``return_v``: V rounded to
    fp64 as a third result."""
    L = _c64(L)
    n = L.shape[0]
    B = _c64(B)
    if B.ndim == 1:
        B = B[:, None]
    m = B.shape[1]
    assert B.shape[0] == n
    q = np.zeros(m, dtype=np.longdouble)
    mu = np.zeros(m, dtype=np.longdouble) if (z is not None or r is not None) else None
    V = np.empty((n, m)) if return_v else None
    z_, r_ = _c64(z, (-1,)), (None if z is not None else _c64(r, (-1,)))
    rc = _linalg().ld_solve_many(n, _p(L), m, _p(B), _p(z_), _p(r_), _pl(q), _pl(mu), None, _p(V))
    _check_rc(rc, "solve_many")
    return (q, mu, V) if return_v else (q, mu)


def lml_and_gradients(L, X, y, mX=None, vX=None, variance=1.0, lengthscale=1.0):
    """Log marginal likelihood and its gradients (gp_oracle.log_marginal_likelihood_gradients restated) with every
    solve on the GIVEN factor L: alpha = (L L^T)^-1 (y - m(X)), log det = 2 sum log L_ii, W = (L L^T)^-1 formed from L,
    1/2 tr((alpha alpha^T - W) dK) contracted in long double with kernel entries from direct coordinate differences.
    O(n^3) long-double work: n <= ~2100.  Returns (values, magnitudes), dicts of numpy.longdouble with keys lml,
    d_variance, d_noise (scalars) and d_lengthscale (array); the magnitudes are the same sums over absolute terms."""
    L = _c64(L)
    n = L.shape[0]
    X, ls, ard = _hyper(X, lengthscale)
    d = X.shape[1]
    r = _c64(y, (-1,)) - (0.0 if mX is None else _c64(mX, (-1,)))
    r = np.ascontiguousarray(r)
    nl = d if ard else 1
    out = np.zeros(3 + nl, dtype=np.longdouble)
    mag = np.zeros(3 + nl, dtype=np.longdouble)
    rc = _linalg().ld_lml_gradients(n, d, _p(L), _p(X), _p(r), _p(_c64(vX, (-1,))), float(variance), _p(ls), ard,
                                    _pl(out), _pl(mag), None)
    _check_rc(rc, "lml_and_gradients")
    unpack = lambda a: {"lml": a[0], "d_variance": a[1], "d_noise": a[2], "d_lengthscale": a[3:].copy()}
    return unpack(out), unpack(mag)


def prediction_gradients(L, alpha, X, Xs, vX=None, vXs=None, variance=1.0, lengthscale=1.0):
    """(dmean (M,d), dvar (M,d)) of gp_oracle.predict_gradients with the solves Ky^-1 k(X, x*) on the GIVEN factor L
    and the GIVEN alpha, in long double; plus their magnitudes (the same sums over absolute terms).  Returns
    (dmean, dvar, mag_mean, mag_var), numpy.longdouble arrays."""
    L = _c64(L)
    n = L.shape[0]
    X, ls, ard = _hyper(X, lengthscale)
    Xs = _c64(Xs)
    d = X.shape[1]
    m = Xs.shape[0]
    outs = [np.zeros((m, d), dtype=np.longdouble) for _ in range(4)]
    rc = _linalg().ld_prediction_gradients(n, d, _p(L), _p(_c64(alpha, (-1,))), _p(X), m, _p(Xs),
                                           _p(_c64(vX, (-1,))), _p(_c64(vXs, (-1,)) if vX is not None else None),
                                           float(variance), _p(ls), ard, *(_pl(a) for a in outs))
    _check_rc(rc, "prediction_gradients")
    return tuple(outs)
