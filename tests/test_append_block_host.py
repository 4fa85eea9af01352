"""Host tests of the block append (cbo_gp_append_block): the ABI, and the formulas the header states,
restated in numpy (`append_block` below) and checked against the fp64 oracle fitted on the grown data: the factor, z, and
q = sum V^2, mu = V^T z of 300 candidates.

Tolerance.  Both sides are backward-stable fp64 Cholesky computations on the same Ky (Higham, Accuracy and Stability, Thm
10.3 / 10.4: the computed factor is the exact factor of Ky + dK, |dK| <= c n eps |Ky|), so factor and solutions agree to a
modest multiple of n eps cond(Ky): the bound used is C n eps cond(Ky) with C = 4, times the scale of the quantity (max |L|,
max |z|, the prior variance for q, max |y - m| for mu)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg

from conftest import ROOT
from oracle import gp_oracle as O

EPS = 2.220446049250313e-16
C = 4.0


def header_text():
    with open(os.path.join(ROOT, "include", "cbo_hip.h")) as fh:
        return fh.read()


def test_header_declares_the_block_append():
    text = header_text()
    m = re.search(r"int\s+cbo_gp_append_block\s*\(([^;]*)\)\s*;", text)
    assert m, "include/cbo_hip.h does not declare cbo_gp_append_block"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 7
    assert re.search(r"#define\s+CBO_MAX_APPEND\s+64\b", text)
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)


def test_library_exports_the_block_append_and_lib_binds_it():
    from cbo_with_oop_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "cbo_gp_append_block"), "libcbo_hip.so does not export cbo_gp_append_block"
    assert "cbo_gp_append_block" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["cbo_gp_append_block"]
    P = _lib.c_double_p
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_int, P, P, P, P, _lib.c_int_p]
    assert _lib.MAX_APPEND == 64 and _lib.ABI_VERSION == 5


def test_wrapper_has_append_block():
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    assert callable(getattr(HipGaussianProcess, "append_block", None))


# ---- the contract's formulas ------------------------------------------------------------------------------------------------
def append_block(L, z, X, vX, Xb, yb, mb, vb, variance, lengthscale, noise_var):
    """include/cbo_hip.h, cbo_gp_append_block: (L_grown, z_grown, B, L22, zb)."""
    n, k = L.shape[0], Xb.shape[0]
    sigma = noise_var + O.GPY_DIAG_JITTER
    B = scipy.linalg.solve_triangular(L, O.causal_K(X, Xb, vX, vb, variance, lengthscale, False), lower=True)
    S = O.causal_K(Xb, Xb, vb, vb, variance, lengthscale, False)                # X2 explicit
    S[np.diag_indices(k)] = O.causal_Kdiag(k, vb, variance)                    # the diagonal prior term is Kdiag
    S = S + sigma * np.eye(k) - B.T @ B
    L22 = np.linalg.cholesky(S)
    zb = scipy.linalg.solve_triangular(L22, (yb - (0.0 if mb is None else mb)) - B.T @ z, lower=True)
    Lg = np.zeros((n + k, n + k))
    Lg[:n, :n] = L
    Lg[n:, :n] = B.T                                                            # U[0:n, n:n+k] = B
    Lg[n:, n:] = L22                                                            # U[n:n+k, n:n+k] = L22^T
    return Lg, np.concatenate([z, zb]), B, L22, zb


def extend_rows(V, q, mu, B, L22, zb, Kb):
    """The k new rows of a resident V and what they add to q, mu (r in row order)."""
    W = scipy.linalg.solve_triangular(L22, Kb - B.T @ V, lower=True)
    q, mu = q.copy(), mu.copy()
    for r in range(W.shape[0]):
        q += W[r] ** 2
        mu += W[r] * zb[r]
    return np.vstack([V, W]), q, mu


@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("causal", [False, True])
def test_formulas_match_the_oracle_on_the_grown_data(causal, k):
    n0, d, m = 90, 2, 300
    rng = np.random.default_rng(100 * k + causal)
    X = rng.uniform(-2, 2, (n0 + k, d))
    y = np.sin(X[:, 0]) + 0.3 * np.cos(2 * X[:, 1]) + 0.05 * rng.standard_normal(n0 + k)
    Xs = rng.uniform(-2, 2, (m, d))
    mean = (lambda a: 0.1 * a[:, 0]) if causal else None
    vadj = (lambda a: 0.2 + 0.1 * np.cos(a[:, 1]) ** 2) if causal else None
    mX, vX = (mean(X), vadj(X)) if causal else (None, None)
    vXs = vadj(Xs) if causal else None
    hyper = dict(variance=1.3, lengthscale=0.9, noise_var=1e-2)
    sl = lambda a, lo, hi: None if a is None else a[lo:hi]

    # the parent model through the oracle; its z, V, q, mu
    parent = O.fit(X[:n0], y[:n0], sl(mX, 0, n0), sl(vX, 0, n0), **hyper)
    r0 = y[:n0] - (0.0 if mX is None else mX[:n0])
    z0 = scipy.linalg.solve_triangular(parent.L, r0, lower=True)
    V0 = scipy.linalg.solve_triangular(parent.L, O.causal_K(X[:n0], Xs, sl(vX, 0, n0), vXs, **{k_: hyper[k_] for k_ in
                                                             ("variance", "lengthscale")}), lower=True)
    Lg, zg, B, L22, zb = append_block(parent.L, z0, X[:n0], sl(vX, 0, n0), X[n0:], y[n0:], sl(mX, n0, None),
                                      sl(vX, n0, None), **hyper)
    Kb = O.causal_K(X[n0:], Xs, sl(vX, n0, None), vXs, hyper["variance"], hyper["lengthscale"], False)
    Vg, qg, mug = extend_rows(V0, np.sum(V0 ** 2, 0), V0.T @ z0, B, L22, zb, Kb)

    # the oracle on the grown data
    grown = O.fit(X, y, mX, vX, **hyper)
    assert grown.tries == 0
    r = y - (0.0 if mX is None else mX)
    z_ref = scipy.linalg.solve_triangular(grown.L, r, lower=True)
    V_ref = scipy.linalg.solve_triangular(grown.L, O.causal_K(X, Xs, vX, vXs, hyper["variance"], hyper["lengthscale"],
                                                              False), lower=True)
    Ky = grown.L @ grown.L.T
    bound = C * (n0 + k) * EPS * np.linalg.cond(Ky)
    prior_var = hyper["variance"] + (0.0 if vXs is None else float(np.max(vXs)))
    assert np.max(np.abs(Lg - grown.L)) <= bound * np.max(np.abs(grown.L))
    assert np.max(np.abs(zg - z_ref)) <= bound * np.max(np.abs(z_ref))
    assert np.max(np.abs(qg - np.sum(V_ref ** 2, 0))) <= bound * prior_var
    assert np.max(np.abs(mug - V_ref.T @ z_ref)) <= bound * np.max(np.abs(r))
    # ... and q, mu are the oracle's predictive variance and mean
    mu_o, var_o = O.predict(grown, Xs, None, vXs, include_noise=False)
    kss = O.causal_Kdiag(m, vXs, hyper["variance"])
    assert np.max(np.abs((kss - qg) - var_o[:, 0])) <= bound * prior_var
    assert np.max(np.abs(mug - mu_o[:, 0])) <= bound * np.max(np.abs(r))
