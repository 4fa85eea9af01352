"""CPU tests of the absolute-accuracy machinery: the long-double routines of oracle/gp_linalg_ld.c against mpmath at 40
digits (small n) and against scipy / LAPACK (n = 300), and the decision helpers of tests/accuracy_support.py shown
SHARP: they accept LAPACK's factor and a legitimately different (right-looking blocked) one, and reject a factor with
one 128 x 128 tile rounded through fp32, a factor whose diagonal is off by 2e-14, and a substitution with one 32-row
stage rounded through fp32 -- what the GPU gates of tests/test_accuracy_gpu.py would then see from a subtly wrong kernel."""
import mpmath
import numpy as np
import pytest
import scipy.linalg

from accuracy_support import (EPS, check_alpha, check_factor, check_gradients, check_solves, lapack_factor,
                              sample_rows)
from oracle import gp_oracle as O
from oracle import truth as T

mp = mpmath.mp


def _problem(n, d, seed, noise=1e-1, causal=False, ard=False):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X).sum(1) + 0.1 * rng.standard_normal(n)
    mX = 0.3 * X[:, 0] if causal else None
    vX = rng.uniform(0.1, 0.5, n) if causal else None
    ls = rng.uniform(0.7, 1.5, d) if ard else 1.1
    K = O.causal_K(X, X, vX, vX, 1.3, ls)
    K[np.diag_indices(n)] += noise
    return X, y, mX, vX, ls, K, np.linalg.cholesky(K)


def _mp_kernel(a, b, variance, ls, ard):
    r2 = mp.mpf(0)
    g = [mp.mpf(0)] * len(a)
    for k in range(len(a)):
        l = mp.mpf(float(ls[k] if ard else ls))
        diff = mp.mpf(float(a[k])) - mp.mpf(float(b[k]))
        r2 += (diff / l) ** 2
        g[k] = diff * diff / l ** 3
    return mp.mpf(variance) * mp.exp(-r2 / 2), (g if ard else [sum(g)])


def _mp_fwd(L, b):
    n = len(b)
    v = [mp.mpf(0)] * n
    for i in range(n):
        v[i] = (b[i] - sum((mp.mpf(float(L[i, k])) * v[k] for k in range(i)), mp.mpf(0))) / mp.mpf(float(L[i, i]))
    return v


def _mp_bwd(L, z):
    n = len(z)
    x = [mp.mpf(0)] * n
    for i in reversed(range(n)):
        x[i] = (z[i] - sum((mp.mpf(float(L[k, i])) * x[k] for k in range(i + 1, n)), mp.mpf(0))) / mp.mpf(float(L[i, i]))
    return x


def _rel(a, b, scale):
    """|a - b| / scale, a a numpy.longdouble (printed with every digit), b an mpf; a zero scale means a zero b"""
    diff = abs(mp.mpf(np.format_float_scientific(np.longdouble(a), unique=True)) - b)
    return float(diff / scale) if scale != 0 else float(diff)


@pytest.mark.parametrize("n", [1, 2, 7, 12])
def test_backward_error_and_solves_agree_with_mpmath(n):
    with mp.workdps(40):
        X, y, mX, vX, ls, K, L = _problem(n, 2, seed=n)
        Lp = L.copy()
        Lp[np.tril_indices(n, -1)] *= 1 + 3e-13 * np.random.default_rng(n).standard_normal(n * (n - 1) // 2)
        rows = np.arange(n)
        be, _ = T.backward_error_rows(Lp, K, rows)
        ref = max(abs(sum((mp.mpf(float(Lp[i, k])) * mp.mpf(float(Lp[j, k])) for k in range(min(i, j) + 1)), mp.mpf(0))
                      - mp.mpf(float(K[i, j]))) / mp.sqrt(mp.mpf(float(K[i, i])) * mp.mpf(float(K[j, j])))
                  for i in range(n) for j in range(n))
        assert _rel(be, ref, 1) <= 1e-17 and (n == 1 or ref > 0)
        B = np.random.default_rng(n + 1).standard_normal((n, 5))
        q, mu = T.solve_many(L, B, r=y)
        z = _mp_fwd(L, [mp.mpf(float(v)) for v in y])
        for c in range(5):
            v = _mp_fwd(L, [mp.mpf(float(b)) for b in B[:, c]])
            q_ref = sum(t * t for t in v)
            mu_ref = sum(a * b for a, b in zip(v, z))
            assert _rel(q[c], q_ref, q_ref) <= 1e-17
            assert _rel(mu[c], mu_ref, sum(abs(a * b) for a, b in zip(v, z))) <= 1e-17


@pytest.mark.parametrize("n,d,ard,causal", [(1, 1, False, False), (5, 2, False, True), (12, 3, True, False),
                                            (12, 2, True, True)])
def test_likelihood_and_prediction_gradients_agree_with_mpmath(n, d, ard, causal):
    with mp.workdps(40):
        X, y, mX, vX, ls, K, L = _problem(n, d, seed=10 + n, causal=causal, ard=ard)
        val, mag = T.lml_and_gradients(L, X, y, mX, vX, 1.3, ls)
        r = y - (mX if causal else 0.0)
        z = _mp_fwd(L, [mp.mpf(float(v)) for v in r])
        al = _mp_bwd(L, z)
        Lm = mp.matrix([[mp.mpf(float(L[i, j])) if j <= i else 0 for j in range(n)] for i in range(n)])
        Li = mp.inverse(Lm)
        W = Li.T * Li
        sv = [mp.sqrt(mp.mpf(float(v))) for v in vX] if causal else [mp.mpf(0)] * n
        nl = d if ard else 1
        dv, dn, dls = mp.mpf(0), mp.mpf(0), [mp.mpf(0)] * nl
        for i in range(n):
            for j in range(n):
                dk = (al[i] * al[j] - W[i, j]) / 2
                krbf, g = _mp_kernel(X[i], X[j], 1.3, ls, ard)
                dv += dk * (krbf + sv[i] * sv[j])
                dls = [a + dk * krbf * gt for a, gt in zip(dls, g)]
                if i == j:
                    dn += dk
        lml = -(n * mp.log(2 * mp.pi) + 2 * sum(mp.log(mp.mpf(float(L[i, i]))) for i in range(n))
                + sum(mp.mpf(float(r[i])) * al[i] for i in range(n))) / 2
        assert _rel(val["lml"], lml, mag["lml"]) <= 1e-17
        assert _rel(val["d_variance"], dv / mp.mpf(1.3), mag["d_variance"]) <= 1e-17
        assert _rel(val["d_noise"], dn, mag["d_noise"]) <= 1e-17
        for t in range(nl):
            assert _rel(val["d_lengthscale"][t], dls[t], mag["d_lengthscale"][t]) <= 1e-17
        # prediction gradients with the given alpha (fp64-rounded here, as the device hands it over)
        alpha = np.array([float(a) for a in al])
        Xs = np.random.default_rng(n).uniform(-2, 2, (3, d))
        vXs = np.random.default_rng(n + 1).uniform(0.1, 0.5, 3) if causal else None
        dmean, dvar, mm, mv = T.prediction_gradients(L, alpha, X, Xs, vX, vXs, 1.3, ls)
        for c in range(3):
            kx, kr = [], []
            for i in range(n):
                k, _ = _mp_kernel(X[i], Xs[c], 1.3, ls, ard)
                kr.append(k)
                kx.append(k + (sv[i] * mp.sqrt(mp.mpf(float(vXs[c]))) if causal else 0))
            w = _mp_bwd(L, _mp_fwd(L, kx))
            for k in range(d):
                l2 = mp.mpf(float(ls[k] if ard else ls)) ** 2
                t = [kr[i] * (mp.mpf(float(X[i, k])) - mp.mpf(float(Xs[c, k]))) / l2 for i in range(n)]
                assert _rel(dmean[c, k], sum(mp.mpf(float(alpha[i])) * t[i] for i in range(n)), mm[c, k]) <= 1e-17
                assert _rel(dvar[c, k], -2 * sum(w[i] * t[i] for i in range(n)), mv[c, k]) <= 1e-17


@pytest.mark.parametrize("causal,ard", [(False, False), (True, True)])
def test_long_double_routines_agree_with_lapack_at_300(causal, ard):
    n, d = 300, 3
    X, y, mX, vX, ls, K, L = _problem(n, d, seed=3, noise=1e-3, causal=causal, ard=ard)
    rows = sample_rows(n, np.random.default_rng(0))
    be, _ = T.backward_error_rows(L, K, rows)
    be_np = np.max(np.abs(L[rows] @ L.T - K[rows]) / np.sqrt(np.outer(np.diag(K)[rows], np.diag(K))))
    assert 0 < float(be) < 50 * EPS and abs(float(be) - be_np) < 2 * n * EPS
    Xs = np.random.default_rng(4).uniform(-2, 2, (40, d))
    vXs = np.random.default_rng(5).uniform(0.1, 0.5, 40) if causal else None
    Kx = O.causal_K(X, Xs, vX, vXs, 1.3, ls)
    r = y - (mX if causal else 0.0)
    q, mu = T.solve_many(L, Kx, r=r)
    V = scipy.linalg.solve_triangular(L, Kx, lower=True)
    z = scipy.linalg.solve_triangular(L, r, lower=True)
    assert np.allclose(np.asarray(q, dtype=np.float64), np.sum(V * V, 0), rtol=1e-11, atol=0)
    assert np.allclose(np.asarray(mu, dtype=np.float64), V.T @ z, rtol=0, atol=1e-11 * np.max(np.abs(V.T @ z)))
    # the same factor and alpha in the fp64 oracle
    alpha = scipy.linalg.cho_solve((L, True), r)[:, None]
    post = O.Posterior(X, y[:, None], None if mX is None else mX[:, None], vX, 1.3, ls, 0.0, L, alpha, 0.0, 0, False)
    val, mag = T.lml_and_gradients(L, X, y, mX, vX, 1.3, ls)
    d_var, d_ls, d_noise = O.log_marginal_likelihood_gradients(post)
    assert abs(float(val["lml"]) - O.log_marginal_likelihood(post)) < 1e-11 * float(mag["lml"])
    for a, b, s in [(val["d_variance"], d_var, mag["d_variance"]), (val["d_noise"], d_noise, mag["d_noise"])] + \
            list(zip(val["d_lengthscale"], np.atleast_1d(d_ls), mag["d_lengthscale"])):
        assert abs(float(a) - b) < 1e-11 * float(s), (a, b, s)
    dm, dv, mm, mv = T.prediction_gradients(L, alpha, X, Xs, vX, vXs, 1.3, ls)
    dm_o, dv_o = O.predict_gradients(post, Xs, vXs)
    assert np.all(np.abs(np.asarray(dm, dtype=np.float64) - dm_o) < 1e-11 * np.asarray(mm, dtype=np.float64) + 1e-300)
    assert np.all(np.abs(np.asarray(dv, dtype=np.float64) - dv_o) < 1e-11 * np.asarray(mv, dtype=np.float64) + 1e-300)


# ------------------------------------------------------------------------------- sharpness of the decision helpers
def _blocked_right_looking(A, nb=128):
    """Right-looking blocked Cholesky (LAPACK's dpotrf per diagonal block, a TRSM per panel, a SYRK of the trailing
    matrix): a legitimate other order of the same operations."""
    A = np.array(A, dtype=np.float64, copy=True)
    n = A.shape[0]
    for k in range(0, n, nb):
        e = min(k + nb, n)
        A[k:e, k:e] = np.linalg.cholesky(A[k:e, k:e])
        if e < n:
            A[e:, k:e] = scipy.linalg.solve_triangular(A[k:e, k:e], A[e:, k:e].T, lower=True).T
            A[e:, e:] -= A[e:, k:e] @ A[e:, k:e].T
    return np.tril(A)


def _staged_solve(L, B, stage=32, round_stage=None):
    """Blocked forward substitution, 32-row stages; ``round_stage``: that stage's rows of V rounded through fp32 before
    the later stages use them."""
    V = np.zeros_like(B)
    for s0 in range(0, L.shape[0], stage):
        s1 = min(s0 + stage, L.shape[0])
        V[s0:s1] = scipy.linalg.solve_triangular(L[s0:s1, s0:s1], B[s0:s1] - L[s0:s1, :s0] @ V[:s0], lower=True)
        if round_stage is not None and s0 == stage * round_stage:
            V[s0:s1] = V[s0:s1].astype(np.float32)
    return V


@pytest.fixture(scope="module")
def sharp_problem():
    n, noise = 2048, 1e-2
    rng = np.random.default_rng(7)
    X = rng.uniform(-5, 5, (n, 3))
    y = np.sin(X).sum(1) + 0.1 * rng.standard_normal(n)
    Ky = O.causal_K(X, X, None, None, 1.0, 1.0, zero_diag=True)
    Ky[np.diag_indices(n)] += noise + O.GPY_DIAG_JITTER
    L_ref = lapack_factor(Ky)
    Xs = rng.uniform(-5, 5, (256, 3))
    return dict(n=n, noise=noise, X=X, y=y, Ky=Ky, L_ref=L_ref, L=np.tril(L_ref), rows=sample_rows(n, rng), Xs=Xs,
                Kx=O.causal_K(X, Xs, None, None, 1.0, 1.0))


def test_factor_gate_accepts_lapack_and_a_blocked_factor(sharp_problem):
    p = sharp_problem
    ok = check_factor(p["L"], p["Ky"], p["rows"], p["L_ref"])
    assert ok["ok"] and ok["ratio"] == 1.0, ok
    blocked = check_factor(_blocked_right_looking(p["Ky"]), p["Ky"], p["rows"], p["L_ref"])
    assert blocked["ok"], blocked
    alpha = scipy.linalg.cho_solve((_blocked_right_looking(p["Ky"]), True), p["y"])
    a = check_alpha(alpha, p["Ky"], p["y"], p["L_ref"])
    assert a["ok"], a


@pytest.mark.parametrize("defect", ["fp32_tile", "diagonal_2e-14"])
def test_factor_gate_rejects_a_subtly_wrong_factor(sharp_problem, defect):
    p = sharp_problem
    L = p["L"].copy()
    if defect == "fp32_tile":
        L[1024:1152, 512:640] = L[1024:1152, 512:640].astype(np.float32)
    else:
        L[np.diag_indices(p["n"])] *= 1 + 2e-14
    bad = check_factor(L, p["Ky"], p["rows"], p["L_ref"])
    assert not bad["ok"] and bad["ratio"] > 2 * 8, bad
    if defect == "fp32_tile":
        alpha = scipy.linalg.cho_solve((L, True), p["y"])
        a = check_alpha(alpha, p["Ky"], p["y"], p["L_ref"])
        assert not a["ok"], a


def _sweep_like(L, Kx, y, noise, V):
    z = scipy.linalg.solve_triangular(L, y, lower=True)
    return np.clip(1.0 - np.sum(V * V, 0), 1e-15, None) + noise, V.T @ z


def test_solve_gate_accepts_a_staged_solve_and_rejects_an_fp32_stage(sharp_problem):
    p = sharp_problem
    L, Kx, y, noise = p["L"], p["Kx"], p["y"], p["noise"]
    kss = np.ones(Kx.shape[1])
    scale = np.max(np.abs(y))
    var, mean = _sweep_like(L, Kx, y, noise, _staged_solve(L, Kx))
    good = check_solves(L, Kx, y, kss, noise, var, mean, y_scale=scale)
    assert good["ok"], good
    var, mean = _sweep_like(L, Kx, y, noise, _staged_solve(L, Kx, round_stage=20))
    bad = check_solves(L, Kx, y, kss, noise, var, mean, y_scale=scale)
    assert not bad["ok"] and bad["var_dev"] > 10 * bad["var_bound"], bad


def test_gradient_gate_rule():
    truth = np.array([1.0, -2.0, 1e-3], dtype=np.longdouble)
    mag = np.array([10.0, 10.0, 10.0])
    oracle = np.asarray(truth, dtype=np.float64) * (1 + 1e-13)
    assert check_gradients(np.asarray(truth, dtype=np.float64) * (1 + 5e-13), oracle, truth, mag, "x")["ok"]
    assert not check_gradients(np.asarray(truth, dtype=np.float64) * (1 + 1e-11), oracle, truth, mag, "x")["ok"]
    # an exact oracle leaves the eps floor
    assert check_gradients(np.asarray(truth, dtype=np.float64) + 3 * EPS * mag, truth, truth, mag, "x")["ok"]
    assert not check_gradients(np.asarray(truth, dtype=np.float64) + 100 * EPS * mag, truth, truth, mag, "x")["ok"]
