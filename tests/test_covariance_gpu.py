"""GPU tests of the joint posterior (cbo_gp_predict_cov / cbo_gp_cov_between, kernels_joint.hip) against the numpy
restatement of GPy's full_cov branch and posterior_covariance_between_points:
    K(X1, X2) - (L^-1 K(X, X1))^T (L^-1 K(X, X2))   (+ noise_var I for predict(full_cov=True)),
with GPy's RBF K(X) (zero diagonal distance) for non-causal models and CausalRBF.K (X2 explicit, rank-1 term) for
causal ones (include/cbo_hip.h)."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.linalg

from conftest import load_fixture
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def model(X, y, dtype="f64", **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, dtype=dtype, **kw)


def fixture_model(f):
    ls = f["lengthscale_arg"]
    kw = dict(variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls), noise_var=float(f["noise_var"]))
    if f["mX"] is not None:
        pts = np.vstack([f["X"], f["Xs"]])
        lut_m = {tuple(r): v for r, v in zip(map(tuple, pts), np.vstack([f["mX"], f["mXs"]])[:, 0])}
        lut_v = {tuple(r): v for r, v in zip(map(tuple, pts), np.vstack([f["vX"], f["vXs"]])[:, 0])}
        kw["mean_function"] = lambda a: np.array([[lut_m[tuple(r)]] for r in a])
        kw["variance_adjustment"] = lambda a: np.array([[lut_v[tuple(r)]] for r in a])
    return model(f["X"], f["y"], **kw), kw


def restated_cov(post, X1, X2, v1=None, v2=None, sym=False):
    """numpy: K(X1,X2) - V1^T V2 with V = L^-1 K(X, .), the prior term as GPy evaluates it."""
    causal = post.vX is not None
    ls, var = post.lengthscale, post.variance
    K12 = O.causal_K(X1, X2, v1 if causal else None, v2 if causal else None, var, ls, zero_diag=sym and not causal)
    V1 = scipy.linalg.solve_triangular(post.L, O.causal_K(post.X, X1, post.vX, v1, var, ls), lower=True)
    V2 = V1 if sym else scipy.linalg.solve_triangular(post.L, O.causal_K(post.X, X2, post.vX, v2, var, ls), lower=True)
    return K12 - V1.T @ V2


def oracle_post(f):
    return O.fit(f["X"], f["y"], f["mX"], f["vX"], float(f["variance"]), f["lengthscale_arg"], float(f["noise_var"]))


@pytest.mark.parametrize("name", ["toy_bo_d2", "complete_bo_d3", "graph_ard_d4", "coral_max_d3", "causal_d2",
                                  "jitter_ladder"])
def test_full_covariance_matches_the_restatement(lib, name):
    f = load_fixture(name)
    m, _ = fixture_model(f)
    post = oracle_post(f)
    Xs, sig2, noise = f["Xs"], float(f["variance"]), float(f["noise_var"])
    mean, cov = m.predict(Xs, full_cov=True)
    M = Xs.shape[0]
    assert mean.shape == (M, 1) and cov.shape == (M, M)
    ref = restated_cov(post, Xs, Xs, f["vXs"], f["vXs"], sym=True) + noise * np.eye(M)
    bound = 1e-9 * sig2
    if name == "jitter_ladder":
        # the oracle itself is off by eps * cond(Ky) here: its diagonal's error against the 80-bit arbiter bounds it
        # (|dC_ij| <= sqrt(|dC_ii| |dC_jj|) for the error of a Gram product), with the slack assert_parity uses
        bound += 8.0 * np.max(np.abs(f["var"] - f["var_truth"]))
    err = np.max(np.abs(cov - ref))
    assert err <= bound, (name, err, bound)
    # the mean is cbo_gp_predict's, bit for bit; the covariance is symmetric bit for bit
    mean_p, var_p = m.predict(Xs)
    assert np.array_equal(mean, mean_p)
    assert np.array_equal(cov, cov.T)
    # include_noise touches the diagonal only
    _, cov0 = m.predict(Xs, include_likelihood=False, full_cov=True)
    off = ~np.eye(M, dtype=bool)
    assert np.array_equal(cov0[off], cov[off])
    assert np.array_equal(np.diag(cov0) + noise, np.diag(cov))
    _, lat = m.predict(Xs, include_likelihood=False)
    if f["vX"] is None:
        # the diagonal is the latent variance wherever that is above its clip
        keep = lat[:, 0] > 1e-15
        assert np.max(np.abs(np.diag(cov0)[keep] - lat[keep, 0])) <= 1e-12 * sig2 + (bound if name == "jitter_ladder" else 0)
    else:
        # causal: CausalRBF.K on the diagonal, sigma^2 exp(-r2_ii / 2) + v -- not Kdiag's sigma^2 + v
        r2 = np.diag(O.unscaled_sqdist(Xs, Xs, zero_diag=False)) / float(np.ravel(f["lengthscale"])[0]) ** 2
        quad = np.sum(np.square(scipy.linalg.solve_triangular(
            post.L, O.causal_K(post.X, Xs, post.vX, f["vXs"], sig2, f["lengthscale_arg"]), lower=True)), 0)
        expect = sig2 * np.exp(-0.5 * r2) + f["vXs"][:, 0] - quad
        assert np.max(np.abs(np.diag(cov0) - expect)) <= 1e-9 * sig2
        assert np.any(r2 > 0)


@pytest.mark.parametrize("name", ["complete_bo_d3", "graph_ard_d4", "causal_d2"])
def test_covariance_between_points(lib, name):
    f = load_fixture(name)
    m, _ = fixture_model(f)
    post = oracle_post(f)
    sig2 = float(f["variance"])
    X1, X2 = f["Xs"][:37], f["Xs"][40:130]
    v1 = f["vXs"][:37] if f["vXs"] is not None else None
    v2 = f["vXs"][40:130] if f["vXs"] is not None else None
    c12 = m.posterior_covariance_between_points(X1, X2)
    assert c12.shape == (37, 90)
    assert np.max(np.abs(c12 - restated_cov(post, X1, X2, v1, v2))) <= 1e-9 * sig2
    c21 = m.get_covariance_between_points(X2, X1)
    assert np.max(np.abs(c12 - c21.T)) <= 1e-12 * sig2
    Xs = f["Xs"][:150]
    cxx = m.posterior_covariance_between_points(Xs, Xs)
    _, cov0 = m.predict(Xs, include_likelihood=False, full_cov=True)
    off = ~np.eye(Xs.shape[0], dtype=bool)
    assert np.max(np.abs(cxx[off] - cov0[off])) <= 1e-12 * sig2


def random_problem(n, m, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.0, 2.0, (m, d))
    return X, y, Xs


@pytest.mark.parametrize("n", [1, 7, 129, 300, 1000])
def test_ragged_sizes(lib, n):
    for m_pts in (1, 63, 65, 200, 1000):
        X, y, Xs = random_problem(n, m_pts, seed=n + m_pts)
        g = model(X, y, noise_var=1e-2)
        post = O.fit(X, y, noise_var=1e-2)
        _, cov = g.predict(Xs, full_cov=True)
        ref = restated_cov(post, Xs, Xs, sym=True) + 1e-2 * np.eye(m_pts)
        assert np.max(np.abs(cov - ref)) <= 1e-9, (n, m_pts)
        X2 = Xs[: max(1, m_pts // 2)]
        c = g.posterior_covariance_between_points(Xs, X2)
        assert np.max(np.abs(c - restated_cov(post, Xs, X2))) <= 1e-9, (n, m_pts)
        g.close()


def test_large_size_on_sampled_tiles(lib):
    n, m_pts = 4096, 8192
    X, y, Xs = random_problem(n, m_pts, seed=7)
    g = model(X, y, noise_var=1e-2)
    post = O.fit(X, y, noise_var=1e-2)
    mean, cov = g.predict(Xs, full_cov=True)
    assert np.array_equal(cov, cov.T)
    rng = np.random.default_rng(3)
    last = m_pts - 64
    tiles = [(0, 0), (4096, 4096), (last, last), (0, last), (last, 128)] + [tuple(rng.integers(0, m_pts - 64, 2)) for _ in range(3)]
    for i, j in tiles:
        A, B = Xs[i:i + 64], Xs[j:j + 64]
        Ka = O.rbf_K(X, A)
        Kb = O.rbf_K(X, B)
        Va = scipy.linalg.solve_triangular(post.L, Ka, lower=True)
        Vb = scipy.linalg.solve_triangular(post.L, Kb, lower=True)
        K12 = O.rbf_K(A, B)
        if i == j:
            K12 = O.rbf_K(A, A, zero_diag=True) + 1e-2 * np.eye(64)
        ref = K12 - Va.T @ Vb
        assert np.max(np.abs(cov[i:i + 64, j:j + 64] - ref)) <= 1e-9, (i, j)
    g.close()


def test_fp32_model_answers_from_the_fp64_factor(lib):
    X, y, Xs = random_problem(300, 200, seed=11)
    g64 = model(X, y, noise_var=1e-3)
    g32 = model(X, y, dtype="f32", noise_var=1e-3)
    m64, c64 = g64.predict(Xs, full_cov=True)
    m32, c32 = g32.predict(Xs, full_cov=True)
    assert np.max(np.abs(c32 - c64)) <= 1e-12
    assert np.max(np.abs(m32 - m64)) <= 1e-12
    b64 = g64.posterior_covariance_between_points(Xs[:50], Xs[60:])
    b32 = g32.posterior_covariance_between_points(Xs[:50], Xs[60:])
    assert np.max(np.abs(b32 - b64)) <= 1e-12


def test_errors_and_determinism(lib):
    X, y, Xs = random_problem(50, 100, d=2, seed=5)
    g = model(X, y, fit=False)
    mean, cov = np.empty(100), np.empty((100, 100))
    P = lib.dptr
    rc = g._lib.cbo_gp_predict_cov(g._handle, 100, P(Xs), None, None, 1, P(mean), P(cov))
    assert rc == lib.CBO_ERR_NOT_FITTED
    rc = g._lib.cbo_gp_cov_between(g._handle, 100, P(Xs), None, 100, P(Xs), None, P(cov))
    assert rc == lib.CBO_ERR_NOT_FITTED
    g.ensure_fitted()
    assert g._lib.cbo_gp_predict_cov(g._handle, 0, P(Xs), None, None, 1, P(mean), P(cov)) == lib.CBO_ERR_INVALID
    assert g._lib.cbo_gp_predict_cov(g._handle, 100, P(Xs), None, None, 1, P(mean), None) == lib.CBO_ERR_INVALID
    a = g.predict(Xs, full_cov=True)[1]
    b = g.predict(Xs, full_cov=True)[1]
    assert np.array_equal(a, b)
    assert np.array_equal(g.posterior_covariance_between_points(Xs[:30], Xs), g.posterior_covariance_between_points(Xs[:30], Xs))
    g.close()
    f = load_fixture("causal_d2")
    cm, _ = fixture_model(f)
    Xc = np.ascontiguousarray(f["Xs"][:20])
    mean, cov = np.empty(20), np.empty((20, 20))
    assert cm._lib.cbo_gp_predict_cov(cm._handle, 20, P(Xc), None, None, 1, P(mean), P(cov)) == lib.CBO_ERR_INVALID
    assert cm._lib.cbo_gp_cov_between(cm._handle, 20, P(Xc), None, 20, P(Xc), None, P(cov)) == lib.CBO_ERR_INVALID
    # the prior mean is needed only for the mean
    pv = np.ascontiguousarray(f["vXs"][:20, 0])
    assert cm._lib.cbo_gp_predict_cov(cm._handle, 20, P(Xc), None, P(pv), 1, None, P(cov)) == lib.CBO_OK
    assert np.array_equal(cov, cm.predict(Xc, full_cov=True)[1])


def test_append_is_seen_and_sweeps_are_untouched(lib):
    from cbo_with_oop_amd import CausalExpectedImprovement
    X, y, Xs = random_problem(200, 500, seed=21)
    g = model(X, y, noise_var=1e-2)
    ei = CausalExpectedImprovement(float(y.min()), "min", g)
    before = ei.evaluate(Xs)
    _, c_before = g.predict(Xs, full_cov=True)
    after = ei.evaluate(Xs)
    assert np.array_equal(before, after)
    x_new, y_new = Xs[:1].copy(), np.array([[0.3]])
    assert g.append(x_new, y_new)
    assert g.X.shape[0] == 201
    _, c_after = g.predict(Xs, full_cov=True)
    post = O.fit(np.vstack([X, x_new]), np.vstack([y, y_new]), noise_var=1e-2)
    ref = restated_cov(post, Xs, Xs, sym=True) + 1e-2 * np.eye(500)
    assert np.max(np.abs(c_after - ref)) <= 1e-9
    assert not np.array_equal(c_after, c_before)
    g.close()


def test_emukit_wrapper_methods(lib):
    X, y, Xs = random_problem(80, 120, d=2, seed=31)
    g = model(X, y, noise_var=1e-2)
    post = O.fit(X, y, noise_var=1e-2)
    m, c = g.predict_with_full_covariance(Xs)
    assert np.array_equal(c, g.predict(Xs, full_cov=True)[1])
    pc = g.predict_covariance(Xs, with_noise=False)
    assert np.array_equal(pc, np.clip(g.predict(Xs, include_likelihood=False, full_cov=True)[1], 1e-10, np.inf))
    x_new = Xs[:1]
    vr = g.calculate_variance_reduction(x_new, Xs)
    cov = restated_cov(post, x_new, Xs)
    var = O.predict(post, x_new)[1]
    expect = cov ** 2 / var
    assert vr.shape == (1, 120)
    assert np.max(np.abs(vr - expect)) <= 1e-9 * max(1.0, np.max(np.abs(expect)))
    g.close()
