"""GPU tests of the joint posterior samples (cbo_gp_posterior_samples, kernels_joint.hip): with the identity as normals
the samples minus the mean are the device's factor L of Sigma + jitter I, checked against the numpy restatement of
GPy's full_cov branch (tests/test_covariance_gpu.py); with random normals they are mean + L Z^T."""
import ctypes

import numpy as np
import pytest

from conftest import load_fixture
from oracle import gp_oracle as O
from test_covariance_gpu import fixture_model, model, oracle_post, random_problem, restated_cov

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def device_factor(g, Xs):
    """(L, mean, jitter): the samples for normals = I are mean + L."""
    M = Xs.shape[0]
    s = g.posterior_samples_f(Xs, M, normals=np.eye(M))[:, 0, :]
    mean = g.predict(Xs)[0][:, 0]
    return s - mean[:, None], mean, g.last_sample_jitter


def check_factor(L, sigma, jitter, bound):
    M = L.shape[0]
    assert np.all(L[np.triu_indices(M, 1)] == 0.0)
    assert np.all(np.diag(L) > 0.0)
    err = np.max(np.abs(L @ L.T - (sigma + jitter * np.eye(M))))
    assert err <= bound, (err, bound)


def check_product(samples, mean, L, Z):
    """samples = mean + L Z^T up to GEMM rounding (L itself carries the rounding of mean + L - mean)."""
    ref = mean[:, None] + L @ Z.T
    scale = np.tril(np.abs(L) + np.abs(mean)[:, None]) @ np.abs(Z).T
    bound = 1e-13 * scale + 1e-15 * np.abs(mean)[:, None] + 1e-300
    assert np.all(np.abs(samples - ref) <= bound), np.max(np.abs(samples - ref) / bound)


@pytest.mark.parametrize("name", ["toy_bo_d2", "complete_bo_d3", "graph_ard_d4", "coral_max_d3", "causal_d2",
                                  "jitter_ladder"])
def test_factor_is_the_cholesky_factor_of_sigma(lib, name):
    f = load_fixture(name)
    g, _ = fixture_model(f)
    post = oracle_post(f)
    Xs, sig2 = f["Xs"], float(f["variance"])
    L, mean, (tries, jitter) = device_factor(g, Xs)
    # Sigma is the noise-free full covariance, the causal diagonal quirk included
    sigma = restated_cov(post, Xs, Xs, f["vXs"], f["vXs"], sym=True)
    bound = 1e-9 * sig2
    if name == "jitter_ladder":
        bound += 8.0 * np.max(np.abs(f["var"] - f["var_truth"]))      # the oracle's own error (test_covariance_gpu.py)
    assert (tries == 0) == (jitter == 0.0)
    check_factor(L, sigma, jitter, bound)
    # the mean under normals = 0 is predict's, bit for bit, in every column
    s0 = g.posterior_samples_f(Xs, 3, normals=np.zeros((3, Xs.shape[0])))[:, 0, :]
    assert np.array_equal(s0, np.repeat(mean[:, None], 3, axis=1))


@pytest.mark.parametrize("M", [1, 17, 130, 1000])
def test_product_at_ragged_sizes(lib, M):
    X, y, Xs = random_problem(300, M, seed=M)
    g = model(X, y, noise_var=1e-2)
    L, mean, _ = device_factor(g, Xs)
    for size in (1, 17, 130):
        Z = np.random.default_rng(size + M).standard_normal((size, M))
        s = g.posterior_samples_f(Xs, size, normals=Z)
        assert s.shape == (M, 1, size)
        check_product(s[:, 0, :], mean, L, Z)
    g.close()


def test_product_at_4096_points(lib):
    X, y, Xs = random_problem(1024, 4096, seed=4)
    g = model(X, y, noise_var=1e-2)
    L, mean, _ = device_factor(g, Xs)
    Z = np.random.default_rng(5).standard_normal((1024, 4096))
    s = g.posterior_samples_f(Xs, 1024, normals=Z)[:, 0, :]
    check_product(s, mean, L, Z)
    g.close()


def test_sample_statistics(lib):
    X, y, Xs = random_problem(40, 32, d=2, seed=8)
    g = model(X, y, noise_var=1e-2)
    post = O.fit(X, y, noise_var=1e-2)
    np.random.seed(17)
    s = g.posterior_samples_f(Xs, 20000)[:, 0, :]
    N = s.shape[1]
    mean = O.predict(post, Xs)[0][:, 0]
    sigma = restated_cov(post, Xs, Xs, sym=True) + g.last_sample_jitter[1] * np.eye(32)
    sd = np.sqrt(np.diag(sigma))
    assert np.all(np.abs(s.mean(1) - mean) <= 5.0 * sd / np.sqrt(N) + 1e-12)
    S = np.cov(s)
    tol = 6.0 * np.sqrt((np.outer(sd ** 2, sd ** 2) + sigma ** 2) / N) + 1e-12
    assert np.all(np.abs(S - sigma) <= tol)
    # a seeded run is deterministic, and leaves the stream where multivariate_normal would
    after = np.random.rand()
    np.random.seed(17)
    s2 = g.posterior_samples_f(Xs, 20000)[:, 0, :]
    assert np.array_equal(s, s2)
    assert np.random.rand() == after
    g.close()


def test_ladder_on_training_points_and_duplicates(lib):
    # a noise-free model on well-separated points: its posterior is ~0 at the training points
    g1, g2 = np.meshgrid(np.arange(4) * 1.5, np.arange(3) * 1.5)
    X = np.column_stack([g1.ravel(), g2.ravel()])
    y = np.sin(X).sum(1, keepdims=True)
    g = model(X, y)
    post = O.fit(X, y, noise_var=g.noise_var)
    for Xs in (X.copy(), np.vstack([X, X[:5], X[:5]]), np.vstack([X[:1]] * 6)):
        L, mean, (tries, jitter) = device_factor(g, Xs)
        assert np.all(np.isfinite(L))
        assert (tries == 0) == (jitter == 0.0)
        if tries:
            assert np.isclose(jitter, 1e-6 * g.variance * 10.0 ** (tries - 1), rtol=1e-12)
        check_factor(L, restated_cov(post, Xs, Xs, sym=True), jitter, 1e-9 * g.variance)
    g.close()


def test_fp32_model_samples_are_the_fp64_models(lib):
    X, y, Xs = random_problem(300, 200, seed=11)
    g64 = model(X, y, noise_var=1e-3)
    g32 = model(X, y, dtype="f32", noise_var=1e-3)
    Z = np.random.default_rng(2).standard_normal((50, 200))
    assert np.array_equal(g32.posterior_samples_f(Xs, 50, normals=Z), g64.posterior_samples_f(Xs, 50, normals=Z))


def test_samples_leave_the_model_alone_and_follow_it(lib):
    from cbo_with_oop_amd import CausalExpectedImprovement
    X, y, Xs = random_problem(200, 300, seed=21)
    g = model(X, y, noise_var=1e-2)
    ei = CausalExpectedImprovement(float(y.min()), "min", g)
    before = ei.evaluate(Xs)
    Z = np.random.default_rng(0).standard_normal((64, 300))
    s_before = g.posterior_samples_f(Xs, 64, normals=Z)
    assert np.array_equal(before, ei.evaluate(Xs))
    assert np.array_equal(s_before, g.posterior_samples_f(Xs, 64, normals=Z))
    x_new, y_new = Xs[:1].copy(), np.array([[0.3]])
    assert g.append(x_new, y_new)
    post = O.fit(np.vstack([X, x_new]), np.vstack([y, y_new]), noise_var=1e-2)
    L, _, (_, jitter) = device_factor(g, Xs)
    check_factor(L, restated_cov(post, Xs, Xs, sym=True), jitter, 1e-9)
    assert not np.array_equal(s_before, g.posterior_samples_f(Xs, 64, normals=Z))
    X2, y2 = X[:150], y[:150]
    g.set_data(X2, y2)
    post = O.fit(X2, y2, noise_var=1e-2)
    L, _, (_, jitter) = device_factor(g, Xs)
    check_factor(L, restated_cov(post, Xs, Xs, sym=True), jitter, 1e-9)
    g.close()


def test_likelihood_samples_add_the_noise(lib):
    X, y, Xs = random_problem(60, 40, d=2, seed=3)
    g = model(X, y, noise_var=0.04)
    np.random.seed(5)
    ys = g.posterior_samples(Xs, 7)
    after = np.random.rand()
    np.random.seed(5)
    fs = g.posterior_samples_f(Xs, 7)
    expect = np.array([np.random.normal(v, 0.2, size=1) for v in fs[:, 0, :].flatten()]).reshape(40, 7)
    assert ys.shape == (40, 1, 7)
    assert np.array_equal(ys[:, 0, :], expect)
    assert np.random.rand() == after
    g.close()


def test_errors(lib):
    X, y, Xs = random_problem(50, 100, d=2, seed=5)
    g = model(X, y, fit=False)
    P = lib.dptr
    Z, out = np.zeros((4, 100)), np.empty((100, 4))
    call = g._lib.cbo_gp_posterior_samples
    assert call(g._handle, 100, P(Xs), None, None, 4, P(Z), P(out), None, None) == lib.CBO_ERR_NOT_FITTED
    g.ensure_fitted()
    assert call(g._handle, 100, P(Xs), None, None, 4, P(Z), P(out), None, None) == lib.CBO_OK
    assert call(g._handle, 100, P(Xs), None, None, 4, None, P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(g._handle, 100, P(Xs), None, None, 4, P(Z), None, None, None) == lib.CBO_ERR_INVALID
    assert call(g._handle, 100, None, None, None, 4, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(None, 100, P(Xs), None, None, 4, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(g._handle, 0, P(Xs), None, None, 4, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(g._handle, 100, P(Xs), None, None, 0, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(g._handle, 100, P(Xs), None, None, -1, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    g.close()
    f = load_fixture("causal_d2")
    cm, _ = fixture_model(f)
    Xc = np.ascontiguousarray(f["Xs"][:20])
    pm, pv = np.ascontiguousarray(f["mXs"][:20, 0]), np.ascontiguousarray(f["vXs"][:20, 0])
    Z, out = np.zeros((3, 20)), np.empty((20, 3))
    tries, jitter = ctypes.c_int(-1), ctypes.c_double(-1.0)
    call = cm._lib.cbo_gp_posterior_samples
    assert call(cm._handle, 20, P(Xc), None, P(pv), 3, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(cm._handle, 20, P(Xc), P(pm), None, 3, P(Z), P(out), None, None) == lib.CBO_ERR_INVALID
    assert call(cm._handle, 20, P(Xc), P(pm), P(pv), 3, P(Z), P(out), ctypes.byref(tries), ctypes.byref(jitter)) == lib.CBO_OK
    assert tries.value >= 0 and jitter.value >= 0.0
    assert np.array_equal(out, np.repeat(cm.predict(Xc)[0], 3, axis=1))
