"""GPU tests of the integrated variance reduction (cbo_gp_integrated_variance_reduction: ivr_tile_kernel of
kernels_joint.hip and its closing launch) against emukit's own composition,
    IVR(x_i) = np.mean(model.calculate_variance_reduction(x_i, X_mc)) = mean_j C(x_i, x_j)^2 / var(x_i),
on the device's calculate_variance_reduction, and against a numpy restatement with scipy's Cholesky
(C = K(Xc, X_mc) - (L^-1 K(X, Xc))^T L^-1 K(X, X_mc), var = GPy's predictive variance with the noise)."""
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
    return model(f["X"], f["y"], **kw)


def box(*point_sets):
    pts = np.vstack(point_sets)
    return list(zip(pts.min(0), pts.max(0)))


def ivr(g, Xc, Xint, cost=1.0):
    from cbo_with_oop_amd import IntegratedVarianceReduction
    a = IntegratedVarianceReduction(g, box(Xc, Xint), x_monte_carlo=Xint)
    return a.sweep(Xc, cost=cost, want_acq=True)


def composed(g, Xc, Xint):
    """emukit's evaluate loop: one calculate_variance_reduction per candidate."""
    return np.array([[np.mean(g.calculate_variance_reduction(Xc[[i]], Xint))] for i in range(Xc.shape[0])])


def restated(post, Xc, Xint, vc=None, vi=None, tol=1e-9):
    """numpy / scipy: (IVR (M,1), the bound on |device - restatement| from the cross covariance's tolerance tol * sigma^2
    (tests/test_covariance_gpu.py) and the same absolute tolerance on the predictive variance)."""
    causal = post.vX is not None
    ls, var = post.lengthscale, post.variance
    K12 = O.causal_K(Xc, Xint, vc if causal else None, vi if causal else None, var, ls)
    V1 = scipy.linalg.solve_triangular(post.L, O.causal_K(post.X, Xc, post.vX, vc, var, ls), lower=True)
    V2 = scipy.linalg.solve_triangular(post.L, O.causal_K(post.X, Xint, post.vX, vi, var, ls), lower=True)
    C = K12 - V1.T @ V2
    v = O.predict(post, Xc, None, vc)[1]
    ref = np.mean(C ** 2, 1, keepdims=True) / v
    tc = tol * var
    bound = (2.0 * np.mean(np.abs(C), 1, keepdims=True) * tc + tc * tc) / v + ref * (tc / v) + 1e-13 * np.max(ref)
    return ref, bound


def random_problem(n, m, p, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return X, y, rng.uniform(-2.0, 2.0, (m, d)), rng.uniform(-2.0, 2.0, (p, d))


def raw_call(g, Xc, Xint, pv=None, pvi=None, cost=1.0, want=(True, True, True), m=None, p=None):
    from cbo_with_oop_amd import _lib
    m = Xc.shape[0] if m is None else m
    p = Xint.shape[0] if p is None else p
    out = np.empty(max(m, 1))
    bv, bi = ctypes.c_double(0.0), ctypes.c_int64(-1)
    rc = g._lib.cbo_gp_integrated_variance_reduction(
        g._handle, m, _lib.dptr(Xc), _lib.dptr(pv), p, _lib.dptr(Xint), _lib.dptr(pvi), float(cost),
        _lib.dptr(out) if want[0] else None, ctypes.byref(bv) if want[1] else None, ctypes.byref(bi) if want[2] else None)
    return rc, out[:m], bv.value, bi.value


@pytest.mark.parametrize("name", ["complete_bo_d3", "graph_ard_d4", "causal_d2"])
def test_composition_on_golden_fixtures(lib, name):
    f = load_fixture(name)
    g = fixture_model(f)
    Xs = np.ascontiguousarray(f["Xs"])
    Xc, Xint = Xs[:130], Xs[20:]
    vc = f["vXs"][:130] if f["vXs"] is not None else None
    vi = f["vXs"][20:] if f["vXs"] is not None else None
    res = ivr(g, Xc, Xint)
    got = res["acq"]
    assert got.shape == (130, 1) and res["mean"] is None and res["var"] is None
    comp = composed(g, Xc, Xint)
    assert np.max(np.abs(got - comp)) <= 1e-12 * np.max(np.abs(comp)), name
    ref, bound = restated(O.fit(f["X"], f["y"], f["mX"], f["vX"], float(f["variance"]), f["lengthscale_arg"],
                                float(f["noise_var"])), Xc, Xint, vc, vi)
    assert np.all(np.abs(got - ref) <= bound), (name, np.max(np.abs(got - ref) / bound))
    assert res["best_idx"] == int(np.argmax(got[:, 0])) and res["best_val"] == got[res["best_idx"], 0]
    g.close()


@pytest.mark.parametrize("n", [1, 50, 129, 1000])
def test_ragged_sizes(lib, n):
    X, y, Xc_all, Xi_all = random_problem(n, 300, 300, seed=n)
    g = model(X, y, noise_var=1e-2)
    post = O.fit(X, y, noise_var=1e-2)
    for m in (1, 127, 129, 300):
        for p in (1, 127, 129, 300):
            Xc, Xint = Xc_all[:m], Xi_all[:p]
            got = ivr(g, Xc, Xint)["acq"]
            ref, bound = restated(post, Xc, Xint)
            assert np.all(np.abs(got - ref) <= bound), (n, m, p)
    g.close()


def test_chunked_integration_set_gives_the_same_bits(lib, monkeypatch):
    from cbo_with_oop_amd import _lib
    n, m, p = 50, 129, 3000
    X, y, Xc, Xint = random_problem(n, m, p, seed=3)
    g = model(X, y, noise_var=1e-2)
    one = ivr(g, Xc, Xint)
    # 1 MiB of workspace over n_pad = 128 rows: 1024 columns, 256 of them the candidates' (up to a tile boundary), so
    # 768 integration points per chunk and four chunks
    cols = (1 << 20) // (8 * 128) // 64 * 64
    per_chunk = (cols - 256) // 128 * 128
    assert -(-p // per_chunk) >= 3
    monkeypatch.setenv("CBO_HIP_WORKSPACE_MB", "1")
    ctx = _lib.Context(0)
    g2 = model(X, y, noise_var=1e-2, context=ctx)
    many = ivr(g2, Xc, Xint)
    assert np.array_equal(one["acq"], many["acq"])
    assert one["best_idx"] == many["best_idx"] and one["best_val"] == many["best_val"]
    # the candidates' solution (with one tile) must fit: 1000 candidates take 1024 columns
    Xbig = np.ascontiguousarray(np.vstack([Xc] * 8)[:1000])
    assert raw_call(g2, Xbig, Xint)[0] == lib.CBO_ERR_INVALID
    g2.close()
    ctx.close()
    g.close()


def test_determinism_argmax_cost_and_optimizer(lib):
    from cbo_with_oop_amd import Cost
    from cbo_with_oop_amd.utils_functions import CausalGradientAcquisitionOptimizer, IntegratedVarianceReduction
    X, y, Xc, Xint = random_problem(200, 1000, 2000, d=2, seed=9)
    g = model(X, y, noise_var=1e-2)
    rc, a1, bv1, bi1 = raw_call(g, Xc, Xint)
    rc2, a2, bv2, bi2 = raw_call(g, Xc, Xint)
    assert rc == rc2 == lib.CBO_OK
    assert np.array_equal(a1, a2) and bv1 == bv2 and bi1 == bi2
    assert bi1 == int(np.argmax(a1)) and bv1 == a1[bi1]
    # ties: the lowest index wins
    Xt = np.ascontiguousarray(np.vstack([Xc[bi1:bi1 + 1], Xc[:5], Xc[bi1:bi1 + 1]]))
    assert raw_call(g, Xt, Xint)[3] == 0
    # the cost divides the result; each output may be asked for alone
    rc, a3, bv3, bi3 = raw_call(g, Xc, Xint, cost=3.0)
    assert np.array_equal(a3, a1 / 3.0) and bi3 == bi1
    assert raw_call(g, Xc, Xint, want=(False, True, False))[2] == bv1
    assert raw_call(g, Xc, Xint, want=(False, False, True))[3] == bi1
    # the grid optimiser returns the best grid point, alone and over a Cost
    bounds = [(-2.0, 2.0), (-2.0, 2.0)]
    acq = IntegratedVarianceReduction(g, bounds, x_monte_carlo=Xint)
    opt = CausalGradientAcquisitionOptimizer(bounds, grid_shape=[40, 40])
    grid = opt.candidates()
    vals = acq.evaluate(grid)[:, 0]
    x, fx = opt.optimize(acq)
    assert np.array_equal(x[0], grid[int(np.argmax(vals))]) and fx[0, 0] == vals.max()
    cost = Cost({"a": lambda v: 2.0, "b": lambda v: 0.5}, ["a", "b"])
    xq, fq = opt.optimize(acq / cost)
    assert np.array_equal(xq, x) and fq[0, 0] == vals.max() / 2.5
    with pytest.raises(ValueError, match="gradients"):
        opt.optimize(acq, refine=True)
    g.close()


def test_model_is_untouched_and_append_is_seen(lib):
    from cbo_with_oop_amd import CausalExpectedImprovement
    X, y, Xc, Xint = random_problem(300, 400, 900, seed=21)
    g = model(X, y, noise_var=1e-2)
    ei = CausalExpectedImprovement(float(y.min()), "min", g)
    grid_before = ei.sweep(Xc, want_acq=True, want_posterior=True)
    L0, a0 = g.posterior_state()
    before = ivr(g, Xc, Xint)["acq"]
    grid_after = ei.sweep(Xc, want_acq=True, want_posterior=True)
    L1, a1 = g.posterior_state()
    for key in ("acq", "mean", "var"):
        assert np.array_equal(grid_before[key], grid_after[key]), key
    assert np.array_equal(L0, L1) and np.array_equal(a0, a1)
    x_new, y_new = Xc[:1].copy(), np.array([[0.3]])
    assert g.append(x_new, y_new)
    after = ivr(g, Xc, Xint)["acq"]
    assert not np.array_equal(after, before)
    ref, bound = restated(O.fit(np.vstack([X, x_new]), np.vstack([y, y_new]), noise_var=1e-2), Xc, Xint)
    assert np.all(np.abs(after - ref) <= bound)
    g.close()


def test_fp32_model_gives_the_fp64_bits(lib):
    X, y, Xc, Xint = random_problem(300, 200, 700, seed=11)
    g64 = model(X, y, noise_var=1e-3)
    g32 = model(X, y, dtype="f32", noise_var=1e-3)
    r64, r32 = ivr(g64, Xc, Xint), ivr(g32, Xc, Xint)
    assert np.array_equal(r64["acq"], r32["acq"]) and r64["best_idx"] == r32["best_idx"]
    g64.close()
    g32.close()


def test_error_codes(lib):
    X, y, Xc, Xint = random_problem(50, 100, 200, d=2, seed=5)
    g = model(X, y, fit=False)
    assert raw_call(g, Xc, Xint)[0] == lib.CBO_ERR_NOT_FITTED
    g.ensure_fitted()
    assert raw_call(g, Xc, Xint)[0] == lib.CBO_OK
    assert raw_call(g, Xc, Xint, want=(False, False, False))[0] == lib.CBO_ERR_INVALID
    assert raw_call(g, Xc, Xint, m=0)[0] == lib.CBO_ERR_INVALID
    assert raw_call(g, Xc, Xint, p=0)[0] == lib.CBO_ERR_INVALID
    for cost in (0.0, -1.0, float("nan")):
        assert raw_call(g, Xc, Xint, cost=cost)[0] == lib.CBO_ERR_INVALID
    out = np.empty(100)
    P = lib.dptr
    assert g._lib.cbo_gp_integrated_variance_reduction(g._handle, 100, None, None, 200, P(Xint), None, 1.0, P(out),
                                                       None, None) == lib.CBO_ERR_INVALID
    assert g._lib.cbo_gp_integrated_variance_reduction(g._handle, 100, P(Xc), None, 200, None, None, 1.0, P(out),
                                                       None, None) == lib.CBO_ERR_INVALID
    assert g._lib.cbo_gp_integrated_variance_reduction(None, 100, P(Xc), None, 200, P(Xint), None, 1.0, P(out),
                                                       None, None) == lib.CBO_ERR_INVALID
    g.close()
    f = load_fixture("causal_d2")
    cm = fixture_model(f)
    Xs = np.ascontiguousarray(f["Xs"])
    pv = np.ascontiguousarray(f["vXs"][:, 0])
    assert raw_call(cm, Xs[:20], Xs, None, pv)[0] == lib.CBO_ERR_INVALID
    assert raw_call(cm, Xs[:20], Xs, pv[:20], None)[0] == lib.CBO_ERR_INVALID
    rc, out, _, _ = raw_call(cm, Xs[:20], Xs, pv[:20], pv)
    assert rc == lib.CBO_OK and np.array_equal(out[:, None], ivr(cm, Xs[:20], Xs)["acq"])
    cm.close()


def test_failed_workspace_allocation_is_a_hip_error(lib, monkeypatch):
    """An integration set whose one-chunk solution is larger than the device's memory, with the workspace cap lifted:
    the allocation fails and the call returns CBO_ERR_HIP (the context stays usable)."""
    from cbo_with_oop_amd import _lib
    monkeypatch.setenv("CBO_HIP_WORKSPACE_MB", str(1 << 30))
    ctx = _lib.Context(0)
    X, y, Xc, _ = random_problem(4096, 64, 1, d=1, seed=13)
    g = model(X, y, noise_var=1e-2, context=ctx)
    # 4096 rows x 2^24 columns x 8 B = 512 GiB of workspace
    Xint = np.zeros((1 << 24, 1))
    assert raw_call(g, Xc, Xint)[0] == lib.CBO_ERR_HIP
    Xsmall = np.ascontiguousarray(Xint[:500])
    rc, out, _, _ = raw_call(g, Xc, Xsmall)
    assert rc == lib.CBO_OK and np.all(np.isfinite(out))
    g.close()
    ctx.close()


def test_failed_output_allocation_leaves_the_context_usable(lib):
    """cbo_gp_predict_cov with an m x m output larger than the device's memory (2^18 points at n = 4096: 512 GiB) returns
    CBO_ERR_HIP before it writes the caller's buffers, and the next call on the same context succeeds."""
    from cbo_with_oop_amd import _lib
    ctx = _lib.Context(0)
    X, y, Xc, _ = random_problem(4096, 64, 1, d=1, seed=13)
    g = model(X, y, noise_var=1e-2, context=ctx)
    P = _lib.dptr
    big, cov = np.zeros((1 << 18, 1)), np.empty(1)
    assert g._lib.cbo_gp_predict_cov(g._handle, 1 << 18, P(big), None, None, 1, None, P(cov)) == lib.CBO_ERR_HIP
    mean, cov = np.empty(64), np.empty((64, 64))
    assert g._lib.cbo_gp_predict_cov(g._handle, 64, P(Xc), None, None, 1, P(mean), P(cov)) == lib.CBO_OK
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T)
    g.close()
    ctx.close()


def test_full_size_on_sampled_candidates(lib):
    n, m, p = 4096, 8192, 16384
    X, y, Xc, Xint = random_problem(n, m, p, seed=7)
    g = model(X, y, noise_var=1e-2)
    res = ivr(g, Xc, Xint)
    got = res["acq"][:, 0]
    assert np.all(np.isfinite(got)) and res["best_idx"] == int(np.argmax(got))
    rng = np.random.default_rng(1)
    rows = np.concatenate([[0, 127, 128, m - 1, res["best_idx"]], rng.integers(0, m, 5)])
    comp = composed(g, Xc[rows], Xint)[:, 0]
    assert np.max(np.abs(got[rows] - comp)) <= 1e-12 * np.max(np.abs(comp))
    g.close()
