"""GPU tests of max-value entropy search (cbo_gp_mes_gumbel: gumbel_quantiles_kernel; cbo_acq_sweep_mes: mes_acq_kernel of
kernels_mes.hip) against a restatement of emukit 0.4's MaxValueEntropySearch with scipy, fed the device's own predictive
mean and variance:
    _fit_gumbel:  probf(x) = 1 - exp(sum log_ndtr(-(x - fmean) / fsd)), scipy.optimize.bisect at 0.25 / 0.5 / 0.75
    evaluate:     mean_k(-gamma pdf(gamma) / (2 minus_cdf) - log(minus_cdf)), gamma = (mins - fmean) / max(fsd, 1e-10),
                  minus_cdf = clip(1 - ndtr(gamma), 1e-10, 1)."""
import ctypes
import warnings

import numpy as np
import pytest
from scipy.optimize import bisect
from scipy.special import log_ndtr
from scipy.stats import norm

from conftest import load_fixture

pytestmark = pytest.mark.gpu

INVALID, NOT_FITTED = -1, -5


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


def fixture_model(name):
    f = load_fixture(name)
    assert f["mX"] is None
    ls = f["lengthscale_arg"]
    return model(f["X"], f["y"], variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls),
                 noise_var=float(f["noise_var"])), f


def causal_model(n=40, d=2, seed=3):
    """A causal model whose mean_function / variance_adjustment are closed forms (any point can be asked)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))
    mf = lambda a: 0.3 * np.sin(a).sum(1, keepdims=True)
    va = lambda a: 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2
    return model(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-4, mean_function=mf, variance_adjustment=va)


def random_model(n=30, d=2, seed=0, dtype="f64"):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(2 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return model(X, y, dtype=dtype, variance=1.0, lengthscale=0.7, noise_var=1e-3)


def box(g):
    return [(-2.5, 2.5)] * g.input_dim


def gumbel(lib, g, grid):
    """cbo_gp_mes_gumbel on the device: (quantiles (3,), a, b, mean (m,), var (m,))."""
    m = grid.shape[0]
    pm = pv = None
    if g.causal:
        pm, pv = np.ascontiguousarray(g.mean_function(grid)[:, 0]), np.ascontiguousarray(g.variance_adjustment(grid)[:, 0])
    q, mean, var = np.empty(3), np.empty(m), np.empty(m)
    a, b = ctypes.c_double(), ctypes.c_double()
    lib.check(lib.load().cbo_gp_mes_gumbel(g._handle, m, lib.dptr(grid), lib.dptr(pm), lib.dptr(pv), lib.dptr(q),
                                           ctypes.byref(a), ctypes.byref(b), lib.dptr(mean), lib.dptr(var)))
    return q, a.value, b.value, mean, var


def gumbel_restated(fmean, fvar):
    fsd = np.sqrt(fvar)

    def probf(x):
        return 1 - np.exp(np.sum(log_ndtr(-(x - fmean) / fsd), axis=0))

    left, right = np.min(fmean - 5 * fsd), np.max(fmean + 5 * fsd)
    q = [bisect(lambda x: probf(x) - val, left, right, maxiter=10000) for val in (0.25, 0.5, 0.75)]
    return np.array(q), left, right


def mes_restated(mean, var, mins):
    """(MES (M,), per-sample terms (M,K), the per-row effect of one ulp of ndtr near 1 (M,)) from mean / var (M,).

    1 - ndtr(gamma) is formed as written: where ndtr(gamma) is within a few 1e-6 of 1, a difference of ONE ulp of 1 between
    two correct ndtr implementations (the device's shares the density's exponential) is a relative change of 1.1e-16 /
    minus_cdf in minus_cdf, and the term moves by |d term / d minus_cdf| 1.1e-16.  The restatement's own conditioning:
    it is added to the tolerance, as a bound of two such ulps."""
    fsd = np.maximum(np.sqrt(var[:, None]), 1e-10)
    gamma = (mins[None, :] - mean[:, None]) / fsd
    raw = 1 - norm.cdf(gamma)
    minus_cdf = np.clip(raw, 1e-10, 1)
    pdf = norm.pdf(gamma)
    terms = -gamma * pdf / (2 * minus_cdf) - np.log(minus_cdf)
    slope = np.abs(gamma) * pdf / (2 * minus_cdf ** 2) + 1 / minus_cdf
    ulp_effect = np.mean(np.where(raw > 1e-10, slope * 2.3e-16, 0.0), axis=1)
    return np.mean(terms, axis=1), terms, ulp_effect


def sweep_mes(lib, g, cands, mins, cost=1.0):
    """cbo_acq_sweep_mes: (acq, mean, var, best_val, best_idx)."""
    m = len(cands)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    mins = np.ascontiguousarray(mins, dtype=np.float64)
    lib.check(lib.load().cbo_acq_sweep_mes(g._handle, cands._handle, mins.size, lib.dptr(mins), float(cost),
                                           lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                           ctypes.byref(bi)))
    return acq, mean, var, bv.value, bi.value


def sweep_ei(g, cands):
    from cbo_with_oop_amd import CausalExpectedImprovement
    r = CausalExpectedImprovement(0.0, "min", g).sweep(cands, want_posterior=True)
    return r["mean"][:, 0], r["var"][:, 0]


def mins_spanning(mean, var, k, lo=-40.0, hi=40.0):
    """Samples whose gamma at candidate 0 runs from lo to hi (both clips of minus_cdf are met)."""
    return mean[0] + np.linspace(lo, hi, k) * np.sqrt(var[0])


def check_mes(acq, mean, var, mins, cost=1.0, best_val=None, best_idx=None, offset=0):
    ref, terms, ulp_effect = mes_restated(mean, var, mins)
    ref = ref / cost
    tol = 1e-12 * np.abs(ref) + 1e-15 * np.max(np.abs(terms), axis=1) / cost + ulp_effect / cost
    err = np.abs(acq - ref)
    assert np.all(err <= tol), f"worst {np.max(err / np.maximum(tol, 1e-300)):.3g} x tolerance"
    # most rows meet the bar without the conditioning term
    plain = err <= 1e-12 * np.abs(ref) + 1e-15 * np.max(np.abs(terms), axis=1) / cost
    assert np.mean(plain) >= 0.999, np.mean(plain)
    if best_idx is not None:
        assert best_val == np.max(acq) and best_idx - offset == int(np.argmax(acq))
        order = np.argsort(ref)[::-1]
        if ref.size > 1 and ref[order[0]] - ref[order[1]] > tol[order[0]] + tol[order[1]]:
            assert best_idx - offset == order[0]
    return float(np.max(err / np.maximum(np.abs(ref), 1e-300)))


# ---- the Gumbel fit ------------------------------------------------------------------------------------------------
def grid_for(g, size=5000, seed=1):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box(g)).T
    return np.ascontiguousarray(np.vstack([g.X, rng.uniform(lo, hi, (size, g.input_dim))]))


def check_gumbel(lib, g, grid):
    q, a, b, mean, var = gumbel(lib, g, grid)
    pmean, pvar = g.predict(grid)
    assert np.array_equal(mean, pmean[:, 0]) and np.array_equal(var, pvar[:, 0])
    qr, left, right = gumbel_restated(mean, var)
    assert np.all(np.abs(q - qr) <= 1e-10 * (right - left) + 4e-12), (q, qr)
    bb = (q[0] - q[2]) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    assert b == pytest.approx(bb, rel=1e-15, abs=0) and a == pytest.approx(q[1] - bb * np.log(np.log(2.0)), rel=1e-15,
                                                                           abs=1e-300)
    return q


@pytest.mark.parametrize("name", ["toy_bo_d2", "complete_bo_d3", "coral_max_d3", "graph_ard_d4", "toy_c1_Z50"])
def test_gumbel_fit_on_fixtures(lib, name):
    g, f = fixture_model(name)
    pts = np.vstack([f["X"], f["Xs"]])
    rng = np.random.default_rng(5)
    grid = np.ascontiguousarray(np.vstack([f["X"], rng.uniform(pts.min(0), pts.max(0), (5000, pts.shape[1]))]))
    check_gumbel(lib, g, grid)


def test_gumbel_fit_causal_and_large(lib):
    check_gumbel(lib, causal_model(), grid_for(causal_model()))
    check_gumbel(lib, random_model(n=300), grid_for(random_model(n=300), size=20000))


def test_gumbel_fit_is_deterministic_and_reads_only(lib):
    g = random_model()
    L0, a0 = g.posterior_state()
    grid = grid_for(g)
    q1 = gumbel(lib, g, grid)
    q2 = gumbel(lib, g, grid)
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(q1, q2))
    L1, a1 = g.posterior_state()
    assert np.array_equal(L0, L1) and np.array_equal(a0, a1)


def test_gumbel_fit_errors(lib):
    g = random_model()
    grid = grid_for(g)
    q, a, b = np.empty(3), ctypes.c_double(), ctypes.c_double()
    L = lib.load()
    assert L.cbo_gp_mes_gumbel(g._handle, 0, lib.dptr(grid), None, None, lib.dptr(q), ctypes.byref(a), ctypes.byref(b),
                               None, None) == INVALID
    assert L.cbo_gp_mes_gumbel(g._handle, 10, lib.dptr(grid), None, None, None, ctypes.byref(a), ctypes.byref(b),
                               None, None) == INVALID
    c = causal_model()
    cg = grid_for(c)
    assert L.cbo_gp_mes_gumbel(c._handle, cg.shape[0], lib.dptr(cg), None, None, lib.dptr(q), ctypes.byref(a),
                               ctypes.byref(b), None, None) == INVALID
    u = model(g.X, g.Y, variance=1.0, lengthscale=0.7, noise_var=1e-3, fit=False)
    assert L.cbo_gp_mes_gumbel(u._handle, 10, lib.dptr(grid), None, None, lib.dptr(q), ctypes.byref(a),
                               ctypes.byref(b), None, None) == NOT_FITTED
    # 2^21 points with one mean and variance: probf(left) = 1 - ndtr(5)^m > 0.25, the bracket does not change sign (scipy's
    # ValueError)
    same = np.ascontiguousarray(np.zeros((1 << 21, g.input_dim)))
    assert L.cbo_gp_mes_gumbel(g._handle, same.shape[0], lib.dptr(same), None, None, lib.dptr(q), ctypes.byref(a),
                               ctypes.byref(b), None, None) == INVALID
    assert b"different signs" in L.cbo_last_error()


# ---- the scoring sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 511, 513, 1000, (1 << 16) + 1, 2 * 2048 * 256 + 3])
def test_sweep_matches_restatement_ragged(lib, m):
    """511 and 513 are one lane short of and one past a workgroup's span (256 lanes, two candidates each); the largest
    size is past the grid-stride wrap of the 2048 workgroups with an odd tail -- there only the 3-sample case runs, so that
    the numpy restatement stays within seconds."""
    from cbo_with_oop_amd import CandidateGrid
    g = random_model()
    rng = np.random.default_rng(m)
    pts = rng.uniform(-2.5, 2.5, (m, 2))
    cands = CandidateGrid(pts, g)
    mean, var = sweep_ei(g, cands)
    for k, mins in ((10, mins_spanning(mean, var, 10)), (3, np.array([-1.5, -0.4, 0.2])),
                    (64, mins_spanning(mean, var, 64, -8.0, 8.0))):
        if m > (1 << 20) and k > 4:
            continue
        acq, mm, vv, bv, bi = sweep_mes(lib, g, cands, mins)
        assert np.array_equal(mm, mean) and np.array_equal(vv, var)
        check_mes(acq, mean, var, mins, best_val=bv, best_idx=bi)


def test_sweep_causal_fixtures_and_fp32(lib):
    from cbo_with_oop_amd import CandidateGrid
    for g in (causal_model(), fixture_model("coral_max_d3")[0], random_model(dtype="f32"), random_model(n=700)):
        rng = np.random.default_rng(9)
        pts = rng.uniform(-2.5, 2.5, (5000, g.input_dim))
        cands = CandidateGrid(pts, g)
        mean, var = sweep_ei(g, cands)
        mins = mins_spanning(mean, var, 10)
        acq, mm, vv, bv, bi = sweep_mes(lib, g, cands, mins, cost=2.5)
        assert np.array_equal(mm, mean) and np.array_equal(vv, var)
        worst = check_mes(acq, mean, var, mins, cost=2.5, best_val=bv, best_idx=bi)
        print(f"{g.dtype} causal={g.causal}: worst relative deviation {worst:.3g}")


def test_gamma_spans_both_clips(lib):
    from cbo_with_oop_amd import CandidateGrid
    g = random_model()
    pts = np.ascontiguousarray(np.vstack([g.X, np.random.default_rng(2).uniform(-2.5, 2.5, (2000, 2))]))
    cands = CandidateGrid(pts, g)
    mean, var = sweep_ei(g, cands)
    mins = mins_spanning(mean, var, 33)
    gamma = (mins[None, :] - mean[:, None]) / np.sqrt(var[:, None])
    assert gamma.min() <= -40 and gamma.max() >= 40
    assert np.any(1 - norm.cdf(gamma) < 1e-10)             # the clip of minus_cdf is met
    acq, _, _, bv, bi = sweep_mes(lib, g, cands, mins)
    check_mes(acq, mean, var, mins, best_val=bv, best_idx=bi)


def test_cached_resweep_determinism_model_untouched_and_append(lib):
    from cbo_with_oop_amd import CandidateGrid
    g = random_model()
    pts = np.random.default_rng(4).uniform(-2.5, 2.5, (3000, 2))
    cands = CandidateGrid(pts, g)
    mean, var = sweep_ei(g, cands)
    mins = mins_spanning(mean, var, 10, -3.0, 3.0)
    L0, a0 = g.posterior_state()
    first = sweep_mes(lib, g, cands, mins)
    again = sweep_mes(lib, g, cands, mins)                    # cached q, mu
    fresh = sweep_mes(lib, g, CandidateGrid(pts, g), mins)
    for r in (again, fresh):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(first, r))
    L1, a1 = g.posterior_state()
    assert np.array_equal(L0, L1) and np.array_equal(a0, a1)
    assert g.append(np.array([[0.3, -0.2]]), 0.7)
    after = sweep_mes(lib, g, cands, mins)
    m2, v2 = sweep_ei(g, CandidateGrid(pts, g))
    assert not np.array_equal(after[1], first[1])
    assert np.array_equal(after[1], m2) and np.array_equal(after[2], v2)
    check_mes(after[0], m2, v2, mins)


def test_ties_offset_and_cost(lib):
    from cbo_with_oop_amd import CandidateGrid
    g = random_model()
    pts = np.repeat(np.array([[0.5, 0.5], [1.0, -1.0], [-2.0, 2.0]]), 40, axis=0)
    mins = np.array([-2.0, -1.0, 0.0])
    a1, mean, var, bv, bi = sweep_mes(lib, g, CandidateGrid(pts, g, index_offset=1000), mins)
    top = int(np.argmax(a1))
    assert top % 40 == 0 and bi == 1000 + top and bv == a1[top]
    a3 = sweep_mes(lib, g, CandidateGrid(pts, g), mins, cost=3.0)[0]
    assert np.array_equal(a3, a1 / 3.0)


def test_sweep_errors(lib):
    from cbo_with_oop_amd import CandidateGrid
    L = lib.load()
    g = random_model()
    cands = CandidateGrid(np.zeros((5, 2)), g)
    good = np.array([0.1, 0.2])

    def call(gp, c, k, mins, cost):
        return L.cbo_acq_sweep_mes(gp._handle, c._handle, k, None if mins is None else lib.dptr(mins), cost,
                                   None, None, None, None, None)

    assert call(g, cands, 2, good, 1.0) == 0
    assert call(g, cands, 0, good, 1.0) == INVALID
    assert call(g, cands, 65, np.zeros(65), 1.0) == INVALID
    assert call(g, cands, 64, np.zeros(64), 1.0) == 0
    assert call(g, cands, 2, None, 1.0) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        assert call(g, cands, 2, np.array([0.1, bad]), 1.0) == INVALID
    for cost in (0.0, -1.0, float("nan")):
        assert call(g, cands, 2, good, cost) == INVALID
    c = causal_model()
    assert call(c, CandidateGrid(np.zeros((5, 2))), 2, good, 1.0) == INVALID     # candidates without prior
    u = model(g.X, g.Y, variance=1.0, lengthscale=0.7, noise_var=1e-3, fit=False)
    u_cands = CandidateGrid(np.zeros((5, 2)), u)
    assert L.cbo_acq_sweep_mes(u._handle, u_cands._handle, 2, lib.dptr(good), 1.0, None, None, None, None,
                               None) == NOT_FITTED


def test_full_size_grid_sampled_rows(lib):
    from cbo_with_oop_amd import CandidateGrid
    g = random_model(d=1)
    m = 1 << 24
    pts = np.linspace(-2.5, 2.5, m)[:, None]
    cands = CandidateGrid(pts, g)
    mean, var = sweep_ei(g, cands)
    mins = mins_spanning(mean, var, 10, -6.0, 6.0)
    acq, mm, vv, bv, bi = sweep_mes(lib, g, cands, mins)
    rows = np.unique(np.concatenate([np.random.default_rng(0).integers(0, m, 200000), [0, m - 1, int(np.argmax(acq))]]))
    assert np.array_equal(mm[rows], mean[rows]) and np.array_equal(vv[rows], var[rows])
    check_mes(acq[rows], mean[rows], var[rows], mins)
    assert bv == np.max(acq) and bi == int(np.argmax(acq))


# ---- through the public interface ----------------------------------------------------------------------------------
def test_class_and_grid_optimiser(lib):
    from cbo_with_oop_amd import Cost, MaxValueEntropySearch
    from cbo_with_oop_amd.utils_functions import CausalGradientAcquisitionOptimizer
    g = random_model()
    bounds = box(g)
    np.random.seed(21)
    mes = MaxValueEntropySearch(g, bounds, num_samples=12)
    x = np.random.default_rng(1).uniform(-2.5, 2.5, (500, 2))
    v = mes.evaluate(x)
    # the restatement of update_parameters on the device's quantiles and evaluate on the device's mean and variance
    np.random.seed(21)
    grid = np.vstack([g.X, np.hstack([np.random.uniform(lo, hi, (5000, 1)) for lo, hi in bounds])])
    q, a, b, gm, gv = gumbel(lib, g, np.ascontiguousarray(grid))
    assert mes.gumbel == (q[0], q[1], q[2], a, b)
    u = np.random.rand(12)
    assert np.array_equal(mes.mins, np.log(-np.log(1 - u)) * b + a)
    mean, var = g.predict(x)
    check_mes(v[:, 0], mean[:, 0], var[:, 0], mes.mins)
    # MES / Cost through the grid optimiser
    cost = Cost({"a": lambda z: 2.0}, ["a"])
    opt = CausalGradientAcquisitionOptimizer(bounds, grid_shape=[40, 40])
    xb, fb = opt.optimize(mes / cost)
    pts = opt.candidates()
    vals = mes.evaluate(pts)[:, 0] / 2.0
    assert np.array_equal(xb[0], pts[int(np.argmax(vals))]) and fb[0, 0] == np.max(vals)


def test_find_next_y_point_mes_and_default_draws(lib):
    from cbo_with_oop_amd import MaxValueEntropySearch, find_next_y_point
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    g = random_model()
    bounds = box(g)
    costs = {"a": lambda z: 1.5}
    np.random.seed(8)
    y, x = find_next_y_point(bounds, g, 0.0, ["a"], costs, grid_shape=[30, 30], acquisition="MES")
    np.random.seed(8)
    mes = MaxValueEntropySearch(g, bounds)
    pts = meshgrid_candidates(bounds, [30, 30])
    vals = mes.evaluate(pts)[:, 0] / 1.5
    assert np.array_equal(x[0], pts[int(np.argmax(vals))]) and y[0, 0] == np.max(vals)
    # the default (EI) path draws nothing from numpy's global stream
    np.random.seed(8)
    find_next_y_point(bounds, g, 0.0, ["a"], costs, grid_shape=[30, 30])
    after = np.random.rand()
    np.random.seed(8)
    assert after == np.random.rand()
