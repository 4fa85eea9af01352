"""GPU tests of the point-wise acquisitions (cbo_acq_sweep_kind: pointwise_acq_kernel and plugin_incumbent_kernel of
kernels_pointwise.hip; cbo_gp_plugin_incumbent) and of their Python layer.

What is compared with what, and why each comparison is exact:
  * mean_out / var_out are cbo_acq_sweep's bits (the same posterior_of on the same q, mu), hence cbo_gp_predict's.
  * VAR at cost 1 is var_out itself.
  * PI at cost 1 is the pof_out of cbo_acq_sweep_constrained without an objective: the same device function on the same
    mean and variance.
  * MPEI is cbo_acq_sweep with the incumbent cbo_gp_plugin_incumbent returns, which is np.min / np.max of
    cbo_gp_predict's means at the model's own inputs.
  * LCB against numpy on the device's own mean_out and var_out: -(mean - beta * sqrt(var)), or mean + beta * sqrt(var).
    The kernel takes the compiler's IEEE square root (__dsqrt_rn: correctly rounded, as np.sqrt is), then one IEEE
    multiplication and one IEEE subtraction or addition with contraction off (no FMA is formed); the negation is exact.  Both
    sides are the same chain of correctly rounded operations on the same inputs, so EQUALITY is asserted, no tolerance.
  * the quotient by a cost of 3 is numpy's IEEE division: the kernel's reciprocal-plus-remainder form is the correctly
    rounded quotient for a cost whose significand is not all ones (cbo_device.h, acquisition_of); only the sign of a zero
    may differ, which assert_array_equal does not tell apart.
"""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

INVALID, NOT_FITTED = -1, -5
LCB, PI, VAR, MPEI = 1, 2, 3, 4
LE, GE = 0, 1
SIZES = [1, 7, 511, 513, 1000, 2 * 2048 * 256 + 3]


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


def causal_data(n=40, d=2, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    return X, np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))


def causal_model(n=40, d=2, seed=3, nan_at=None, **kw):
    """A causal model whose mean_function / variance_adjustment are closed forms.  nan_at: a point whose prior mean is NaN."""
    X, y = causal_data(n, d, seed)

    def mf(a):
        out = 0.3 * np.sin(a).sum(1, keepdims=True)
        if nan_at is not None:
            out[np.all(a == nan_at[None, :], axis=1)] = np.nan
        return out

    va = lambda a: 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2
    return model(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-4, mean_function=mf, variance_adjustment=va, **kw)


def random_model(n=30, d=2, seed=0, dtype="f64", **kw):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(2 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return model(X, y, dtype=dtype, variance=1.0, lengthscale=0.7, noise_var=1e-3, **kw)


def fixture_model(name):
    f = load_fixture(name)
    assert f["mX"] is None
    ls = f["lengthscale_arg"]
    return model(f["X"], f["y"], variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls),
                 noise_var=float(f["noise_var"])), f


def points(m, d=2, seed=1):
    return np.random.default_rng(seed).uniform(-2.5, 2.5, (m, d))


def grid_for(g, pts, **kw):
    from cbo_with_oop_amd import CandidateGrid
    return CandidateGrid(pts, g, **kw)


def kind_sweep(lib, g, grid, kind, y_best=0.0, task="min", param=0.0, cost=1.0, want=True):
    """cbo_acq_sweep_kind: (rc, acq, mean, var, best_val, best_idx)."""
    m = len(grid) if grid is not None else 1
    acq, mean, var = (np.empty(m) for _ in range(3)) if want else (None, None, None)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    task = lib.TASK_CODE.get(task, task)
    rc = lib.load().cbo_acq_sweep_kind(g._handle if g is not None else None, grid._handle if grid is not None else None,
                                       int(kind), float(y_best), int(task), float(param), float(cost), lib.dptr(acq),
                                       lib.dptr(mean), lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi))
    return rc, acq, mean, var, bv.value, bi.value


def plain_sweep(lib, g, grid, y_best, task, jitter, cost):
    """cbo_acq_sweep: (acq, mean, var, best_val, best_idx)."""
    m = len(grid)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                       float(cost), lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                       ctypes.byref(bi)))
    return acq, mean, var, bv.value, bi.value


def feasibility(lib, g, grid, value, jitter, sense):
    """pof_out of cbo_acq_sweep_constrained(NULL, NULL, ..., n_con = 1, ...)."""
    pof = np.empty((1, len(grid)))
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    one = lambda h: (ctypes.c_void_p * 1)(h)      # noqa: E731
    val, jit, sen = np.array([float(value)]), np.array([float(jitter)]), (ctypes.c_int * 1)(sense)
    lib.check(lib.load().cbo_acq_sweep_constrained(None, None, 0.0, 0, 0.0, 1.0, 1, one(g._handle), one(grid._handle),
                                                   lib.dptr(val), lib.dptr(jit), sen, None, None, lib.dptr(pof),
                                                   ctypes.byref(bv), ctypes.byref(bi)))
    return pof[0]


def incumbent(lib, g, task):
    out = ctypes.c_double()
    lib.check(lib.load().cbo_gp_plugin_incumbent(g._handle, lib.TASK_CODE[task], ctypes.byref(out)))
    return out.value


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def check_winner(acq, bv, bi, offset=0):
    """numpy's argmax: lowest index on ties, NaN maximal."""
    assert bi - offset == int(np.argmax(acq)), (bi - offset, int(np.argmax(acq)))
    assert same(bv, acq[bi - offset])


def check_every_kind(lib, g, grid, pts, offset=0, beta=1.5, jitter=0.01, cost=3.0, nontrivial=False):
    """Every kind and task on one (model, set) pair, per-candidate outputs and winner, with and without outputs; returns the
    per-candidate acquisitions by (kind, task)."""
    base = plain_sweep(lib, g, grid, 0.0, "min", 0.0, 1.0)
    mean_p, var_p = (a[:, 0] for a in g.predict(pts))
    np.testing.assert_array_equal(base[1], mean_p)
    np.testing.assert_array_equal(base[2], var_p)
    finite = base[1][np.isfinite(base[1])]
    y_best = float(np.median(finite)) if finite.size else 0.0      # PI neither 0 nor 1 everywhere
    out = {}
    with np.errstate(invalid="ignore"):
        for kind, task, param in ((LCB, "min", beta), (LCB, "max", beta), (PI, "min", jitter), (PI, "max", jitter),
                                  (VAR, "min", 0.0), (MPEI, "min", jitter), (MPEI, "max", jitter)):
            for c in (1.0, cost):
                rc, acq, mean, var, bv, bi = kind_sweep(lib, g, grid, kind, y_best, task, param, c)
                lib.check(rc)
                np.testing.assert_array_equal(mean, base[1])
                np.testing.assert_array_equal(var, base[2])
                if kind == LCB:
                    ref = -(mean - beta * np.sqrt(var)) if task == "min" else mean + beta * np.sqrt(var)
                elif kind == PI:
                    ref = feasibility(lib, g, grid, y_best, jitter, LE if task == "min" else GE)
                elif kind == VAR:
                    ref = var
                else:
                    inc = incumbent(lib, g, task)
                    ref, _, _, bv_ei, bi_ei = plain_sweep(lib, g, grid, inc, task, jitter, c)
                    assert bi == bi_ei and same(bv, bv_ei)
                np.testing.assert_array_equal(acq, ref if kind == MPEI else ref / c)
                check_winner(acq, bv, bi, offset)
                rc, _, _, _, bv2, bi2 = kind_sweep(lib, g, grid, kind, y_best, task, param, c, want=False)
                lib.check(rc)
                assert bi2 == bi and same(bv2, bv)
                out[(kind, task, c)] = acq
    pi = out[(PI, "min", 1.0)]
    if nontrivial and len(pi) >= 500:
        # (prior variance 1 and means spread about the median incumbent: far from a step function)
        assert np.mean((pi > 0.05) & (pi < 0.95)) > 0.1, "the probability of improvement is trivial on this set"
    return out


# ---- values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_sizes(lib, m):
    """An odd tail, one lane short of and one past a workgroup's span (512), a partial last workgroup, and the grid-stride
    wrap past 2048 workgroups -- a plain and a causal model, a non-zero index_offset."""
    pts = points(m, seed=m % 97)
    g, cm = random_model(seed=0), causal_model(seed=4)
    go, gc = grid_for(g, pts, index_offset=1000), grid_for(cm, pts)
    check_every_kind(lib, g, go, pts, offset=1000, nontrivial=True)
    check_every_kind(lib, cm, gc, pts, nontrivial=True)
    go.close(); gc.close()


def test_golden_fixture(lib):
    g, f = fixture_model("toy_bo_d2")
    pts = np.ascontiguousarray(f["Xs"])
    grid = grid_for(g, pts)
    check_every_kind(lib, g, grid, pts)
    grid.close()


def test_fp32_model_lower_confidence_bound(lib):
    pts = points(1500, seed=6)
    g = random_model(n=60, seed=1, dtype="f32")
    grid = grid_for(g, pts)
    for task in ("min", "max"):
        rc, acq, mean, var, bv, bi = kind_sweep(lib, g, grid, LCB, 0.0, task, 2.0, 1.5)
        lib.check(rc)
        ref = -(mean - 2.0 * np.sqrt(var)) if task == "min" else mean + 2.0 * np.sqrt(var)
        np.testing.assert_array_equal(acq, ref / 1.5)
        check_winner(acq, bv, bi)
        base = plain_sweep(lib, g, grid, 0.0, "min", 0.0, 1.0)
        np.testing.assert_array_equal(mean, base[1])
        np.testing.assert_array_equal(var, base[2])
    grid.close()


def test_plugin_incumbent_is_the_best_predicted_mean(lib):
    for g in (random_model(seed=0), causal_model(seed=4), random_model(n=33, seed=2, dtype="f32")):
        mean = g.predict(g.X)[0][:, 0]
        assert incumbent(lib, g, "min") == np.min(mean) and incumbent(lib, g, "max") == np.max(mean)
        assert np.min(mean) < np.max(mean)
    # more observations than one pass of the reduction's 256 lanes
    g = random_model(n=300, seed=5)
    mean = g.predict(g.X)[0][:, 0]
    assert incumbent(lib, g, "min") == np.min(mean) and incumbent(lib, g, "max") == np.max(mean)


def test_nan_training_prior_mean_gives_the_sweep_with_a_nan_incumbent(lib):
    X, _ = causal_data(seed=4)
    cm = causal_model(seed=4, nan_at=X[5].copy())
    pts = points(700, seed=8)
    grid = grid_for(cm, pts)
    with np.errstate(invalid="ignore"):
        for task in ("min", "max"):
            assert np.isnan(incumbent(lib, cm, task))
            rc, acq, _, _, bv, bi = kind_sweep(lib, cm, grid, MPEI, 0.0, task, 0.0, 2.0)
            lib.check(rc)
            ref, _, _, bv_ei, bi_ei = plain_sweep(lib, cm, grid, np.nan, task, 0.0, 2.0)
            np.testing.assert_array_equal(acq, ref)
            assert bi == bi_ei and same(bv, bv_ei)
    grid.close()


# ---- arg-max -----------------------------------------------------------------------------------------------------------
def test_ties_and_nan_candidates(lib):
    base = points(300, seed=9)
    pts = np.vstack([base, base, base[:50]])             # every candidate twice or three times: ties everywhere
    g = random_model(seed=0)
    grid = grid_for(g, pts, index_offset=77)
    out = check_every_kind(lib, g, grid, pts, offset=77)
    for acq in out.values():
        win = int(np.argmax(acq))
        assert win < 300 and np.sum(acq == acq[win]) >= 2      # the first of the tied copies
    grid.close()
    # NaN: the prior mean of one candidate of a causal model's set (and of its copies)
    bad = 123
    cm = causal_model(seed=5, nan_at=pts[bad].copy())
    grid = grid_for(cm, pts)
    out = check_every_kind(lib, cm, grid, pts)
    dup = [i for i in range(len(pts)) if np.array_equal(pts[i], pts[bad])]
    for (kind, _, _), acq in out.items():
        if kind == VAR:                                   # the variance does not read the prior mean
            assert not np.isnan(acq).any()
        else:
            assert int(np.argmax(acq)) == dup[0] and np.isnan(acq[dup]).all() and np.isnan(acq).sum() == len(dup)
    grid.close()


# ---- state -------------------------------------------------------------------------------------------------------------
CALLS = ((LCB, 0.0, "min", 1.5), (PI, 0.1, "max", 0.01), (VAR, 0.0, "min", 0.0), (MPEI, 0.0, "min", 0.01))


def run_calls(lib, g, grid, cost=2.5):
    res = []
    for kind, y_best, task, param in CALLS:
        out = kind_sweep(lib, g, grid, kind, y_best, task, param, cost)
        lib.check(out[0])
        res.append(out[1:])
    return res


def assert_same_results(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)


def test_repeated_cached_and_fresh_calls_give_the_same_bits_and_leave_the_ei_sweep_alone(lib):
    pts = points(2500, seed=21)
    for make in (lambda: causal_model(seed=3), lambda: random_model(seed=0)):
        g = make()
        grid = grid_for(g, pts)
        first = run_calls(lib, g, grid)                  # the first call substitutes, the others read the cached q, mu
        again = run_calls(lib, g, grid)
        assert_same_results(first, again)
        g2 = make()
        grid2 = grid_for(g2, pts)
        ei_before = plain_sweep(lib, g2, grid2, 0.2, "min", 0.0, 2.0)          # cached by cbo_acq_sweep
        state = [np.array(a, copy=True) for a in g2.posterior_state()]
        assert_same_results(first, run_calls(lib, g2, grid2))
        ei_after = plain_sweep(lib, g2, grid2, 0.2, "min", 0.0, 2.0)
        for a, b in zip(ei_before, ei_after):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(state, g2.posterior_state()):
            np.testing.assert_array_equal(a, b)
        # every kind substituting for itself (a fresh set each)
        for i, (kind, y_best, task, param) in enumerate(CALLS):
            fresh = grid_for(g2, pts)
            out = kind_sweep(lib, g2, fresh, kind, y_best, task, param, 2.5)
            lib.check(out[0])
            assert_same_results([first[i]], [out[1:]])
            fresh.close()
        grid.close(); grid2.close()


def test_appended_model_extends_its_kept_solution(lib):
    """After cbo_gp_append the call reaches q, mu by the one-row extension, as cbo_acq_sweep does: the same posterior as a
    freshly fitted model's to rounding (rtol 1e-9, atol 1e-12: the figure tests/test_constrained_gpu.py uses for it)."""
    pts = points(1200, seed=31)
    x_new, y_new = np.array([[0.3, -0.7]]), np.array([[0.25]])
    g = random_model(n=40, seed=13)
    grid = grid_for(g, pts, keep_solution=True)
    lib.check(kind_sweep(lib, g, grid, VAR)[0])           # V stays with the set
    n0 = int(lib.load().cbo_gp_n(g._handle))
    g.append(x_new, y_new)
    assert int(lib.load().cbo_gp_n(g._handle)) == n0 + 1
    extended = run_calls(lib, g, grid, cost=1.0)
    fresh_model = model(g.X, g.Y, variance=1.0, lengthscale=0.7, noise_var=1e-3)
    fresh_grid = grid_for(fresh_model, pts)
    refitted = run_calls(lib, fresh_model, fresh_grid, cost=1.0)
    for a, b in zip(extended, refitted):
        for u, v in zip(a[:3], b[:3]):                    # acquisition, mean, variance
            np.testing.assert_allclose(u, v, rtol=1e-9, atol=1e-12)
        assert a[4] == b[4] or abs(a[0][a[4]] - a[0][b[4]]) <= 1e-9 * abs(a[0][a[4]]) + 1e-12      # the winner, or a near tie
    # ... and bit for bit what the EI sweep's extension leaves: mean and variance of a second model with the same history
    g2 = random_model(n=40, seed=13)
    grid2 = grid_for(g2, pts, keep_solution=True)
    plain_sweep(lib, g2, grid2, 0.0, "min", 0.0, 1.0)
    g2.append(x_new, y_new)
    base = plain_sweep(lib, g2, grid2, 0.0, "min", 0.0, 1.0)
    np.testing.assert_array_equal(extended[0][1], base[1])
    np.testing.assert_array_equal(extended[0][2], base[2])
    for x in (grid, grid2, fresh_grid):
        x.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_invalid_and_unfitted(lib):
    from cbo_with_oop_amd import CandidateGrid
    pts = points(100, seed=41)
    g, cm = random_model(seed=0), causal_model(seed=2)
    grid = grid_for(g, pts)
    L = lib.load()

    def refused(code, *args, **kw):
        assert kind_sweep(lib, *args, **kw)[0] == code, (args, kw)
        assert L.cbo_last_error()

    assert kind_sweep(lib, g, grid, LCB, param=1.0)[0] == 0
    for kind in (0, 5, -1, 100):
        refused(INVALID, g, grid, kind)
    for kind in (LCB, PI, MPEI):
        for param in (np.nan, np.inf, -np.inf):
            refused(INVALID, g, grid, kind, param=param)
        refused(INVALID, g, grid, kind, task=7)
        refused(INVALID, g, grid, kind, task=-1)
    assert b"task" in L.cbo_last_error()
    refused(INVALID, g, grid, LCB, param=-0.5)
    assert b"beta" in L.cbo_last_error()
    for y_best in (np.nan, np.inf):
        refused(INVALID, g, grid, PI, y_best=y_best)
    for kind in (LCB, PI, VAR, MPEI):
        for cost in (0.0, -1.0, np.nan):
            refused(INVALID, g, grid, kind, cost=cost)
        refused(INVALID, None, grid, kind)
        refused(INVALID, g, None, kind)
        refused(INVALID, cm, grid, kind)                  # a causal model whose set carries no prior
        refused(INVALID, random_model(d=3, seed=4), grid, kind)
    # what a kind does not read is not checked
    assert kind_sweep(lib, g, grid, VAR, y_best=np.nan, task=7, param=np.nan)[0] == 0
    assert kind_sweep(lib, g, grid, MPEI, y_best=np.nan)[0] == 0
    assert kind_sweep(lib, g, grid, LCB, y_best=np.inf, param=0.0)[0] == 0
    other = lib.Context(grid._ctx.device_id)
    try:
        far = CandidateGrid(pts, context=other)
        refused(INVALID, g, far, VAR)
        far.close()
    finally:
        other.close()
    u = model(g.X, g.Y, variance=1.0, lengthscale=0.7, noise_var=1e-3, fit=False)
    gu = grid_for(u, pts)
    for kind in (LCB, PI, VAR, MPEI):
        refused(NOT_FITTED, u, gu, kind)
    out = ctypes.c_double()
    assert L.cbo_gp_plugin_incumbent(u._handle, 0, ctypes.byref(out)) == NOT_FITTED and L.cbo_last_error()
    assert L.cbo_gp_plugin_incumbent(g._handle, 2, ctypes.byref(out)) == INVALID and L.cbo_last_error()
    assert L.cbo_gp_plugin_incumbent(g._handle, 0, None) == INVALID
    assert L.cbo_gp_plugin_incumbent(None, 0, ctypes.byref(out)) == INVALID
    # the refusals left the valid calls working
    assert kind_sweep(lib, g, grid, PI, y_best=0.1)[0] == 0
    assert L.cbo_gp_plugin_incumbent(g._handle, 0, ctypes.byref(out)) == 0
    grid.close(); gu.close()


# ---- the Python layer --------------------------------------------------------------------------------------------------
def restated(name, g, pts, y_best, task):
    """The acquisition restated in numpy / scipy from the device's predict (find_next_y_point's defaults: beta 1, jitter 0)."""
    from scipy.stats import norm
    mean, var = (a[:, 0] for a in g.predict(pts))
    sd = np.sqrt(var)
    if name == "LCB":
        return -(mean - sd) if task == "min" else mean + sd
    if name == "VAR":
        return var
    if name == "MPEI":
        fit = g.predict(g.X)[0][:, 0]
        y_best = fit.min() if task == "min" else fit.max()
    u = (y_best - mean) / sd
    if name == "PI":
        return norm.cdf(u) if task == "min" else norm.cdf(-u)
    ei = sd * (u * norm.cdf(u) + norm.pdf(u))
    return ei if task == "min" else -ei


@pytest.mark.parametrize("name", ["LCB", "PI", "MPEI", "VAR"])
def test_find_next_y_point(lib, name):
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import find_next_y_point
    bounds = [(-2.5, 2.5)] * 2
    pts = meshgrid_candidates(bounds, [30, 30])
    for g, task in ((random_model(seed=0), "min"), (causal_model(seed=9), "max")):
        if name == "MPEI":
            task = "min"            # ('max' keeps the reference's sign quirk, -EI: its arg-max is the flat zero region)
        y_best = float(g.Y.min() if task == "min" else g.Y.max())
        for costs in ({"a": lambda c: 1.0, "b": lambda c: 1.0}, {"a": lambda c: 1.0 + np.sum(np.abs(c)), "b": lambda c: 2.0}):
            y, x = find_next_y_point(bounds, g, y_best, ["a", "b"], costs, task=task, grid_shape=[30, 30], acquisition=name)
            assert y.shape == (1, 1) and x.shape == (1, 2)
            batch_cost = sum(costs[k](pts[:, j]) for j, k in enumerate(("a", "b")))
            ref = restated(name, g, pts, y_best, task) / batch_cost
            win = int(np.argmax(ref))
            near = np.abs(ref - ref[win]) <= 1e-12 * abs(ref[win])
            got = int(np.argmin(np.abs(pts - x).sum(1)))
            assert np.array_equal(pts[got], x[0]) and near[got], (got, win)
            point_cost = sum(costs[k](x[:, j]) for j, k in enumerate(("a", "b")))
            np.testing.assert_allclose(y[0, 0], restated(name, g, x, y_best, task)[0] / point_cost, rtol=1e-12, atol=1e-300)
        # the reference's own optimiser: 100 uniform anchors, L-BFGS from the best, re-evaluated at the point found
        np.random.seed(11)
        anchors = np.hstack([np.random.uniform(lo, hi, (100, 1)) for lo, hi in bounds])
        np.random.seed(11)
        y, x = find_next_y_point(bounds, g, y_best, ["a", "b"], {"a": lambda c: 1.0, "b": lambda c: 2.0}, task=task,
                                 anchors="uniform", acquisition=name)
        assert y.shape == (1, 1) and x.shape == (1, 2) and np.all(x >= -2.5) and np.all(x <= 2.5)
        best_anchor = np.max(restated(name, g, anchors, y_best, task) / 3.0)
        assert y[0, 0] >= best_anchor - 1e-9 * abs(best_anchor), (y[0, 0], best_anchor)


@pytest.mark.parametrize("task", ["min", "max"])
def test_evaluate_with_gradients_equals_the_analytic_formulas(lib, task):
    from scipy.stats import norm
    from cbo_with_oop_amd.utils_functions import (CausalMeanPluginExpectedImprovement, CausalNegativeLowerConfidenceBound,
                                                  CausalProbabilityOfImprovement, ModelVariance)
    x = points(9, seed=3)
    sign = 1.0 if task == "min" else -1.0
    for g in (random_model(seed=0), causal_model(seed=9)):
        mean, var = g.predict(x)
        dmean, dvar = g.get_prediction_gradients(x)
        sd = np.sqrt(var)
        dsd = dvar / (2 * sd)
        y_best, beta, jitter = float(np.median(g.Y)), 1.7, 0.02
        f, df = CausalNegativeLowerConfidenceBound(task, g, beta).evaluate_with_gradients(x)
        np.testing.assert_allclose(f, -(mean - beta * sd) if task == "min" else mean + beta * sd, rtol=1e-12)
        np.testing.assert_allclose(df, -(dmean - beta * dsd) if task == "min" else dmean + beta * dsd, rtol=1e-12)
        f, df = CausalProbabilityOfImprovement(y_best, task, g, jitter).evaluate_with_gradients(x)
        u = (y_best - (mean + jitter)) / sd
        np.testing.assert_allclose(f, norm.cdf(sign * u), rtol=1e-12)
        np.testing.assert_allclose(df, sign * -norm.pdf(u) * (dmean + u * dsd) / sd, rtol=1e-12)
        f, df = ModelVariance(g).evaluate_with_gradients(x)
        np.testing.assert_allclose(f, var, rtol=1e-12)
        np.testing.assert_allclose(df, dvar, rtol=1e-12)
        acq = CausalMeanPluginExpectedImprovement(task, g, jitter)
        fit = g.predict(g.X)[0][:, 0]
        inc = fit.min() if task == "min" else fit.max()
        assert acq.incumbent() == inc
        f, df = acq.evaluate_with_gradients(x)
        u = (inc - (mean + jitter)) / sd
        np.testing.assert_allclose(f, sign * sd * (u * norm.cdf(u) + norm.pdf(u)), rtol=1e-12)
        np.testing.assert_allclose(df, sign * (dsd * norm.pdf(u) - norm.cdf(u) * dmean), rtol=1e-12)
        # evaluate() is the device's value of the same formula
        for a in (CausalNegativeLowerConfidenceBound(task, g, beta), ModelVariance(g)):
            np.testing.assert_allclose(a.evaluate(x), a.evaluate_with_gradients(x)[0], rtol=1e-12)
