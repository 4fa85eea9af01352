"""GPU tests of the per-candidate intervention costs: cbo_cands_set_cost / _get_cost (cands_cost_kernel),
cbo_acq_sweep_pointcost (pointcost_acq_kernel: acq_pass with the cost stream), cbo_acq_sweep_sets_pointcost
(small_sets_kernel<kEiPointKind / kLogEiPointKind>), cbo_acq_refine_sets_pointcost (small_sets_refine_kernel of the same kinds)
and the Python layers on top.

Everything but two comparisons is exact, as bit patterns: the cost vector against ``one_row_cost``, the EI form against
cbo_acq_sweep's values divided in numpy, mean and variance against cbo_acq_sweep's, the one launch against the per-set calls on
fitted twins, the refinement's value against the one-point sweep.  The log form subtracts the DEVICE library's log(c_j): it is
held to |delta| <= ulp(log c_j) + the rounding of the subtraction's result against numpy's logarithm, the number of differing
candidates printed.  The device gradient is held to the project's 1e-9 (relative to max(1, |g|)) against the host class."""
import ctypes
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOT_FITTED = -5
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    assert _lib.CBO_ERR_INVALID == INVALID
    return _lib


def gp(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def mean_f(a):
    return 0.3 * np.sin(a).sum(1, keepdims=True)


def var_f(a):
    return 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def handles(objs):
    return (ctypes.c_void_p * len(objs))(*[o._handle for o in objs])


def table_of(d):
    """The cost table the tests price with: fix (1, 2, 0.5), flags (1, 0, 1) -- column 1 is a fixed cost alone."""
    return np.array([1.0, 2.0, 0.5][:d]), np.array([1, 0, 1][:d], dtype=np.int32)


def set_cost(lib, grid, fix, variable):
    fix, variable = np.ascontiguousarray(fix, dtype=np.float64), np.ascontiguousarray(variable, dtype=np.int32)
    return lib.load().cbo_cands_set_cost(grid._handle, lib.dptr(fix), variable.ctypes.data_as(lib.c_int_p))


def get_cost(lib, grid):
    out = np.full(len(grid), -7.0)
    lib.check(lib.load().cbo_cands_get_cost(grid._handle, lib.dptr(out)))
    return out


def host_cost(fix, variable, pts):
    from cbo_with_oop_amd.utils_functions.causal_optimizer import one_row_cost
    return np.array([one_row_cost(fix, variable, row) for row in pts])


def sweep_pointcost(lib, model, grid, log_form, y_best, task, jitter=0.0, want=True):
    m = len(grid)
    acq, mean, var = (np.empty(m), np.empty(m), np.empty(m)) if want else (None, None, None)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep_pointcost(model._handle, grid._handle, int(log_form), float(y_best), lib.TASK_CODE[task],
                                                 float(jitter), lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                                 ctypes.byref(bi)))
    return dict(acq=acq, mean=mean, var=var, best_val=bv.value, best_idx=bi.value)


def sweep_plain(lib, model, grid, log_form, y_best, task, jitter=0.0):
    """cbo_acq_sweep (EI) or cbo_acq_sweep_logei at cost 1."""
    m = len(grid)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    call = lib.load().cbo_acq_sweep_logei if log_form else lib.load().cbo_acq_sweep
    lib.check(call(model._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter), 1.0, lib.dptr(acq),
                   lib.dptr(mean), lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi)))
    return dict(acq=acq, mean=mean, var=var, best_val=bv.value, best_idx=bi.value)


def numpy_argmax(acq):
    """numpy.argmax's rule: NaN is maximal, the lowest index wins ties."""
    return int(np.argmax(acq))


# ------------------------------------------------------------------------------------------------------------ 1. the cost vector
def test_the_cost_vector_is_one_row_cost(lib):
    from cbo_with_oop_amd import CandidateGrid
    rng = np.random.default_rng(1)
    ctx = lib.Context.get(0)
    # d = 1
    pts = rng.uniform(-5, 20, (513, 1))
    grid = CandidateGrid(pts, context=ctx)
    out = np.empty(513)
    assert lib.load().cbo_cands_get_cost(grid._handle, lib.dptr(out)) == INVALID and b"cost vector" in lib.load().cbo_last_error()
    lib.check(set_cost(lib, grid, [1.0], [1]))
    assert np.array_equal(bits(get_cost(lib, grid)), bits(host_cost([1.0], [1], pts)))
    # ... a second table replaces the first; clearing drops it
    lib.check(set_cost(lib, grid, [0.25], [0]))
    assert np.all(get_cost(lib, grid) == 0.25)
    lib.check(lib.load().cbo_cands_clear_cost(grid._handle))
    assert lib.load().cbo_cands_get_cost(grid._handle, lib.dptr(out)) == INVALID
    # the checks of the table
    for fix, flags, word in (([0.0], [1], b"positive"), ([-1.0], [0], b"positive"), ([np.nan], [1], b"finite"),
                             ([np.inf], [1], b"finite"), ([1.0], [2], b"cost_variable"), ([1.0], [-1], b"cost_variable")):
        assert set_cost(lib, grid, fix, flags) == INVALID and word in lib.load().cbo_last_error(), (fix, flags)
    assert lib.load().cbo_cands_get_cost(grid._handle, lib.dptr(out)) == INVALID      # (a refused table leaves none)
    grid.close()
    # d = 3, flags (1, 0, 1); zeros, negative values and one NaN row
    pts = rng.uniform(-3, 3, (130, 3))
    pts[0] = 0.0
    pts[1] = [-1.5, -2.5, -0.0]
    pts[7] = [np.nan, 1.0, 2.0]
    pts[9] = [1.0, np.nan, 2.0]          # (a NaN in the fixed-cost column does not reach the cost)
    fix, flags = table_of(3)
    grid = CandidateGrid(pts, context=ctx)
    lib.check(set_cost(lib, grid, fix, flags))
    got, want = get_cost(lib, grid), host_cost(fix, flags, pts)
    assert np.isnan(got[7]) and np.isnan(want[7]) and got[9] == want[9] == 1.0 + 1.0 + 2.0 + 0.5 + 2.0
    keep = ~np.isnan(want)
    assert np.array_equal(bits(got[keep]), bits(want[keep])) and got[0] == 3.5
    grid.close()


# ------------------------------------------------------------------------------------------------------------ 2. the pass
class Fitted:
    def __init__(self, n, d, m, ard=False, causal=False, seed=None, keep_solution=False):
        from cbo_with_oop_amd import CandidateGrid
        rng = np.random.default_rng(100 * n + d if seed is None else seed)
        self.X = rng.uniform(-5.0, 5.0, (n, d))
        self.y = np.cos(self.X).sum(1, keepdims=True) - np.exp(-self.X[:, :1] / 20.0)
        self.kw = dict(variance=1.0, lengthscale=(0.8 + 0.3 * np.arange(d)) if ard else 1.0, ard=ard, noise_var=1e-4)
        if causal:
            self.kw.update(mean_function=mean_f, variance_adjustment=var_f)
        self.model = gp(self.X, self.y, **self.kw)
        self.points = rng.uniform(self.X.min(0) - 0.5, self.X.max(0) + 0.5, (m, d))
        self.grid = CandidateGrid(self.points, self.model, keep_solution=keep_solution)
        self.fix, self.flags = table_of(d)

    def close(self):
        self.grid.close()
        self.model.close()


def check_pass(lib, c, task, log_form, y_best, jitter=0.0078125):
    cost = get_cost(lib, c.grid)
    res = sweep_pointcost(lib, c.model, c.grid, log_form, y_best, task, jitter)
    plain = sweep_plain(lib, c.model, c.grid, log_form, y_best, task, jitter)
    ei = sweep_plain(lib, c.model, c.grid, False, y_best, task, jitter)
    assert np.array_equal(bits(res["mean"]), bits(ei["mean"])) and np.array_equal(bits(res["var"]), bits(ei["var"]))
    if not log_form:
        assert np.array_equal(bits(res["acq"]), bits(plain["acq"] / cost))
    else:
        # the device's log(c_j) against numpy's: at most one ulp of log c_j apart, plus the subtraction's own rounding
        want = plain["acq"] - np.log(cost)
        differ = int(np.sum(bits(res["acq"]) != bits(want)))
        bound = np.spacing(np.abs(np.log(cost))) + np.spacing(np.abs(want))
        print(f"log form, m={len(cost)} task={task}: {differ} of {len(cost)} candidates differ from numpy's log in the last bit")
        assert np.all(np.abs(res["acq"] - want) <= bound)
    assert res["best_idx"] == numpy_argmax(res["acq"]) + c.grid.index_offset
    assert bits(res["best_val"])[0] == bits(res["acq"][res["best_idx"] - c.grid.index_offset])[0]
    # the arg-max without the per-candidate outputs is the same
    lean = sweep_pointcost(lib, c.model, c.grid, log_form, y_best, task, jitter, want=False)
    assert lean["best_idx"] == res["best_idx"] and bits(lean["best_val"])[0] == bits(res["best_val"])[0]
    return res


# the pair tail and the 512-candidate span boundary (n = 12, d = 1); d = 3 ARD; a causal model
PASS_SHAPES = {f"n12 d1 m{m}": dict(n=12, d=1, m=m) for m in (1, 2, 511, 512, 513, 1025)}
PASS_SHAPES["n17 d3 ard m63"] = dict(n=17, d=3, m=63, ard=True)
PASS_SHAPES["n12 d1 m257 causal"] = dict(n=12, d=1, m=257, causal=True)


@pytest.fixture(scope="module")
def fitted(lib):
    cases = {name: Fitted(**kw) for name, kw in PASS_SHAPES.items()}
    for c in cases.values():
        lib.check(set_cost(lib, c.grid, c.fix, c.flags))
    yield cases
    for c in cases.values():
        c.close()


@pytest.mark.parametrize("log_form", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("name", list(PASS_SHAPES))
def test_the_pass(lib, fitted, name, task, log_form):
    c = fitted[name]
    check_pass(lib, c, task, log_form, float(c.y.min()) if task == "min" else float(c.y.max()))


@pytest.mark.parametrize("log_form", [0, 1])
def test_the_pass_with_a_second_grid_stride_iteration(lib, log_form):
    """m = 2048 * 512 + 513: the grid-stride loop of the 2048 workgroups runs a second iteration, which ends in a tail."""
    c = Fitted(12, 1, 2048 * 512 + 513)
    lib.check(set_cost(lib, c.grid, c.fix, c.flags))
    check_pass(lib, c, "min", log_form, float(c.y.min()))
    c.close()


def test_a_nan_cost_is_maximal_and_a_set_without_costs_is_refused(lib):
    from cbo_with_oop_amd import CandidateGrid
    c = Fitted(12, 1, 300)
    r = lib.load().cbo_acq_sweep_pointcost(c.model._handle, c.grid._handle, 0, 0.0, 0, 0.0, None, None, None, None, None)
    assert r == INVALID and b"cost vector" in lib.load().cbo_last_error()
    pts = c.points.copy()
    pts[211, 0] = np.nan
    pts[17, 0] = np.nan
    grid = CandidateGrid(pts, c.model, index_offset=1000)
    lib.check(set_cost(lib, grid, c.fix, c.flags))
    for log_form in (0, 1):
        res = sweep_pointcost(lib, c.model, grid, log_form, float(c.y.min()), "min")
        assert np.isnan(res["acq"][17]) and np.isnan(res["acq"][211]) and res["best_idx"] == 1017 and np.isnan(res["best_val"])
    grid.close()
    c.close()


def test_after_an_append_and_from_a_kept_solution(lib):
    """The route to q, mu is cbo_acq_sweep's.  A sweep from a kept solution and one from the cached vectors return the bits of a
    fresh fit's sweep.  After cbo_gp_append the solution is extended by one row: bit for bit what cbo_acq_sweep's own values
    over the cost vector give after the same append -- and, against a freshly fitted model, the row update's rounding, which
    the library has for every sweep (rtol 1e-9, atol 1e-12: the figures tests/test_pointwise_gpu.py holds the same step to;
    measured here: 327 of 513 EI values differ in the last bits, 4.2e-9 relative at worst, on values below 1e-50)."""
    c = Fitted(12, 1, 513, keep_solution=True)
    lib.check(set_cost(lib, c.grid, c.fix, c.flags))
    y_best = float(c.y.min())
    first = sweep_pointcost(lib, c.model, c.grid, 0, y_best, "min")
    cached = sweep_pointcost(lib, c.model, c.grid, 0, y_best, "min")                 # (from the cached q, mu)
    assert np.array_equal(bits(first["acq"]), bits(cached["acq"]))
    fresh = Fitted(12, 1, 513)                                                        # (the same data, nothing kept)
    lib.check(set_cost(lib, fresh.grid, c.fix, c.flags))
    assert np.array_equal(bits(sweep_pointcost(lib, fresh.model, fresh.grid, 0, y_best, "min")["acq"]), bits(cached["acq"]))
    x_new, y_new = np.array([[0.123]]), np.array([[0.5]])
    assert c.model.append(x_new, y_new)
    fresh.model.close()
    fresh.model = gp(np.vstack([c.X, x_new]), np.vstack([c.y, y_new]), **c.kw)
    lib.check(set_cost(lib, fresh.grid, c.fix, c.flags))
    for log_form in (0, 1):
        got = sweep_pointcost(lib, c.model, c.grid, log_form, y_best, "min")
        want = sweep_pointcost(lib, fresh.model, fresh.grid, log_form, y_best, "min")
        appended = sweep_plain(lib, c.model, c.grid, log_form, y_best, "min")
        # (what an append gives is cbo_acq_sweep's own after that append: the row update, not a refit)
        cost = get_cost(lib, c.grid)
        if not log_form:
            assert np.array_equal(bits(got["acq"]), bits(appended["acq"] / cost))
        else:
            # cbo_acq_sweep_logei after the same append, minus numpy's log(c_j): the pass's own bound (check_pass)
            after = appended["acq"] - np.log(cost)
            assert np.all(np.abs(got["acq"] - after) <= np.spacing(np.abs(np.log(cost))) + np.spacing(np.abs(after)))
        assert np.array_equal(bits(got["mean"]), bits(appended["mean"])) and got["best_idx"] == numpy_argmax(got["acq"])
        diff = np.abs(got["acq"] - want["acq"]) / np.maximum(np.abs(want["acq"]), 1e-300)
        print(f"log_form={log_form}: appended against a fresh fit, {int(np.sum(bits(got['acq']) != bits(want['acq'])))} of 513 "
              f"candidates differ, worst relative {diff.max():.3e}")
        np.testing.assert_allclose(got["acq"], want["acq"], rtol=1e-9, atol=1e-12)
    fresh.close()
    c.close()


class Example:
    """The arg-max example of DESIGN.md §4y: n = 12, seed 7, hyper-parameters (1, 1, 1e-4), 200 grid points, cost 1 + |x|."""

    def __init__(self):
        from cbo_with_oop_amd import CandidateGrid
        self.X = np.random.default_rng(7).uniform(-5, 20, (12, 1))
        self.y = np.cos(self.X) - np.exp(-self.X / 20)
        self.kw = dict(variance=1.0, lengthscale=1.0, noise_var=1e-4)
        self.model = gp(self.X, self.y, **self.kw)
        self.points = np.linspace(-5, 20, 200)[:, None]
        self.grid = CandidateGrid(self.points, self.model)
        self.y_best = float(self.y.min())
        self.lo, self.hi, self.d = np.array([-5.0]), np.array([20.0]), 1


@pytest.fixture(scope="module")
def example(lib):
    e = Example()
    lib.check(set_cost(lib, e.grid, [1.0], [1]))
    yield e
    e.grid.close()
    e.model.close()


def test_the_argmax_example(lib, example):
    plain = sweep_plain(lib, example.model, example.grid, False, example.y_best, "min")
    priced = sweep_pointcost(lib, example.model, example.grid, 0, example.y_best, "min")
    print("EI arg-max", plain["best_idx"], "EI / c arg-max", priced["best_idx"])
    assert plain["best_idx"] == 65 and priced["best_idx"] == 64
    assert sweep_pointcost(lib, example.model, example.grid, 1, example.y_best, "min")["best_idx"] == 64


# ------------------------------------------------------------------------------------------------------------ 3. one launch
class Pair:
    """One exploration set twice: the model under test (never fitted) with its grid, and the fitted twin with its own."""

    def __init__(self, lib, n, m, d, causal=False, ard=False, offset=0, dtype=None, noise_var=1e-3):
        from cbo_with_oop_amd import CandidateGrid
        rng = np.random.default_rng(1000 * n + 10 * m + d)
        X = rng.uniform(-2.0, 2.0, (n, d))
        y = np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))
        pts = rng.uniform(-2.5, 2.5, (m, d))
        kw = dict(variance=1.3, lengthscale=(0.7 + 0.2 * np.arange(d)) if ard else 0.9, ard=ard, noise_var=noise_var)
        if causal:
            kw.update(mean_function=mean_f, variance_adjustment=var_f)
        if dtype:
            kw.update(dtype=dtype)
        self.model, self.twin = gp(X, y, fit=False, **kw), gp(X, y, **kw)
        self.grid = CandidateGrid(pts, self.model, index_offset=offset)
        self.twin_grid = CandidateGrid(pts, self.twin, index_offset=offset)
        for g in (self.grid, self.twin_grid):
            lib.check(set_cost(lib, g, *table_of(d)))

    def close(self):
        for o in (self.grid, self.twin_grid, self.model, self.twin):
            o.close()


def sweep_sets_pointcost(lib, models, grids, log_form, y_best, task, jitter=0.0):
    s = len(models)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)))
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    rc = lib.load().cbo_acq_sweep_sets_pointcost(s, handles(models), handles(grids), int(log_form), lib.dptr(yb),
                                                 lib.TASK_CODE[task], float(jitter), lib.dptr(vals),
                                                 idxs.ctypes.data_as(lib.c_int64_p))
    return rc, vals, idxs


def per_set(lib, pairs, log_form, y_best, task, jitter):
    vals, idxs = np.empty(len(pairs)), np.empty(len(pairs), dtype=np.int64)
    for i, p in enumerate(pairs):
        p.twin.ensure_fitted()
        r = sweep_pointcost(lib, p.twin, p.twin_grid, log_form, y_best[i], task, jitter, want=False)
        vals[i], idxs[i] = r["best_val"], r["best_idx"]
    return vals, idxs


# (n, m) in {(1, 1), (16, 63), (17, 257), (128, 200), (20, 769)} x d in {1, 3}; ARD and causal sets; an index offset;
# 769 candidates are 13 blocks: the two-launch form
NINE = [dict(n=1, m=1, d=1), dict(n=16, m=63, d=3), dict(n=17, m=257, d=1, causal=True), dict(n=128, m=200, d=3, ard=True),
        dict(n=20, m=769, d=1), dict(n=16, m=63, d=1, offset=4000), dict(n=17, m=257, d=3), dict(n=128, m=200, d=1),
        dict(n=16, m=63, d=3, causal=True)]


@pytest.fixture(scope="module")
def nine(lib):
    pairs = [Pair(lib, **kw) for kw in NINE]
    yield pairs
    for p in pairs:
        p.close()


@pytest.mark.parametrize("log_form", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("count", [2, 9])
def test_one_launch_equals_the_per_set_calls(lib, nine, count, task, log_form):
    pairs = nine[2:4] if count == 2 else nine
    y_best = np.linspace(-0.6, 0.4, count)
    rc, vals, idxs = sweep_sets_pointcost(lib, [p.model for p in pairs], [p.grid for p in pairs], log_form, y_best, task, 0.01)
    lib.check(rc)
    want_v, want_i = per_set(lib, pairs, log_form, y_best, task, 0.01)
    print(task, count, log_form, "values", vals.tolist(), "indices", idxs.tolist())
    assert np.array_equal(idxs, want_i) and np.array_equal(bits(vals), bits(want_v))
    out = np.empty(1)
    for p in pairs:
        assert p.model.stale and lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == NOT_FITTED


def test_the_two_launch_form_alone(lib, nine):
    rc, vals, idxs = sweep_sets_pointcost(lib, [nine[4].model], [nine[4].grid], 0, [0.0], "min")
    lib.check(rc)
    want_v, want_i = per_set(lib, [nine[4]], 0, [0.0], "min", 0.0)
    assert idxs[0] == want_i[0] and bits(vals)[0] == bits(want_v)[0]


def test_mixed_routing_and_untouched_models(lib, nine):
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    large, single = Pair(lib, 129, 100, 2), Pair(lib, 40, 90, 2, dtype="f32", noise_var=1e-2)
    small = nine[1]
    kept_grid = CandidateGrid(small.twin_grid.points, small.twin, keep_solution=True)
    lib.check(set_cost(lib, kept_grid, *table_of(3)))
    ei = CausalExpectedImprovement(0.1, "min", small.twin)
    before = ei.sweep(kept_grid, cost=1.0, want_acq=True)
    lml_before, lml_after = np.empty(1), np.empty(1)
    assert lib.load().cbo_gp_log_marginal(small.twin._handle, lib.dptr(lml_before)) == 0 and not small.twin.stale
    pairs = [small, large, single, nine[2]]
    models = [small.twin, large.model, single.model, nine[2].model]
    grids = [kept_grid, large.grid, single.grid, nine[2].grid]
    y_best = np.array([0.1, -0.2, 0.3, 0.0])
    for log_form in (0, 1):
        rc, vals, idxs = sweep_sets_pointcost(lib, models, grids, log_form, y_best, "min")
        lib.check(rc)
        want_v, want_i = per_set(lib, pairs, log_form, y_best, "min", 0.0)
        print("mixed", log_form, vals.tolist(), want_v.tolist(), idxs.tolist(), want_i.tolist())
        assert np.array_equal(idxs, want_i) and np.array_equal(bits(vals), bits(want_v))
    assert lib.load().cbo_gp_log_marginal(small.twin._handle, lib.dptr(lml_after)) == 0 and not small.twin.stale
    assert bits(lml_after)[0] == bits(lml_before)[0]
    after = ei.sweep(kept_grid, cost=1.0, want_acq=True)
    assert np.array_equal(bits(before["acq"]), bits(after["acq"])) and before["best_idx"] == after["best_idx"]
    out = np.empty(1)
    assert nine[2].model.stale and lib.load().cbo_gp_log_marginal(nine[2].model._handle, lib.dptr(out)) == NOT_FITTED
    # a set without a cost vector is refused before anything runs
    bare = CandidateGrid(small.twin_grid.points, small.twin)
    rc, _, _ = sweep_sets_pointcost(lib, [small.twin, small.twin], [kept_grid, bare], 0, [0.0, 0.0], "min")
    assert rc == INVALID and b"cost vector" in lib.load().cbo_last_error() and b"set 1" in lib.load().cbo_last_error()
    bare.close(); kept_grid.close(); large.close(); single.close()


# ------------------------------------------------------------------------------------------------------------ 4. refinement
class Case:
    def __init__(self, n, d, seed=0, **extra):
        rng = np.random.default_rng(1000 * n + 10 * d + seed)
        self.lo, self.hi, self.d = np.full(d, -2.0), np.full(d, 2.0), d
        self.X = rng.uniform(self.lo, self.hi, (n, d))
        self.y = np.sin(1.3 * self.X[:, :1]) + 0.3 * (self.X[:, 1:] ** 2).sum(1, keepdims=True) / max(d - 1, 1)
        self.kw = dict(variance=1.2, lengthscale=1.1, noise_var=1e-2, **extra)
        self.model, self.twin = gp(self.X, self.y, fit=False, **self.kw), gp(self.X, self.y, **self.kw)
        self.y_best = float(self.y.min()) - 0.5
        self.rng = rng

    def close(self):
        self.model.close()
        self.twin.close()


def refine_pointcost(lib, cases, starts, costs, log_form, y_best, task="min", jitter=0.0, max_rounds=200, sentinel=0.0):
    n = len(cases)
    starts = [np.ascontiguousarray(s, dtype=np.float64) for s in starts]
    keep = []
    sets = (lib.CboRefineSet * n)()
    for j, c in enumerate(cases):
        lo, hi = np.ascontiguousarray(c.lo, dtype=np.float64), np.ascontiguousarray(c.hi, dtype=np.float64)
        fix, variable = (np.ascontiguousarray(costs[j][0], dtype=np.float64), np.ascontiguousarray(costs[j][1], dtype=np.int32))
        keep += [lo, hi, fix, variable]
        sets[j].k = starts[j].shape[0]
        sets[j].starts = starts[j].ctypes.data_as(lib.c_double_p)
        sets[j].lo, sets[j].hi = lo.ctypes.data_as(lib.c_double_p), hi.ctypes.data_as(lib.c_double_p)
        sets[j].cost_fix, sets[j].cost_variable = fix.ctypes.data_as(lib.c_double_p), variable.ctypes.data_as(lib.c_int_p)
    rows, total = sum(s.size for s in starts), sum(s.shape[0] for s in starts)
    x, g, v = np.full(rows, sentinel), np.full(rows, sentinel), np.full(total, sentinel)
    rounds, status = np.full(total, int(sentinel), dtype=np.int32), np.full(total, int(sentinel), dtype=np.int32)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (n,)))
    rc = lib.load().cbo_acq_refine_sets_pointcost(n, handles([c.model for c in cases]), sets, int(log_form), lib.dptr(yb),
                                                  lib.TASK_CODE[task], jitter, max_rounds, lib.dptr(x), lib.dptr(v), lib.dptr(g),
                                                  rounds.ctypes.data_as(lib.c_int_p), status.ctypes.data_as(lib.c_int_p))
    out, r0, o0 = [], 0, 0
    for s in starts:
        k, d = s.shape
        out.append((x[r0:r0 + k * d].reshape(k, d), v[o0:o0 + k], g[r0:r0 + k * d].reshape(k, d), rounds[o0:o0 + k],
                    status[o0:o0 + k]))
        r0, o0 = r0 + k * d, o0 + k
    return rc, out


def one_point_sweep(lib, model, x, table, log_form, y_best, task, jitter):
    from cbo_with_oop_amd import CandidateGrid
    grid = CandidateGrid(np.ascontiguousarray(x[None, :]), model)
    lib.check(set_cost(lib, grid, *table))
    rc, vals, _ = sweep_sets_pointcost(lib, [model], [grid], log_form, y_best, task, jitter)
    lib.check(rc)
    grid.close()
    return vals[0]


def host_quotient(log_form, y_best, task, model, jitter, table, names):
    import functools
    from cbo_with_oop_amd import graphs
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalLogExpectedImprovement, PointwiseCost
    funcs = {n: functools.partial(graphs.cost, float(f), bool(v)) for n, f, v in zip(names, table[0], table[1])}
    num = (CausalLogExpectedImprovement if log_form else CausalExpectedImprovement)(y_best, task, model, jitter)
    return num / PointwiseCost(funcs, names)


@pytest.mark.parametrize("log_form", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("n,d,k", [(10, 1, 8), (16, 3, 4)])
def test_value_and_gradient_at_the_starts(lib, n, d, k, task, log_form):
    """max_rounds = 0.  The value: bit for bit the point-cost sets sweep on a one-point grid there.  The gradient: within 1e-9
    (relative to max(1, |g|), the project's bound for device gradients) of ``PointCostQuotient.evaluate_with_gradients``.
    One start has x_k = 0 in a variable column (sign(0) = 0); d = 3 prices with flags (1, 0, 1)."""
    c = Case(n, d)
    y_best = c.y_best if task == "min" else float(c.y.max()) + 0.5
    jitter = 0.0078125
    pts = c.rng.uniform(c.lo, c.hi, (k, d))
    pts[1, 0] = 0.0
    pts[2] = -np.abs(pts[2])
    table = table_of(d)
    rc, ((x, val, grad, rounds, status),) = refine_pointcost(lib, [c], [pts], [table], log_form, y_best, task, jitter, max_rounds=0)
    lib.check(rc)
    assert np.array_equal(x, pts) and np.all(rounds == 0)
    for i in range(k):
        assert bits(val[i])[0] == bits(one_point_sweep(lib, c.model, pts[i], table, log_form, y_best, task, jitter))[0], (i, pts[i])
    f, df = host_quotient(log_form, y_best, task, c.twin, jitter, table, ["X", "Z", "W"][:d]).evaluate_with_gradients(pts)
    rel = np.abs(grad - df) / np.maximum(1.0, np.abs(df))
    print(f"n{n} d{d} {task} log_form={log_form}: gradient against the host class, worst {rel.max():.3e}")
    assert rel.max() <= 1e-9
    assert np.allclose(val, f[:, 0], rtol=1e-7, atol=1e-300)           # (a sanity check: the bits are pinned above)
    out = np.empty(1)
    assert c.model.stale and lib.load().cbo_gp_log_marginal(c.model._handle, lib.dptr(out)) == NOT_FITTED
    c.close()


@pytest.mark.parametrize("log_form", [0, 1])
def test_a_search_from_the_grid_winner_does_not_end_lower(lib, example, log_form):
    start = example.points[64][None, :]
    table = (np.array([1.0]), np.array([1], dtype=np.int32))
    rc, ((_, v0, _, _, _),) = refine_pointcost(lib, [example], [start], [table], log_form, example.y_best, max_rounds=0)
    lib.check(rc)
    rc, ((x, v, g, r, s),) = refine_pointcost(lib, [example], [start], [table], log_form, example.y_best)
    lib.check(rc)
    print("start", start.tolist(), v0.tolist(), "end", x.tolist(), v.tolist(), "rounds", r.tolist(), "status", s.tolist())
    grid_val = sweep_pointcost(lib, example.model, example.grid, log_form, example.y_best, "min")["best_val"]
    assert bits(v0)[0] == bits(grid_val)[0]
    assert v[0] >= v0[0] and example.lo[0] <= x[0, 0] <= example.hi[0]
    assert s[0] not in (lib.REFINE_NAN_START, lib.REFINE_DECLINED)
    assert bits(v[0])[0] == bits(one_point_sweep(lib, example.model, x[0], table, log_form, example.y_best, "min", 0.0))[0]


def test_causal_large_and_fp32_sets_are_declined_and_answered_by_the_host_route(lib):
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost,
                                                   PointwiseCost)
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    rng = np.random.default_rng(5)

    class Set:
        def __init__(self, n, **kw):
            self.X = rng.uniform(-2.0, 2.0, (n, 1))
            self.y = np.sin(1.3 * self.X)
            self.model = gp(self.X, self.y, variance=1.2, lengthscale=1.1, noise_var=1e-2, **kw)
            self.lo, self.hi, self.d = np.array([-2.0]), np.array([2.0]), 1
    sets = [Set(20), Set(20, mean_function=mean_f, variance_adjustment=var_f), Set(129), Set(20, dtype="f32")]
    starts = [rng.uniform(-2.0, 2.0, (3, 1)) for _ in sets]
    cost = (np.ones(1), np.ones(1, dtype=np.int32))
    rc, res = refine_pointcost(lib, sets, starts, [cost] * 4, 0, 0.0, sentinel=-77.0)
    lib.check(rc)
    assert np.all(res[0][4] != lib.REFINE_DECLINED) and np.all(res[0][1] != -77.0)
    for i in (1, 2, 3):
        x, val, grad, rounds, status = res[i]
        assert np.all(status == lib.REFINE_DECLINED)
        assert np.all(x == -77.0) and np.all(val == -77.0) and np.all(grad == -77.0) and np.all(rounds == -77)
    # the checks of the table are cbo_acq_refine_sets'
    for bad, word in (((np.zeros(1), np.ones(1, dtype=np.int32)), b"positive"), ((np.ones(1), np.full(1, 2, dtype=np.int32)), b"cost_variable")):
        rc, _ = refine_pointcost(lib, sets[:1], starts[:1], [bad], 0, 0.0)
        assert rc == INVALID and word in lib.load().cbo_last_error()
    # refine_sets: the eligible set from the launch, the others refine_batched's own on the point-cost quotient
    table = ToyGraph.get_cost_structure(4)                          # 1 + |x|
    price, boxes = Cost(table, ["X"]), [[(-2.0, 2.0)]] * 4
    models = [s.model for s in sets]
    got = refine_sets(models, starts, boxes, 0.0, "min", [price] * 4, cost_mode="pointwise")
    assert np.array_equal(bits(got[0][0]), bits(res[0][0])) and np.array_equal(bits(got[0][1]), bits(res[0][1]))
    assert np.array_equal(got[0][2], res[0][4])
    for i in (1, 2, 3):
        acq = CausalExpectedImprovement(0.0, "min", models[i]) / PointwiseCost(table, ["X"])
        xs, fs = CausalGradientAcquisitionOptimizer(boxes[i]).refine_batched(acq, starts[i])
        assert np.array_equal(bits(got[i][0]), bits(xs)) and np.array_equal(bits(got[i][1]), bits(fs))
        assert np.all(got[i][2] == lib.REFINE_DECLINED) and np.all(np.isfinite(got[i][1]))
    # optimize(refine=True, device=True, cost_mode="pointwise") takes the eligible set and refuses the causal one
    opt = CausalGradientAcquisitionOptimizer(boxes[0], grid_shape=[40])
    quotient = CausalExpectedImprovement(0.0, "min", models[0]) / PointwiseCost(table, ["X"])
    x0, f0 = opt.optimize(quotient, cost_mode="pointwise")
    x1, f1 = opt.optimize(quotient, refine=True, num_starts=4, device=True, cost_mode="pointwise")
    assert f1[0, 0] >= f0[0, 0] and -2.0 <= x1[0, 0] <= 2.0
    with pytest.raises(ValueError, match="device=True"):
        CausalGradientAcquisitionOptimizer(boxes[1], grid_shape=[40]).optimize(
            CausalExpectedImprovement(0.0, "min", models[1]) / PointwiseCost(table, ["X"]), refine=True, device=True,
            cost_mode="pointwise")
    for s in sets:
        s.model.close()


# ------------------------------------------------------------------------------------------------------------ 5. Python surface
@pytest.mark.parametrize("acquisition", ["EI", "LOGEI"])
@pytest.mark.parametrize("refine", [False, True])
def test_find_next_y_points_on_the_toy_graph(lib, refine, acquisition):
    """Per set the multi-set call equals the single-set call, and the value is the quotient's own at the returned point."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import PointwiseCost, find_next_y_point, find_next_y_points
    from cbo_with_oop_amd.utils_functions.utils import _acquisition_for
    rng = np.random.default_rng(3)
    es = ToyGraph.get_exploration_set("MIS")
    xs = [rng.uniform(-5, 5, (20, 1)), rng.uniform(-5, 20, (50, 1))]
    ys = [ToyGraph.target_do_x(xs[0]), ToyGraph.target_do_z(xs[1])]
    table = ToyGraph.get_cost_structure(4)                          # 1 + |x|
    spaces = [ToyGraph.bounds(s) for s in es]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys, spaces, grid_shapes=[[200], [200]],
                              comm=None, acquisition=acquisition, refine=refine, cost_mode="pointwise")
    path.update_all_gaussian_processes()
    incumbent = min(float(ys[0].min()), float(ys[1].min()))
    grids = [path.candidate_grid(s) for s in range(2)]
    kw = dict(refine=True, spaces=spaces) if refine else {}
    x_new, y_new = find_next_y_points(path.models, incumbent, es, table, "min", grids, acquisition=acquisition,
                                      cost_mode="pointwise", **kw)
    for s in range(2):
        quotient = _acquisition_for(acquisition, path.models[s], incumbent, "min", None) / PointwiseCost(table, es[s])
        again = quotient.evaluate(x_new[s])
        print("set", s, "x", x_new[s].tolist(), "value", y_new[s].tolist(), "cost", quotient.denominator.evaluate(x_new[s]).tolist())
        assert x_new[s].shape == (1, 1) and y_new[s].shape == (1, 1) and np.isfinite(y_new[s][0, 0])
        assert bits(y_new[s])[0] == bits(again)[0]                     # (the winner's own EI / c(x): nothing re-priced)
        y_one, x_one = find_next_y_point(spaces[s], path.models[s], incumbent, es[s], table, candidates=grids[s],
                                         acquisition=acquisition, cost_mode="pointwise")
        if not refine:
            assert np.array_equal(x_one, x_new[s]) and bits(y_one)[0] == bits(y_new[s])[0]
            assert np.any(np.all(grids[s].points == x_new[s], axis=1))
        else:
            assert y_new[s][0, 0] >= y_one[0, 0]
    x_path, y_path = path.compute_best_acquisition_values(incumbent)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(y_path, y_new))
    assert all(np.array_equal(a, b) for a, b in zip(x_path, x_new))
    # the default mode of the same path data is the batch-priced value: another number
    x_old, y_old = find_next_y_points(path.models, incumbent, es, table, "min", grids, acquisition=acquisition)
    assert any(bits(a)[0] != bits(b)[0] for a, b in zip(y_old, y_new)) or refine


@pytest.mark.parametrize("acquisition", ["EI", "LOGEI"])
def test_the_agent_runs_four_trials(lib, acquisition):
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model

    class Toy(ToyGraph):
        manipulative_variables = ("X", "Z")
        _fit_dependencies = (("X",), ("Z",))
        _fit_parameters = ([1.0, 1.0, 10.0, False], [1.0, 1.0, 10.0, False])

    sem = Toy.define_sem()
    rng = np.random.default_rng(11)
    draws = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(60)]
    obs = {v: np.array([r[v] for r in draws]) for v in draws[0] if not v.startswith("U")}
    init = {k: v[:40] for k, v in obs.items()}
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    xs = [rng.uniform(-5, 5, (6, 1)), rng.uniform(-5, 20, (6, 1))]
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=4, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, type_cost=4,
                    acquisition=acquisition, cost_mode="pointwise")
        mon = agent.run()
    assert agent.cost_mode == "pointwise" and len(mon.type_trial) == 4 and 1 in mon.type_trial
    chosen = [c for c in mon.chosen if c is not None]
    assert len(chosen) == sum(mon.type_trial) and all(np.all(np.isfinite(x)) for _, x in chosen)
    # the cost recorded for every intervention is the grid's cost vector at the chosen candidate
    running, costs = 0.0, [0.0]
    for entry in mon.chosen:
        if entry is not None:
            names, x = entry
            s = [list(e) for e in es].index(list(names))
            grid = agent.candidate_grid(s)
            assert getattr(grid, "_cost_key", None) is not None        # (the sweep gave the grid its cost vector)
            vector = get_cost(lib, grid)
            hit = np.flatnonzero(np.all(grid.points == x, axis=1))
            assert hit.size == 1
            running += vector[hit[0]]
        costs.append(running)
    assert mon.current_cost == costs and mon.cumulative_cost == running > 0
