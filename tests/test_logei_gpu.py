"""GPU tests of the log Expected Improvement: cbo_acq_sweep_logei (pointwise_acq_kernel<kLogEiKind>),
cbo_acq_sweep_sets_logei (small_sets_kernel<kLogEiKind>), cbo_acq_refine_sets_logei (small_sets_refine_kernel<kLogEiKind>) and
the Python layers on top.

The accuracy reference is mpmath at 60 digits, formed per candidate from the mean and variance doubles the call itself
returned: log(npdf(u) + u ncdf(u)) + log sd - log cost.  Everything else is exact: the one launch against the per-set calls
on fitted twins, the refinement's value against the one-point sweep, as bit patterns."""
import ctypes
import warnings

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOT_FITTED = -5
PI_KIND = 2
# The accuracy bound (the issue's rule): 4 x the worst scaled error |got - ref| / max(1, |ref|) the first run on an MI355X
# measured against mpmath over every case of test_accuracy_against_mpmath below, capped at 1e-13.  Measured: 1.726e-15
# (n130 d1 m1000, task 'max', y_best = Y.min(), at u = 33032; DESIGN.md §4x has the worst figure per range).
MEASURED_WORST = 1.726e-15
ACCURACY_BOUND = min(4.0 * MEASURED_WORST, 1e-13)


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
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


def sweep_logei(lib, model, grid, y_best, task, jitter, cost, want=True):
    """cbo_acq_sweep_logei: dict(acq, mean, var, best_val, best_idx)."""
    m = len(grid)
    acq, mean, var = (np.empty(m), np.empty(m), np.empty(m)) if want else (None, None, None)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep_logei(model._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                             float(cost), lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                             ctypes.byref(bi)))
    return dict(acq=acq, mean=mean, var=var, best_val=bv.value, best_idx=bi.value)


def mp_log_ei(mean, var, y_best, task, jitter, cost):
    """The reference at 60 digits from the doubles given."""
    with mp.workdps(60):
        out = []
        for m_, v_ in zip(mean, var):
            m_, s = mp.mpf(float(m_)), mp.sqrt(mp.mpf(float(v_)))
            u = (mp.mpf(y_best) - (m_ + mp.mpf(jitter))) / s if task == "min" else ((m_ - mp.mpf(jitter)) - mp.mpf(y_best)) / s
            out.append(mp.log(mp.npdf(u) + u * mp.ncdf(u)) + mp.log(s) - mp.log(mp.mpf(cost)))
        return out


def scaled_error(got, ref):
    with mp.workdps(60):
        return np.array([float(abs(mp.mpf(float(g)) - r) / max(mp.mpf(1), abs(r))) for g, r in zip(got, ref)])


# ------------------------------------------------------------------------------------------------------------ 1. accuracy
# n: less than a 16-row tile, a partial second tile, more than the one-launch kernels take; m: odd sizes around the pass's 512
# candidates per workgroup and more than one workgroup; the noise of the exploration-set models, 1e-10
ACCURACY_SHAPES = {"n12 d1 m257": dict(n=12, d=1, m=257), "n17 d3 ard m63": dict(n=17, d=3, m=63, ard=True),
                   "n130 d1 m1000": dict(n=130, d=1, m=1000), "n12 d1 m257 causal": dict(n=12, d=1, m=257, causal=True)}


class Fitted:
    def __init__(self, n, d, m, ard=False, causal=False):
        from cbo_with_oop_amd import CandidateGrid
        rng = np.random.default_rng(100 * n + d)
        self.X = rng.uniform(-5.0, 5.0 if n < 100 else 20.0, (n, d))
        self.y = np.cos(self.X).sum(1, keepdims=True) - np.exp(-self.X[:, :1] / 20.0)
        kw = dict(variance=1.0, lengthscale=(0.8 + 0.3 * np.arange(d)) if ard else 1.0, ard=ard, noise_var=1e-10)
        if causal:
            kw.update(mean_function=mean_f, variance_adjustment=var_f)
        self.model = gp(self.X, self.y, **kw)
        self.points = rng.uniform(self.X.min(0) - 0.5, self.X.max(0) + 0.5, (m, d))
        self.grid = CandidateGrid(self.points, self.model)

    def close(self):
        self.grid.close()
        self.model.close()


@pytest.fixture(scope="module")
def fitted(lib):
    cases = {name: Fitted(**kw) for name, kw in ACCURACY_SHAPES.items()}
    yield cases
    for c in cases.values():
        c.close()


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("name", list(ACCURACY_SHAPES))
def test_accuracy_against_mpmath(lib, fitted, name, far, task):
    """y_best at Y.min() and at Y.min() - 1e3 (u ~ -1e7 for task 'min': the far range), both tasks -- and for 'max' also the
    mirrored incumbents Y.max() and Y.max() + 1e3, which put ITS u where 'min' has them."""
    c = fitted[name]
    cost, jitter = 2.0, 0.015625
    incumbents = [float(c.y.min()) - (1e3 if far else 0.0)]
    if task == "max":
        incumbents.append(float(c.y.max()) + (1e3 if far else 0.0))
    for y_best in incumbents:
        res = sweep_logei(lib, c.model, c.grid, y_best, task, jitter, cost)
        m = len(c.grid)
        # mean and var: cbo_acq_sweep_kind's bits for the same call
        mean_k, var_k = np.empty(m), np.empty(m)
        lib.check(lib.load().cbo_acq_sweep_kind(c.model._handle, c.grid._handle, PI_KIND, y_best, lib.TASK_CODE[task], jitter,
                                                cost, None, lib.dptr(mean_k), lib.dptr(var_k), None, None))
        assert np.array_equal(bits(res["mean"]), bits(mean_k)) and np.array_equal(bits(res["var"]), bits(var_k))
        assert np.all(np.isfinite(res["acq"]))
        ref = mp_log_ei(res["mean"], res["var"], y_best, task, jitter, cost)
        err = scaled_error(res["acq"], ref)
        worst = int(np.argmax(err))
        u = (y_best - (res["mean"] + jitter)) / np.sqrt(res["var"]) * (1.0 if task == "min" else -1.0)
        print(f"{name} far={far} task={task} y_best={y_best!r}: worst scaled error {err[worst]:.3e} at u = {u[worst]:.6g} "
              f"(u in [{u.min():.4g}, {u.max():.4g}])")
        assert err[worst] <= ACCURACY_BOUND, (err[worst], u[worst])
        assert res["best_idx"] == int(np.argmax(res["acq"])) and bits(res["best_val"])[0] == bits(res["acq"][res["best_idx"]])[0]
        # the outputs are optional: the winner alone is the same winner
        alone = sweep_logei(lib, c.model, c.grid, y_best, task, jitter, cost, want=False)
        assert alone["best_idx"] == res["best_idx"] and bits(alone["best_val"])[0] == bits(res["best_val"])[0]


# ------------------------------------------------------------------------------------------------------------ 2. the dead region
@pytest.fixture(scope="module")
def dead(lib):
    """The recipe of DESIGN.md §4x: 50 points on [-5, 20], hyper-parameters (1, 1, 1e-10), 200 grid points."""
    from cbo_with_oop_amd import CandidateGrid

    class Dead:
        pass
    d = Dead()
    d.X = np.random.default_rng(7).uniform(-5, 20, (50, 1))
    d.y = np.cos(d.X) - np.exp(-d.X / 20)
    d.y_best = float(d.y.min())
    d.model = gp(d.X, d.y, variance=1.0, lengthscale=1.0, noise_var=1e-10)
    d.points = np.linspace(-5, 20, 200)[:, None]
    d.grid = CandidateGrid(d.points, d.model)
    d.lo, d.hi, d.d = np.array([-5.0]), np.array([20.0]), 1
    yield d
    d.grid.close()
    d.model.close()


def test_the_dead_region_is_ordered(lib, dead):
    from cbo_with_oop_amd import CausalExpectedImprovement, CausalLogExpectedImprovement
    ei = CausalExpectedImprovement(dead.y_best, "min", dead.model).sweep(dead.grid, want_acq=True)
    zeros = int(np.sum(ei["acq"] == 0.0))
    print("EI: exact zeros", zeros, "of 200, arg-max", ei["best_idx"])
    assert zeros >= 100                                              # the precondition: most of the grid is dead for the EI
    log = CausalLogExpectedImprovement(dead.y_best, "min", dead.model).sweep(dead.grid, want_acq=True)
    acq = log["acq"][:, 0]
    assert np.all(np.isfinite(acq)) and len(np.unique(acq)) == 200
    print("log EI: range", acq.min(), acq.max(), "arg-max", log["best_idx"])
    assert log["best_idx"] == ei["best_idx"]
    alive = ei["acq"][:, 0] >= 1e-290
    assert alive.any()
    rel = np.abs(np.exp(acq[alive]) - ei["acq"][alive, 0]) / ei["acq"][alive, 0]
    print("exp(log EI) against EI where EI >= 1e-290:", int(alive.sum()), "candidates, worst relative", rel.max())
    assert rel.max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------ 3. one launch
class Pair:
    """One exploration set twice: the model under test (never fitted) with its grid, and the fitted twin with its own."""

    def __init__(self, n, m, d, causal=False, ard=False, offset=0, dtype=None, noise_var=1e-3):
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

    def close(self):
        for o in (self.grid, self.twin_grid, self.model, self.twin):
            o.close()


def sweep_sets_logei(lib, models, grids, y_best, task, jitter, costs):
    s = len(models)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)))
    cs = np.ascontiguousarray(np.broadcast_to(np.asarray(costs, dtype=np.float64), (s,)))
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    lib.check(lib.load().cbo_acq_sweep_sets_logei(s, handles(models), handles(grids), lib.dptr(yb), lib.TASK_CODE[task],
                                                  float(jitter), lib.dptr(cs), lib.dptr(vals), idxs.ctypes.data_as(lib.c_int64_p)))
    return vals, idxs


def per_set(lib, pairs, y_best, task, jitter, costs):
    vals, idxs = np.empty(len(pairs)), np.empty(len(pairs), dtype=np.int64)
    for i, p in enumerate(pairs):
        p.twin.ensure_fitted()
        r = sweep_logei(lib, p.twin, p.twin_grid, y_best[i], task, jitter, costs[i], want=False)
        vals[i], idxs[i] = r["best_val"], r["best_idx"]
    return vals, idxs


# (n, m) in {(1, 1), (16, 63), (17, 257), (128, 200)} x d in {1, 3}, one ARD and one causal set in the mix, an index offset
NINE = [dict(n=1, m=1, d=1), dict(n=16, m=63, d=3), dict(n=17, m=257, d=1, causal=True), dict(n=128, m=200, d=3, ard=True),
        dict(n=1, m=1, d=3), dict(n=16, m=63, d=1, offset=4000), dict(n=17, m=257, d=3), dict(n=128, m=200, d=1),
        dict(n=16, m=63, d=3, causal=True)]


@pytest.fixture(scope="module")
def nine(lib):
    pairs = [Pair(**kw) for kw in NINE]
    yield pairs
    for p in pairs:
        p.close()


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("count", [2, 9])
def test_one_launch_equals_the_per_set_calls(lib, nine, count, task):
    """Two sets (descriptors by value) and nine (read from the pinned array): per set the bits of cbo_acq_sweep_logei on the
    fitted twin; the models under test stay unfitted."""
    pairs = nine[2:4] if count == 2 else nine
    costs = np.array([2.0, 1.0, 0.5] * 3)[:count]
    y_best = np.linspace(-0.6, 0.4, count)
    vals, idxs = sweep_sets_logei(lib, [p.model for p in pairs], [p.grid for p in pairs], y_best, task, 0.01, costs)
    want_v, want_i = per_set(lib, pairs, y_best, task, 0.01, costs)
    print(task, count, "values", vals.tolist(), "indices", idxs.tolist())
    assert np.array_equal(idxs, want_i) and np.array_equal(bits(vals), bits(want_v))
    assert np.all(np.isfinite(vals))
    out = np.empty(1)
    for p in pairs:
        assert p.model.stale and lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == NOT_FITTED


def test_mixed_routing_and_untouched_models(lib, nine):
    """An n = 129 model and an fp32 model take the general path inside the same call and return their own per-set answers; a
    FITTED small model with a cached sweep and a kept solution goes through the launch and is left as it was."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    large, single = Pair(129, 100, 2), Pair(40, 90, 2, dtype="f32", noise_var=1e-2)
    small = nine[1]
    kept_grid = CandidateGrid(small.twin_grid.points, small.twin, keep_solution=True)
    ei = CausalExpectedImprovement(0.1, "min", small.twin)
    before = ei.sweep(kept_grid, cost=1.0, want_acq=True)
    lml_before, lml_after = np.empty(1), np.empty(1)
    assert lib.load().cbo_gp_log_marginal(small.twin._handle, lib.dptr(lml_before)) == 0 and not small.twin.stale
    pairs = [small, large, single, nine[2]]
    models = [small.twin, large.model, single.model, nine[2].model]
    grids = [kept_grid, large.grid, single.grid, nine[2].grid]
    costs, y_best = np.array([2.0, 1.0, 0.5, 2.0]), np.array([0.1, -0.2, 0.3, 0.0])
    vals, idxs = sweep_sets_logei(lib, models, grids, y_best, "min", 0.0, costs)
    want_v, want_i = per_set(lib, pairs, y_best, "min", 0.0, costs)
    print("mixed", vals.tolist(), want_v.tolist(), idxs.tolist(), want_i.tolist())
    assert np.array_equal(idxs, want_i) and np.array_equal(bits(vals), bits(want_v))
    # the small fitted model: fit state, cached q / mu and the kept solution as they were
    assert lib.load().cbo_gp_log_marginal(small.twin._handle, lib.dptr(lml_after)) == 0 and not small.twin.stale
    assert bits(lml_after)[0] == bits(lml_before)[0]
    after = ei.sweep(kept_grid, cost=1.0, want_acq=True)
    assert np.array_equal(bits(before["acq"]), bits(after["acq"])) and before["best_idx"] == after["best_idx"]
    out = np.empty(1)
    assert nine[2].model.stale and lib.load().cbo_gp_log_marginal(nine[2].model._handle, lib.dptr(out)) == NOT_FITTED
    kept_grid.close(); large.close(); single.close()


# ------------------------------------------------------------------------------------------------------------ 4. refinement
class Case:
    """A small well-conditioned set (noise 1e-2): an unfitted model for the launch, a fitted twin for the host class."""

    def __init__(self, n, d, seed=0):
        rng = np.random.default_rng(1000 * n + 10 * d + seed)
        self.lo, self.hi, self.d = np.full(d, -2.0), np.full(d, 2.0), d
        self.X = rng.uniform(self.lo, self.hi, (n, d))
        self.y = np.sin(1.3 * self.X[:, :1]) + 0.3 * (self.X[:, 1:] ** 2).sum(1, keepdims=True) / max(d - 1, 1)
        self.kw = dict(variance=1.2, lengthscale=1.1, noise_var=1e-2)
        self.model, self.twin = gp(self.X, self.y, fit=False, **self.kw), gp(self.X, self.y, **self.kw)
        self.y_best = float(self.y.min()) - 0.5
        self.rng = rng

    def close(self):
        self.model.close()
        self.twin.close()


def refine_logei(lib, cases, starts, costs, y_best, task="min", jitter=0.0, max_rounds=200, sentinel=0.0, kind=None):
    """cbo_acq_refine_sets_logei (kind None) or cbo_acq_refine_sets(kind): (rc, per set (x, val, grad, rounds, status))."""
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
    gps = handles([c.model for c in cases])
    tail = (max_rounds, lib.dptr(x), lib.dptr(v), lib.dptr(g), rounds.ctypes.data_as(lib.c_int_p),
            status.ctypes.data_as(lib.c_int_p))
    if kind is None:
        rc = lib.load().cbo_acq_refine_sets_logei(n, gps, sets, lib.dptr(yb), lib.TASK_CODE[task], jitter, *tail)
    else:
        rc = lib.load().cbo_acq_refine_sets(n, gps, sets, kind, lib.dptr(yb), lib.TASK_CODE[task], jitter, *tail)
    out, r0, o0 = [], 0, 0
    for s in starts:
        k, d = s.shape
        out.append((x[r0:r0 + k * d].reshape(k, d), v[o0:o0 + k], g[r0:r0 + k * d].reshape(k, d), rounds[o0:o0 + k],
                    status[o0:o0 + k]))
        r0, o0 = r0 + k * d, o0 + k
    return rc, out


def one_point_sweep(lib, model, x, cost, y_best, task, jitter):
    from cbo_with_oop_amd import CandidateGrid
    grid = CandidateGrid(np.ascontiguousarray(x[None, :]), model)
    vals, _ = sweep_sets_logei(lib, [model], [grid], y_best, task, jitter, cost)
    grid.close()
    return vals[0]


def point_cost(fix, variable, x):
    from cbo_with_oop_amd.utils_functions.causal_optimizer import one_row_cost
    return one_row_cost(fix, variable, x)


FD_STEP = 2.0 ** -8
FD_ROUNDING = 3.2e-6          # (derived in test_value_and_gradient_at_the_starts' docstring)


def mp_log_ei_at(model, pts, y_best, task, jitter):
    mean, var = model.predict(np.ascontiguousarray(pts))
    return mp_log_ei(mean[:, 0], var[:, 0], y_best, task, jitter, 1.0)


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("n,d,k", [(10, 1, 8), (16, 3, 4)])
def test_value_and_gradient_at_the_starts(lib, n, d, k, task):
    """max_rounds = 0.  The value: bit for bit the sets sweep on a one-point grid there, at the point's own (variable) cost.
    The gradient: within 1e-9 of ``CausalLogExpectedImprovement.evaluate_with_gradients`` relative to the gradient's largest
    component at that start -- and against central differences of the mpmath reference over the twin's predictions.
    The differences' step is h = 2^-8 in every coordinate and their bound has two parts.
    Truncation: D_h - f' = h^2 f3 / 6 + O(h^4) (f3 the third derivative) and D_2h - D_h = 3 (h^2 f3 / 6) + O(h^4), so
    |D_2h - D_h| / 3 estimates it from the same reference; twice that is allowed, for the O(h^4) terms.
    Rounding: the reference is exact in the doubles ``predict`` returns, but those carry the solve's own error, different at
    x + h and x - h.  Ky = K + 1e-2 I with variance 1.2 and n <= 16 has a condition number below 16 x 1.2 / 1e-2 ~ 2e3, so mean
    and q = k*' Ky^-1 k* are good to 2e3 x 1.1e-16 ~ 2e-13 (of |mean| ~ 1 and of kss = 1.2); var >= 1e-2, so sd is good to
    1.3e-11 relative.  With sd >= 0.1 and |u| <= 30 (the incumbent is 0.5 beyond the data's extreme): du <= 2e-13 / 0.1 +
    30 x 1.3e-11 = 4e-10, and d logEI = A du + d sd / sd with A <= 1 + |u| gives 1.2e-8 per value; two values over 2 h = 2^-7:
    FD_ROUNDING = 2 x 1.2e-8 x 2^7 = 3.2e-6 (the gradients themselves are of order 1 to 100)."""
    from cbo_with_oop_amd import CausalLogExpectedImprovement
    c = Case(n, d)
    y_best = c.y_best if task == "min" else float(c.y.max()) + 0.5
    jitter = 0.0078125
    pts = c.rng.uniform(c.lo, c.hi, (k, d))
    cost = (np.ones(d), np.ones(d, dtype=np.int32))                  # fix 1 per variable plus |x|
    rc, ((x, val, grad, rounds, status),) = refine_logei(lib, [c], [pts], [cost], y_best, task, jitter, max_rounds=0)
    lib.check(rc)
    assert np.array_equal(x, pts) and np.all(rounds == 0)
    assert set(status.tolist()) <= {lib.REFINE_PGTOL, lib.REFINE_MAX_ROUNDS}
    for i in range(k):
        price = point_cost(cost[0], cost[1], pts[i])
        assert bits(val[i])[0] == bits(one_point_sweep(lib, c.model, pts[i], price, y_best, task, jitter))[0], (i, pts[i])
    f, df = CausalLogExpectedImprovement(y_best, task, c.twin, jitter).evaluate_with_gradients(pts)
    rel = np.max(np.abs(grad - df), axis=1) / np.max(np.abs(df), axis=1)
    print(f"n{n} d{d} {task}: gradient against the host class, worst relative {rel.max():.3e}; values", val.tolist())
    assert rel.max() <= 1e-9
    price = np.array([point_cost(cost[0], cost[1], p) for p in pts])
    assert np.allclose(val, f[:, 0] - np.log(price), rtol=1e-12, atol=0.0)
    h = FD_STEP
    for j in range(d):
        e = np.zeros(d)
        e[j] = 1.0
        f_p, f_m = mp_log_ei_at(c.twin, pts + h * e, y_best, task, jitter), mp_log_ei_at(c.twin, pts - h * e, y_best, task, jitter)
        f_pp, f_mm = (mp_log_ei_at(c.twin, pts + 2 * h * e, y_best, task, jitter),
                      mp_log_ei_at(c.twin, pts - 2 * h * e, y_best, task, jitter))
        d_h = np.array([float((a - b) / (2 * h)) for a, b in zip(f_p, f_m)])
        d_2h = np.array([float((a - b) / (4 * h)) for a, b in zip(f_pp, f_mm)])
        bound = 2.0 * np.abs(d_2h - d_h) / 3.0 + FD_ROUNDING
        print(f"  coordinate {j}: |grad - D_h| {np.abs(grad[:, j] - d_h).tolist()} bound {bound.tolist()}")
        assert np.all(np.abs(grad[:, j] - d_h) <= bound)
    out = np.empty(1)
    assert c.model.stale and lib.load().cbo_gp_log_marginal(c.model._handle, lib.dptr(out)) == NOT_FITTED
    c.close()


def test_a_start_in_the_dead_region_moves(lib, dead):
    """x = -4.75 of the dead-region model: EI and its gradient are exact zeros there, kind 0 returns the start after 0 rounds
    (the precondition); the log EI has a value and a gradient, and its search climbs."""
    start = np.array([[-4.75]])
    cost = (np.ones(1), np.zeros(1, dtype=np.int32))
    rc, ((x0, v0, g0, r0, s0),) = refine_logei(lib, [dead], [start], [cost], dead.y_best, kind=0)
    lib.check(rc)
    print("EI at the start:", v0.tolist(), g0.tolist(), "rounds", r0.tolist(), "status", s0.tolist())
    assert np.array_equal(x0, start) and r0[0] == 0 and v0[0] == 0.0 and g0[0, 0] == 0.0
    rc, ((_, v_start, g_start, _, _),) = refine_logei(lib, [dead], [start], [cost], dead.y_best, max_rounds=0)
    lib.check(rc)
    rc, ((x, v, g, r, s),) = refine_logei(lib, [dead], [start], [cost], dead.y_best)
    lib.check(rc)
    print("log EI: start", v_start.tolist(), g_start.tolist(), "end", x.tolist(), v.tolist(), "rounds", r.tolist(), "status",
          s.tolist())
    assert np.isfinite(v_start[0]) and g_start[0, 0] != 0.0
    assert x[0, 0] != start[0, 0] and dead.lo[0] <= x[0, 0] <= dead.hi[0] and r[0] > 0
    assert s[0] not in (lib.REFINE_NAN_START, lib.REFINE_DECLINED)
    assert v[0] > v_start[0]
    assert bits(v[0])[0] == bits(one_point_sweep(lib, dead.model, x[0], 1.0, dead.y_best, "min", 0.0))[0]


def test_causal_large_and_fp32_sets_are_declined_and_answered_by_the_host_route(lib):
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import CausalGradientAcquisitionOptimizer, CausalLogExpectedImprovement, Cost
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
    cost = (np.ones(1), np.zeros(1, dtype=np.int32))
    rc, res = refine_logei(lib, sets, starts, [cost] * 4, 0.0, sentinel=-77.0)
    lib.check(rc)
    assert np.all(res[0][4] != lib.REFINE_DECLINED) and np.all(res[0][1] != -77.0)
    for i in (1, 2, 3):
        x, val, grad, rounds, status = res[i]
        assert np.all(status == lib.REFINE_DECLINED)
        assert np.all(x == -77.0) and np.all(val == -77.0) and np.all(grad == -77.0) and np.all(rounds == -77)
    # refine_sets: the eligible set from the launch, the others refine_batched's own on the log quotient
    table = ToyGraph.get_cost_structure(1)
    price = Cost(table, ["X"])
    boxes = [[(-2.0, 2.0)]] * 4
    models = [s.model for s in sets]
    got = refine_sets(models, starts, boxes, 0.0, "min", [price] * 4, kind=("LOGEI", 0.0))
    assert np.array_equal(bits(got[0][0]), bits(res[0][0])) and np.array_equal(bits(got[0][1]), bits(res[0][1]))
    assert np.array_equal(got[0][2], res[0][4])
    for i in (1, 2, 3):
        acq = CausalLogExpectedImprovement(0.0, "min", models[i]) / price
        xs, fs = CausalGradientAcquisitionOptimizer(boxes[i]).refine_batched(acq, starts[i])
        assert np.array_equal(bits(got[i][0]), bits(xs)) and np.array_equal(bits(got[i][1]), bits(fs))
        assert np.all(got[i][2] == lib.REFINE_DECLINED) and np.all(np.isfinite(got[i][1]))
    # optimize(refine=True, device=True) takes the eligible set and refuses the causal one
    opt = CausalGradientAcquisitionOptimizer(boxes[0], grid_shape=[40])
    x0, f0 = opt.optimize(CausalLogExpectedImprovement(0.0, "min", models[0]) / price)
    x1, f1 = opt.optimize(CausalLogExpectedImprovement(0.0, "min", models[0]) / price, refine=True, num_starts=4, device=True)
    assert f1[0, 0] >= f0[0, 0] and -2.0 <= x1[0, 0] <= 2.0
    with pytest.raises(ValueError, match="device=True"):
        CausalGradientAcquisitionOptimizer(boxes[1], grid_shape=[40]).optimize(
            CausalLogExpectedImprovement(0.0, "min", models[1]) / price, refine=True, device=True)
    for s in sets:
        s.model.close()


# ------------------------------------------------------------------------------------------------------------ 5. Python surface
@pytest.mark.parametrize("refine", [False, True])
def test_find_next_y_points_on_the_toy_graph(lib, refine):
    """Per set the returned value is the class's evaluate at the returned point over that point's cost (the logarithm of the
    quotient: the quotient object's evaluate, bit for bit), and the chosen set is the arg-max of the per-set values."""
    from cbo_with_oop_amd import CBOAcquisitionPath, CausalLogExpectedImprovement, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import Cost, find_next_y_points
    rng = np.random.default_rng(3)
    es = ToyGraph.get_exploration_set("MIS")
    xs = [rng.uniform(-5, 5, (20, 1)), rng.uniform(-5, 20, (50, 1))]
    ys = [ToyGraph.target_do_x(xs[0]), ToyGraph.target_do_z(xs[1])]
    table = ToyGraph.get_cost_structure(4)                          # 1 + |x|: the winner is re-priced at its own cost
    spaces = [ToyGraph.bounds(s) for s in es]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys, spaces, grid_shapes=[[200], [200]],
                              comm=None, acquisition="LOGEI", refine=refine)
    path.update_all_gaussian_processes()
    incumbent = min(float(ys[0].min()), float(ys[1].min()))
    grids = [path.candidate_grid(s) for s in range(2)]
    kw = dict(refine=True, spaces=spaces) if refine else {}
    x_new, y_new = find_next_y_points(path.models, incumbent, es, table, "min", grids, acquisition="LOGEI", **kw)
    values = []
    for s in range(2):
        quotient = CausalLogExpectedImprovement(incumbent, "min", path.models[s]) / Cost(table, es[s])
        again = quotient.evaluate(x_new[s])
        plain = CausalLogExpectedImprovement(incumbent, "min", path.models[s]).evaluate(x_new[s])
        c = float(Cost(table, es[s]).evaluate(x_new[s]))
        print("set", s, "x", x_new[s].tolist(), "value", y_new[s].tolist(), "cost", c)
        assert x_new[s].shape == (1, 1) and y_new[s].shape == (1, 1) and np.isfinite(y_new[s][0, 0])
        if refine:
            # (a refined value may be the host route's: numpy's restatement from ``predict``, not the device's own bits)
            assert abs(y_new[s][0, 0] - again[0, 0]) <= 1e-9 * max(1.0, abs(again[0, 0]))
        else:
            assert bits(y_new[s])[0] == bits(again)[0]
        assert abs(y_new[s][0, 0] - (plain[0, 0] - np.log(c))) <= 1e-9 * max(1.0, abs(y_new[s][0, 0]))
        if not refine:
            assert np.any(np.all(grids[s].points == x_new[s], axis=1))
        values.append(y_new[s][0, 0])
    # the path's own call is the same call, and the pick the arg-max
    x_path, y_path = path.compute_best_acquisition_values(incumbent)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(y_path, y_new))
    assert all(np.array_equal(a, b) for a, b in zip(x_path, x_new))
    assert path.select_next_intervention(y_new)[1] == int(np.argmax(values))


def test_the_agent_runs_four_trials(lib):
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model

    class Toy(ToyGraph):
        """The toy graph with what an observe step needs: its manipulative variables and one graph GP per set."""
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
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, acquisition="LOGEI")
        mon = agent.run()
    assert len(mon.type_trial) == 4 and 1 in mon.type_trial
    chosen = [c for c in mon.chosen if c is not None]
    assert len(chosen) == sum(mon.type_trial) and all(np.all(np.isfinite(x)) for _, x in chosen)
    assert np.all(np.isfinite(mon.global_opt)) and np.all(np.isfinite(mon.current_cost)) and mon.cumulative_cost > 0
    assert sum(x.shape[0] for x in agent.data_x) == 12 + len(chosen)
