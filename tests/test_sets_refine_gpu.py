"""GPU tests of the gradient refinement of every set's starts in one launch: cbo_acq_refine_sets
(small_sets_refine_kernel, kernels_sets_refine.hip) and the Python layers on top.

Shapes are the smallest at which the kernel can go wrong: n in {10, 16, 50, 128} (less than one 16-row tile, exactly one, a
partial last tile, the cap), d in {1, 2, 3, 8} (a start fills 1 + d of a wave's 16 columns: 9 at d = 8) and one ARD model
with the graph_ard_d4 fixture's hyper-parameters (d = 4), k in {1, 4, one more than a workgroup carries at that d}, 1, 3 and
9 sets (nine exceeds the eight descriptors that travel by value), noise 1e-3.  References: the numpy oracle's
expected_improvement_with_gradients over the point's cost at the bars of tests/test_parity_gpu.py's host-route check (value
rtol 1e-6 / atol 1e-12, gradient rtol 1e-5 / atol 1e-10), the host classes' evaluate_with_gradients for the point-wise
kinds at the same bars, and -- bit for bit -- the multi-set sweep on a one-point grid."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import load_fixture
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOT_FITTED = -5
VARIANCE, LENGTHSCALE, NOISE = 1.2, 1.1, 1e-3
VALUE_BAR = dict(rtol=1e-6, atol=1e-12)
GRAD_BAR = dict(rtol=1e-5, atol=1e-10)


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


class Case:
    """One exploration set: data, an UNFITTED device model (the launch works from resident data), the oracle's posterior."""

    def __init__(self, n, d, seed=0, ard=False, lo=-2.0, hi=2.0):
        from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
        rng = np.random.default_rng(1000 * n + 10 * d + seed)
        if ard:
            f = load_fixture("graph_ard_d4")
            self.X, self.y = np.ascontiguousarray(f["X"][:n]), np.ascontiguousarray(f["y"][:n])
            d = self.X.shape[1]
            self.hyper = dict(variance=float(f["variance"]), lengthscale=f["lengthscale"].copy(), noise_var=float(f["noise_var"]))
            self.lo, self.hi = self.X.min(0) - 0.25, self.X.max(0) + 0.25
        else:
            self.lo, self.hi = np.full(d, float(lo)), np.full(d, float(hi))
            self.X = rng.uniform(self.lo, self.hi, (n, d))
            self.y = (np.sin(1.3 * self.X[:, :1]) + 0.3 * (self.X[:, 1:] ** 2).sum(1, keepdims=True) / max(d - 1, 1)
                      + 0.03 * rng.standard_normal((n, 1)))
            self.hyper = dict(variance=VARIANCE, lengthscale=LENGTHSCALE, noise_var=NOISE)
        self.n, self.d, self.ard, self.rng = n, d, ard, rng
        self.y_best = float(self.y.min()) + 0.1
        self.kw = dict(self.hyper, ard=ard)
        self.model = HipGaussianProcess(self.X, self.y, fit=False, **self.kw)
        self._post = self._twin = None

    @property
    def post(self):
        if self._post is None:
            self._post = O.fit(self.X, self.y, **self.hyper)
        return self._post

    @property
    def twin(self):
        """A fitted model on the same data, for the host classes."""
        from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
        if self._twin is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                self._twin = HipGaussianProcess(self.X, self.y, **self.kw)
        return self._twin

    @property
    def per_block(self):
        return 4 * (16 // (1 + self.d))

    def points(self, k):
        """k points in the box: random ones and, from the second on, every other one a point of a regular grid."""
        pts = self.rng.uniform(self.lo, self.hi, (k, self.d))
        grid = np.linspace(self.lo, self.hi, 5)                      # (5, d): per-dimension grid values
        for i in range(1, k, 2):
            pts[i] = grid[self.rng.integers(0, 5, self.d), np.arange(self.d)]
        return pts

    def close(self):
        self.model.close()
        if self._twin is not None:
            self._twin.close()


SHAPES = {"n10 d1": dict(n=10, d=1), "n16 d2": dict(n=16, d=2), "n50 d3": dict(n=50, d=3), "n128 d8": dict(n=128, d=8),
          "n50 d2": dict(n=50, d=2), "n128 d1": dict(n=128, d=1), "ard n50 d4": dict(n=50, d=4, ard=True)}


@pytest.fixture(scope="module")
def zoo(lib):
    cases = {name: Case(**kw) for name, kw in SHAPES.items()}
    yield cases
    for c in cases.values():
        c.close()


def costs_of(case, variable):
    fix = np.ones(case.d) if variable else 1.0 + np.arange(case.d, dtype=np.float64)
    return fix, np.full(case.d, 1 if variable else 0, dtype=np.int32)


def point_cost(fix, variable, x):
    from cbo_with_oop_amd.utils_functions.causal_optimizer import one_row_cost
    return one_row_cost(fix, variable, x)


def refine_call(lib, cases, starts, costs, kind="EI", y_best=None, task="min", param=0.0, max_rounds=200, boxes=None,
                sentinel=None):
    """cbo_acq_refine_sets itself: (rc, per set (x, val, grad, rounds, status)).  ``sentinel`` pre-fills the outputs."""
    n = len(cases)
    starts = [np.ascontiguousarray(s, dtype=np.float64) for s in starts]
    boxes = boxes or [(c.lo, c.hi) for c in cases]
    keep = []
    sets = (lib.CboRefineSet * n)()
    for j, c in enumerate(cases):
        lo, hi = (np.ascontiguousarray(b, dtype=np.float64) for b in boxes[j])
        fix, variable = costs[j]
        fix, variable = np.ascontiguousarray(fix, dtype=np.float64), np.ascontiguousarray(variable, dtype=np.int32)
        keep += [lo, hi, fix, variable]
        sets[j].k = starts[j].shape[0]
        sets[j].starts = starts[j].ctypes.data_as(lib.c_double_p)
        sets[j].lo, sets[j].hi = lo.ctypes.data_as(lib.c_double_p), hi.ctypes.data_as(lib.c_double_p)
        sets[j].cost_fix = fix.ctypes.data_as(lib.c_double_p)
        sets[j].cost_variable = variable.ctypes.data_as(lib.c_int_p)
    rows, total = sum(s.size for s in starts), sum(s.shape[0] for s in starts)
    fill = 0.0 if sentinel is None else sentinel
    x, g, v = np.full(rows, fill), np.full(rows, fill), np.full(total, fill)
    rounds, status = np.full(total, int(fill), dtype=np.int32), np.full(total, int(fill), dtype=np.int32)
    yb = np.array([c.y_best for c in cases] if y_best is None else y_best, dtype=np.float64)
    gps = (ctypes.c_void_p * n)(*[c.model._handle for c in cases])
    rc = lib.load().cbo_acq_refine_sets(n, gps, sets, lib.REFINE_KIND_CODE[kind], lib.dptr(yb), lib.TASK_CODE[task], param,
                                        max_rounds, lib.dptr(x), lib.dptr(v), lib.dptr(g),
                                        rounds.ctypes.data_as(lib.c_int_p), status.ctypes.data_as(lib.c_int_p))
    out, r0, o0 = [], 0, 0
    for s in starts:
        k, d = s.shape
        out.append((x[r0:r0 + k * d].reshape(k, d), v[o0:o0 + k], g[r0:r0 + k * d].reshape(k, d), rounds[o0:o0 + k],
                    status[o0:o0 + k]))
        r0, o0 = r0 + k * d, o0 + k
    return rc, out


def one_point_sweep(lib, case, x, cost, kind="EI", task="min", param=0.0, y_best=None):
    """The multi-set sweep's value for the one-point grid {x}: cbo_acq_sweep_sets (_kind)."""
    from cbo_with_oop_amd.utils_functions import CandidateGrid
    grid = CandidateGrid(np.ascontiguousarray(x[None, :]), case.model)
    gps, cds = (ctypes.c_void_p * 1)(case.model._handle), (ctypes.c_void_p * 1)(grid._handle)
    yb, c = np.array([case.y_best if y_best is None else y_best]), np.array([float(cost)])
    val, idx = np.zeros(1), np.zeros(1, dtype=np.int64)
    if kind == "EI":
        rc = lib.load().cbo_acq_sweep_sets(1, gps, cds, lib.dptr(yb), lib.TASK_CODE[task], param, lib.dptr(c), lib.dptr(val),
                                           idx.ctypes.data_as(lib.c_int64_p))
    else:
        rc = lib.load().cbo_acq_sweep_sets_kind(1, gps, cds, lib.ACQ_KIND_CODE[kind], lib.dptr(yb), lib.TASK_CODE[task],
                                                param, lib.dptr(c), lib.dptr(val), idx.ctypes.data_as(lib.c_int64_p))
    grid.close()
    lib.check(rc)
    return val[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def projected(x, grad, lo, hi):
    """The gradient of the maximised function with what points out of the box at an active bound put to zero."""
    return np.where(((x >= hi) & (grad > 0)) | ((x <= lo) & (grad < 0)), 0.0, grad)


# ---------------------------------------------------------------------------------------------- 1. values and gradients
@pytest.mark.parametrize("variable", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_ei_values_and_gradients_at_the_starts(lib, zoo, name, variable):
    """max_rounds = 0 at random and grid points, k one more than a workgroup carries: the oracle's EI and gradient over the
    point's cost; the value bit for bit the one-point sweep's, under a fixed and under a variable cost."""
    c = zoo[name]
    k = c.per_block + 1
    pts = c.points(k)
    cost = costs_of(c, variable)
    rc, ((x, val, grad, rounds, status),) = refine_call(lib, [c], [pts], [cost], max_rounds=0)
    lib.check(rc)
    assert np.array_equal(x, pts) and np.all(rounds == 0)
    assert set(status.tolist()) <= {lib.REFINE_PGTOL, lib.REFINE_MAX_ROUNDS}
    price = np.array([point_cost(cost[0], cost[1], p) for p in pts])
    fo, dfo = O.expected_improvement_with_gradients(c.post, pts, c.y_best)
    print(name, "value rel", np.max(np.abs(val - fo[:, 0] / price) / np.maximum(np.abs(fo[:, 0] / price), 1e-300)),
          "grad abs", np.max(np.abs(grad - dfo / price[:, None])))
    assert np.allclose(val, fo[:, 0] / price, **VALUE_BAR)
    assert np.allclose(grad, dfo / price[:, None], **GRAD_BAR)
    for i in range(k):
        assert bits(val[i]) == bits(one_point_sweep(lib, c, pts[i], price[i])), (i, pts[i])
    out = np.empty(1)
    assert c.model.stale and lib.load().cbo_gp_log_marginal(c.model._handle, lib.dptr(out)) == NOT_FITTED


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("kind", ["LCB", "PI", "VAR", "MPEI"])
def test_pointwise_kinds_against_the_host_classes(lib, zoo, kind, task):
    from cbo_with_oop_amd.utils_functions import pointwise_acquisitions as pw
    for name in ("n16 d2", "n50 d3", "ard n50 d4"):
        c = zoo[name]
        param = {"LCB": 1.7, "PI": 0.01, "VAR": 0.0, "MPEI": 0.01}[kind]
        host = {"LCB": lambda: pw.CausalNegativeLowerConfidenceBound(task, c.twin, param),
                "PI": lambda: pw.CausalProbabilityOfImprovement(c.y_best, task, c.twin, param),
                "VAR": lambda: pw.ModelVariance(c.twin),
                "MPEI": lambda: pw.CausalMeanPluginExpectedImprovement(task, c.twin, param)}[kind]()
        pts = c.points(5)
        cost = costs_of(c, True)
        rc, ((x, val, grad, _, _),) = refine_call(lib, [c], [pts], [cost], kind=kind, task=task, param=param, max_rounds=0)
        lib.check(rc)
        price = np.array([point_cost(cost[0], cost[1], p) for p in pts])
        f, df = host.evaluate_with_gradients(pts)
        assert np.allclose(val, f[:, 0] / price, **VALUE_BAR), (name, val, f[:, 0] / price)
        assert np.allclose(grad, df / price[:, None], **GRAD_BAR), (name, grad, df / price[:, None])
        for i in range(5):
            assert bits(val[i]) == bits(one_point_sweep(lib, c, pts[i], price[i], kind=kind, task=task, param=param))


# ---------------------------------------------------------------------------------------------- 2. after refinement
def check_refined(lib, c, starts, cost, res, res0, kind="EI", task="min", param=0.0, max_rounds=200):
    x, val, grad, rounds, status = res
    assert np.all(val >= res0[1]), (val, res0[1])                  # never below the start's own value
    assert np.all(x >= c.lo) and np.all(x <= c.hi)
    valid = {lib.REFINE_PGTOL, lib.REFINE_FTOL, lib.REFINE_STEP, lib.REFINE_MAX_ROUNDS}
    assert set(status.tolist()) <= valid and np.all(rounds <= max_rounds) and np.all(rounds >= 0)
    for i in range(len(x)):
        price = point_cost(cost[0], cost[1], x[i])
        assert bits(val[i]) == bits(one_point_sweep(lib, c, x[i], price, kind=kind, task=task, param=param)), i
        if status[i] == lib.REFINE_PGTOL:
            assert np.max(np.abs(projected(x[i], grad[i], c.lo, c.hi))) <= 1e-5
    rc, (again,) = refine_call(lib, [c], [x], [cost], kind=kind, task=task, param=param, max_rounds=0)
    lib.check(rc)
    assert np.array_equal(bits(again[2]), bits(grad)) and np.array_equal(bits(again[1]), bits(val))


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_start_ends_no_lower_inside_the_box_at_a_point_the_sweep_prices_the_same(lib, zoo, name):
    c = zoo[name]
    seen = set()
    for k, variable in ((1, False), (4, True), (c.per_block + 1, False)):
        starts = c.points(k)
        cost = costs_of(c, variable)
        rc, (res0,) = refine_call(lib, [c], [starts], [cost], max_rounds=0)
        lib.check(rc)
        rc, (res,) = refine_call(lib, [c], [starts], [cost])
        lib.check(rc)
        check_refined(lib, c, starts, cost, res, res0)
        rc, (twice,) = refine_call(lib, [c], [starts], [cost])
        lib.check(rc)
        for a, b in zip(res, twice):                                # a second identical call: the same bits everywhere
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        seen |= set(res[4].tolist())
        print(name, k, "rounds", res[3].tolist(), "status", res[4].tolist())
    assert lib.REFINE_PGTOL in seen or lib.REFINE_FTOL in seen      # (somebody converged: the searches are searches)
    # a round budget that runs out says so
    rc, (short,) = refine_call(lib, [c], [c.points(4)], [costs_of(c, False)], max_rounds=1)
    lib.check(rc)
    assert np.all(short[3] <= 1) and np.all((short[4] != lib.REFINE_MAX_ROUNDS) | (short[3] == 1))


@pytest.mark.parametrize("kind,task", [("LCB", "max"), ("PI", "min"), ("VAR", "min"), ("MPEI", "min")])
def test_the_pointwise_kinds_refine_too(lib, zoo, kind, task):
    c = zoo["n50 d2"]
    param = {"LCB": 1.7, "PI": 0.01, "VAR": 0.0, "MPEI": 0.01}[kind]
    starts, cost = c.points(4), costs_of(c, True)
    rc, (res0,) = refine_call(lib, [c], [starts], [cost], kind=kind, task=task, param=param, max_rounds=0)
    lib.check(rc)
    rc, (res,) = refine_call(lib, [c], [starts], [cost], kind=kind, task=task, param=param)
    lib.check(rc)
    check_refined(lib, c, starts, cost, res, res0, kind=kind, task=task, param=param)


@pytest.mark.parametrize("count", [3, 9])
def test_several_sets_in_one_call_are_the_single_set_calls(lib, zoo, count):
    """Three sets (descriptors by value) and nine (read from the pinned array), mixed n, d and k: per set the bits of the
    set's own call, evaluated at the starts and refined."""
    names = list(SHAPES)
    cases = [zoo[names[i % len(names)]] for i in range(count)]
    ks = [(1, 4, c.per_block + 1)[i % 3] for i, c in enumerate(cases)]
    starts = [c.points(k) for c, k in zip(cases, ks)]
    costs = [costs_of(c, i % 2 == 1) for i, c in enumerate(cases)]
    for max_rounds in (0, 200):
        rc, together = refine_call(lib, cases, starts, costs, max_rounds=max_rounds)
        lib.check(rc)
        for i, c in enumerate(cases):
            rc, (alone,) = refine_call(lib, [c], [starts[i]], [costs[i]], max_rounds=max_rounds)
            lib.check(rc)
            for a, b in zip(together[i], alone):
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), i


# ---------------------------------------------------------------------------------------------- 3. d = 1 against lockstep_lbfgs
@pytest.mark.parametrize("n,lo,hi", [(50, -5.0, 5.0), (16, -5.0, 20.0)])
def test_one_dimensional_sets_end_where_lockstep_lbfgs_ends(lib, n, lo, hi):
    """The in-kernel searches against lockstep_lbfgs driven on the host by the max_rounds = 0 entry, from the four best of
    200 grid points: the values agree to rtol 1e-5 (tests/test_parity_gpu.py's bar for a refined value)."""
    from cbo_with_oop_amd.utils_functions.causal_optimizer import lockstep_lbfgs
    c = Case(n, 1, seed=3, lo=lo, hi=hi)
    cost = costs_of(c, False)

    def fun(X):
        rc, ((_, val, grad, _, _),) = refine_call(lib, [c], [X], [cost], max_rounds=0)
        lib.check(rc)
        return val.copy(), grad.copy()

    grid = np.linspace(lo, hi, 200)[:, None]
    acq = np.concatenate([fun(grid[i:i + 50])[0] for i in range(0, 200, 50)])
    starts = grid[np.argsort(-acq, kind="stable")[:4]]
    X, F = lockstep_lbfgs(fun, starts, c.lo, c.hi)
    rc, ((x, val, _, rounds, status),) = refine_call(lib, [c], [starts], [cost])
    lib.check(rc)
    print("n", n, "kernel", val.tolist(), "host", F.tolist(), "rounds", rounds.tolist(), "status", status.tolist())
    assert np.allclose(val, F, rtol=1e-5, atol=0.0)
    c.close()


# ---------------------------------------------------------------------------------------------- 4. an active bound
@pytest.mark.parametrize("d", [1, 2])
def test_a_start_at_a_corner_whose_ascent_points_outward_stays_there(lib, d):
    """Targets that fall towards the corner (-1, ..): the EI of a minimisation rises towards it, the box ends there."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    c = Case(50, d, seed=4, lo=-3.0, hi=3.0)
    c.model.close()
    c.y = c.X.sum(1, keepdims=True) + 0.01 * c.rng.standard_normal((50, 1))
    c.model = HipGaussianProcess(c.X, c.y, fit=False, **c.kw)
    c.y_best = 0.0
    c.lo, c.hi = np.full(d, -1.0), np.full(d, 1.0)
    corner = c.lo[None, :].copy()
    cost = costs_of(c, False)
    rc, ((_, val0, grad0, _, _),) = refine_call(lib, [c], [corner], [cost], max_rounds=0)
    lib.check(rc)
    assert np.all(grad0 < 0.0), grad0                              # the premise: ascent leaves the box in every coordinate
    rc, ((x, val, grad, rounds, status),) = refine_call(lib, [c], [corner], [cost])
    lib.check(rc)
    assert np.array_equal(x, corner) and bits(val[0]) == bits(val0[0])
    assert status[0] in (lib.REFINE_PGTOL, lib.REFINE_STEP)
    c.close()


# ---------------------------------------------------------------------------------------------- 5. a mixed list
def test_a_mixed_list_declines_what_the_kernel_cannot_take(lib, zoo):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions import CandidateGrid, CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    small = zoo["n16 d2"]
    f = load_fixture("causal_d2")
    lut_m = {tuple(r): v for r, v in zip(map(tuple, f["X"]), f["mX"][:, 0])}
    lut_v = {tuple(r): v for r, v in zip(map(tuple, f["X"]), f["vX"][:, 0])}
    # prior closures defined everywhere (a search moves): the fixture's values at its points, a smooth function elsewhere
    mean_fn = lambda a: np.array([[lut_m.get(tuple(r), 0.1 * np.sin(r).sum())] for r in a])                  # noqa: E731
    var_fn = lambda a: np.array([[lut_v.get(tuple(r), 0.5 + 0.1 * np.cos(r).sum() ** 2)] for r in a])      # noqa: E731

    class Holder:
        pass
    causal, large = Holder(), Holder()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        causal.model = HipGaussianProcess(f["X"], f["y"], variance=float(f["variance"]), lengthscale=f["lengthscale_arg"],
                                          noise_var=1e-3, mean_function=mean_fn, variance_adjustment=var_fn)
        rng = np.random.default_rng(21)
        Xl = rng.uniform([-5, -5], [4, 5], (150, 2))
        yl = np.sin(Xl[:, :1]) + 0.1 * Xl[:, 1:] ** 2 + 0.05 * rng.standard_normal((150, 1))
        large.model = HipGaussianProcess(Xl, yl, variance=1.2, lengthscale=1.1, noise_var=1e-3)
    causal.lo, causal.hi, causal.y_best, causal.d = f["X"].min(0), f["X"].max(0), float(f["y"].min()), 2
    large.lo, large.hi, large.y_best, large.d = np.array([-5.0, -5.0]), np.array([4.0, 5.0]), float(yl.min()), 2
    # the same small set twice: once as an unfitted model, once as its FITTED twin with a kept solution -- the fitted
    # state and the kept V = L^-1 K* of a model that goes through the launch are what the call must leave alone
    fitted = Holder()
    fitted.model, fitted.lo, fitted.hi, fitted.y_best, fitted.d = small.twin, small.lo, small.hi, small.y_best, small.d
    cases = [small, causal, large, fitted]
    pts = small.points(4)
    starts = [pts, rng.uniform(causal.lo, causal.hi, (3, 2)), rng.uniform(large.lo, large.hi, (5, 2)), pts]
    costs = [costs_of(c, False) for c in cases]
    grid = CandidateGrid(small.points(40), fitted.model, keep_solution=True)
    ei = CausalExpectedImprovement(0.1, "min", fitted.model)
    before = ei.sweep(grid, cost=1.0, want_acq=True)
    out, lml_before, lml_after = np.empty(1), np.empty(1), np.empty(1)
    assert lib.load().cbo_gp_log_marginal(small.model._handle, lib.dptr(out)) == NOT_FITTED
    assert lib.load().cbo_gp_log_marginal(fitted.model._handle, lib.dptr(lml_before)) == 0 and not fitted.model.stale
    rc, res = refine_call(lib, cases, starts, costs, y_best=[0.1, 0.1, 0.1, 0.1], sentinel=-77.0)
    lib.check(rc)
    for i in (0, 3):
        assert np.all(res[i][4] != lib.REFINE_DECLINED) and np.all(res[i][1] != -77.0) and np.all(res[i][3] >= 0)
    for a, b in zip(res[0], res[3]):                                # fitted or not: the launch works from the resident data
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    for i in (1, 2):
        x, val, grad, rounds, status = res[i]
        assert np.all(status == lib.REFINE_DECLINED)
        assert np.all(x == -77.0) and np.all(val == -77.0) and np.all(grad == -77.0) and np.all(rounds == -77)
    assert lib.load().cbo_gp_log_marginal(small.model._handle, lib.dptr(out)) == NOT_FITTED and small.model.stale
    assert lib.load().cbo_gp_log_marginal(fitted.model._handle, lib.dptr(lml_after)) == 0 and not fitted.model.stale
    assert bits(lml_after)[0] == bits(lml_before)[0]
    after = ei.sweep(grid, cost=1.0, want_acq=True)                 # (re-scored from the kept solution and the cached q, mu)
    assert np.array_equal(bits(before["acq"]), bits(after["acq"])) and before["best_idx"] == after["best_idx"]
    assert bits(before["best_val"])[0] == bits(after["best_val"])[0]
    grid.close()
    cases, starts = cases[:3], starts[:3]
    # refine_sets: the eligible set from the launch, the other two exactly refine_batched's own
    table = CompleteGraph.get_cost_structure(2)
    names = ["B", "D"]
    cost = Cost(table, names)
    boxes = [list(zip(c.lo.tolist(), c.hi.tolist())) for c in cases]
    models = [c.model for c in cases]
    got = refine_sets(models, starts, boxes, 0.1, "min", [cost] * 3)
    fix = np.array([float(table[v].args[0]) for v in names])
    rc, (direct,) = refine_call(lib, [small], [starts[0]], [(fix, np.zeros(2, dtype=np.int32))], y_best=[0.1])
    lib.check(rc)
    assert np.array_equal(bits(got[0][0]), bits(direct[0])) and np.array_equal(bits(got[0][1]), bits(direct[1]))
    assert np.array_equal(got[0][2], direct[4])
    for i in (1, 2):
        acq = CausalExpectedImprovement(0.1, "min", models[i]) / cost
        xs, fs = CausalGradientAcquisitionOptimizer(boxes[i]).refine_batched(acq, starts[i])
        assert np.array_equal(bits(got[i][0]), bits(xs)) and np.array_equal(bits(got[i][1]), bits(fs))
        assert np.all(got[i][2] == lib.REFINE_DECLINED)
    # optimize(device=True): the one-set call for an eligible set, ValueError for the others
    opt = CausalGradientAcquisitionOptimizer(boxes[0], grid_shape=[12, 12])
    small_acq = CausalExpectedImprovement(0.1, "min", small.twin) / cost
    x0, f0 = opt.optimize(small_acq)
    x1, f1 = opt.optimize(small_acq, refine=True, num_starts=4, device=True)
    assert f1[0, 0] >= f0[0, 0] and np.all(x1[0] >= small.lo) and np.all(x1[0] <= small.hi)
    for i in (1, 2):
        with pytest.raises(ValueError, match="device=True"):
            CausalGradientAcquisitionOptimizer(boxes[i], grid_shape=[8, 8]).optimize(
                CausalExpectedImprovement(0.1, "min", models[i]) / cost, refine=True, device=True)
    with pytest.raises(ValueError, match="device=True"):
        opt.optimize(CausalExpectedImprovement(0.1, "min", small.twin) / Cost({"B": lambda col: 1.0, "D": lambda col: 2.0}, names),
                     refine=True, device=True)
    causal.model.close(); large.model.close()


def test_a_set_that_declines_in_the_launch_is_declined_between_its_neighbours(lib, zoo):
    """The jitter fixture (duplicate rows under a negative noise: the launch's pivot at the duplicate is about -2e-9, far
    below rounding, so it declines there) between two ordinary small sets.  This call has no general path: every start of
    the declined set comes back CBO_REFINE_DECLINED with its other entries untouched, no model is fitted, the neighbours'
    outputs are their own calls' bit for bit; the same call again and the neighbours alone right after give the same bits."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("jitter_ladder")

    class Holder:
        pass
    ladder = Holder()
    ladder.model = HipGaussianProcess(f["X"], f["y"], fit=False, variance=float(f["variance"]),
                                      lengthscale=f["lengthscale_arg"], noise_var=float(f["noise_var"]))
    ladder.lo, ladder.hi, ladder.y_best, ladder.d = np.array([-1.0]), np.array([1.0]), float(f["y_best"]), 1
    first, last = zoo["n10 d1"], zoo["n16 d2"]
    cases = [first, ladder, last]
    starts = [first.points(4), np.ascontiguousarray(f["Xs"][::21]), last.points(4)]
    costs = [costs_of(c, i == 2) for i, c in enumerate(cases)]
    alone = []
    for i in (0, 2):
        rc, (res,) = refine_call(lib, [cases[i]], [starts[i]], [costs[i]], sentinel=-77.0)
        lib.check(rc)
        alone.append(res)
    same = lambda a, b: all(np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))  # noqa: E731
                            for u, v in zip(a, b))
    out = np.empty(1)
    for attempt in ("the call", "the same call again"):
        rc, res = refine_call(lib, cases, starts, costs, sentinel=-77.0)
        lib.check(rc)
        x, val, grad, rounds, status = res[1]
        print(attempt, "ladder status", status.tolist(), "neighbours", res[0][4].tolist(), res[2][4].tolist())
        assert np.all(status == lib.REFINE_DECLINED)
        assert np.all(x == -77.0) and np.all(val == -77.0) and np.all(grad == -77.0) and np.all(rounds == -77)
        assert same(res[0], alone[0]) and same(res[2], alone[1]), attempt
        assert np.all(res[0][4] != lib.REFINE_DECLINED) and np.all(res[2][4] != lib.REFINE_DECLINED)
        for c in cases:                                             # the models are only read: nobody was fitted
            assert lib.load().cbo_gp_log_marginal(c.model._handle, lib.dptr(out)) == NOT_FITTED
    rc, res = refine_call(lib, cases[::2], starts[::2], costs[::2], sentinel=-77.0)
    lib.check(rc)
    assert same(res[0], alone[0]) and same(res[1], alone[1]), "the neighbours alone, right after"
    ladder.model.close()


def test_refine_sets_completes_the_kind_and_can_leave_the_host_route_out(lib, zoo):
    """A ``None`` parameter is the kind's default (beta 1) on the device as it is on the host; ``host_fallback=False`` leaves
    a set the launch does not take unrefined; ``optimize(device=True)`` carries a jittered EI's jitter to the launch."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    c = zoo["n16 d2"]
    cost = Cost(CompleteGraph.get_cost_structure(4), ["B", "D"])
    box = list(zip(c.lo.tolist(), c.hi.tolist()))
    starts = c.points(4)
    (x0, f0, s0), = refine_sets([c.model], [starts], [box], 0.1, "max", [cost], kind=("LCB", None))
    (x1, f1, s1), = refine_sets([c.model], [starts], [box], 0.1, "max", [cost], kind=("LCB", 1.0))
    (x2, f2, _), = refine_sets([c.model], [starts], [box], 0.1, "max", [cost], kind=("LCB", 0.0))
    assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(f0), bits(f1)) and np.array_equal(s0, s1)
    assert not np.array_equal(bits(f0), bits(f2))
    with pytest.raises(ValueError):
        refine_sets([c.model], [starts], [box], 0.1, "max", [cost], kind=("LCB", -1.0))
    with pytest.raises(ValueError):
        refine_sets([c.model], [starts], [box], 0.1, "min", [cost], kind=("EI", np.nan))
    rng = np.random.default_rng(2)
    Xl = rng.uniform(c.lo, c.hi, (150, 2))
    large = HipGaussianProcess(Xl, np.sin(Xl[:, :1]) + 0.05 * rng.standard_normal((150, 1)), variance=1.2, lengthscale=1.1,
                               noise_var=1e-3, fit=False)
    got = refine_sets([c.model, large], [starts, starts], [box, box], 0.1, "min", [cost, cost], host_fallback=False)
    assert np.all(got[0][2] != lib.REFINE_DECLINED) and np.all(np.isfinite(got[0][1]))
    assert np.all(got[1][2] == lib.REFINE_DECLINED) and np.all(np.isnan(got[1][1])) and np.array_equal(got[1][0], starts)
    assert large.stale                                              # (no host route: nothing fitted it)
    large.close()
    # a jittered EI: the value optimize(device=True) returns is the jittered acquisition's own at the point it returns
    cost = Cost(CompleteGraph.get_cost_structure(2), ["B", "D"])    # (fixed: the grid's batch cost is the point's cost)
    jittered = CausalExpectedImprovement(0.1, "min", c.twin, 0.05) / cost
    x, f = CausalGradientAcquisitionOptimizer(box, grid_shape=[8, 8]).optimize(jittered, refine=True, num_starts=3, device=True)
    assert np.allclose(f[0, 0], jittered.evaluate(x)[0, 0], rtol=1e-8, atol=0.0)      # (two routes to one number)
    plain = CausalExpectedImprovement(0.1, "min", c.twin) / cost
    assert not np.isclose(f[0, 0], plain.evaluate(x)[0, 0], rtol=1e-6, atol=0.0)


def test_the_library_refuses_bad_sets_before_any_launch(lib, zoo):
    c = zoo["n16 d2"]
    good = dict(starts=c.points(2), cost=costs_of(c, False), box=(c.lo, c.hi))

    def call(starts=good["starts"], cost=good["cost"], box=good["box"], **kw):
        rc, res = refine_call(lib, [c], [starts], [cost], boxes=[box], sentinel=-5.0, **kw)
        return rc, res[0]

    bad = ((dict(box=(c.hi, c.lo)), b"bound"), (dict(box=(c.lo, np.array([np.inf, 1.0]))), b"finite"),
           (dict(starts=np.array([[0.0, np.nan]])), b"starts"), (dict(cost=(np.zeros(2), np.zeros(2, dtype=np.int32))), b"cost"),
           (dict(cost=(np.array([1.0, -1.0]), np.ones(2, dtype=np.int32))), b"cost"),
           (dict(cost=(np.ones(2), np.array([0, 2], dtype=np.int32))), b"cost_variable"),
           (dict(max_rounds=1001), b"max_rounds"), (dict(max_rounds=-1), b"max_rounds"), (dict(task="min", param=np.nan), b"jitter"),
           (dict(starts=np.zeros((65, 2))), b"starts"), (dict(y_best=[np.nan]), b"y_best"))
    for kw, word in bad:
        rc, res = call(**kw)
        assert rc == lib.CBO_ERR_INVALID and word in lib.load().cbo_last_error(), (kw, lib.load().cbo_last_error())
        assert np.all(res[1] == -5.0) and np.all(res[4] == -5)
    n = 1
    gps = (ctypes.c_void_p * n)(c.model._handle)
    assert lib.load().cbo_acq_refine_sets(1, gps, (lib.CboRefineSet * 1)(), 7, lib.dptr(np.zeros(1)), 0, 0.0, 5, lib.dptr(np.zeros(4)),
                                          lib.dptr(np.zeros(2)), lib.dptr(np.zeros(4)),
                                          np.zeros(2, dtype=np.int32).ctypes.data_as(lib.c_int_p),
                                          np.zeros(2, dtype=np.int32).ctypes.data_as(lib.c_int_p)) == lib.CBO_ERR_INVALID
    assert b"kind" in lib.load().cbo_last_error()


# ---------------------------------------------------------------------------------------------- 6. the Python layers
@pytest.mark.parametrize("cost_type", [1, 4])
def test_find_next_y_points_refines_every_winner(lib, cost_type):
    """The toy sets (toy_init_X, toy_init_Z) and the complete graph's d = 3 data (complete_bo_d3) in one call: every refined
    value at least the grid winner's, the points in their boxes, refine=False today's bits."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph, ToyGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import CandidateGrid, find_next_y_points
    fx = [load_fixture(n) for n in ("toy_init_X", "toy_init_Z", "complete_bo_d3")]
    es = [["X"], ["Z"], ["B", "D", "E"]]
    boxes = [ToyGraph.bounds(es[0]), ToyGraph.bounds(es[1]), CompleteGraph.bounds(es[2])]
    table = dict(ToyGraph.get_cost_structure(cost_type))
    table.update(CompleteGraph.get_cost_structure(cost_type))
    models = [HipGaussianProcess(f["X"], f["y"], variance=1.0, lengthscale=1.0, noise_var=1e-3, fit=False) for f in fx]
    grids = [CandidateGrid(meshgrid_candidates(b, shape), m) for b, shape, m in zip(boxes, ([100], [100], [6, 6, 6]), models)]
    y_best = float(min(f["y"].min() for f in fx))
    plain = find_next_y_points(models, y_best, es, table, "min", grids)
    again = find_next_y_points(models, y_best, es, table, "min", grids, refine=False, spaces=boxes)
    fine = find_next_y_points(models, y_best, es, table, "min", grids, refine=True, spaces=boxes)
    moved = 0
    for s in range(3):
        assert np.array_equal(plain[0][s], again[0][s]) and np.array_equal(bits(plain[1][s]), bits(again[1][s]))
        assert fine[1][s].shape == (1, 1) and fine[0][s].shape == (1, len(es[s]))
        assert fine[1][s][0, 0] >= plain[1][s][0, 0]
        assert all(lo <= v <= hi for v, (lo, hi) in zip(fine[0][s][0], boxes[s]))
        moved += int(not np.array_equal(fine[0][s], plain[0][s]))
    print("cost type", cost_type, "grid", [float(y[0, 0]) for y in plain[1]], "refined", [float(y[0, 0]) for y in fine[1]])
    assert moved >= 1                                               # (a 100-point grid does not hold a continuous optimum)
    for g in grids:
        g.close()
    for m in models:
        m.close()


def test_the_agent_intervenes_at_a_refined_point(lib):
    """CBO(toy graph, refine=True).intervene(): the chosen set and point go through one trial; the point is inside the set's
    interventional range and the set's data grew by that row."""
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
    fx = [load_fixture("toy_init_X"), load_fixture("toy_init_Z")]
    data = [(f["X"].copy(), f["y"].copy()) for f in fx]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=3, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, refine=True)
        assert agent.refine is True
        agent.intervene()
    (picked_set, picked_x), = [c for c in agent.monitor.chosen if c is not None]
    s = [list(e) for e in es].index(list(picked_set))
    (lo, hi), = ToyGraph.bounds(es[s])
    assert picked_x.shape == (1, 1) and lo <= picked_x[0, 0] <= hi
    assert agent.data_x[s].shape[0] == 11 and np.array_equal(agent.data_x[s][-1:], picked_x)
    assert agent.data_x[1 - s].shape[0] == 10
