"""GPU tests of causal exploration sets inside the one-launch L-BFGS refinement: cbo_acq_refine_sets_prior
(small_sets_refine_kernel's causal instantiations, do_prior_at) and the Python layers on top.

A causal set is a CausalRBF model whose prior closures are the do-calculus closures of a fitted RBF graph GP
(do_prior_functions), plus that graph GP's device-resident prior (DoPrior).  Set models of 10, 16, 17 and 50 observations
(less than one 16-row tile, exactly one, one row more, a partial fourth), d = 1, 2, 3, priors of 17 and 129 rows (one row
more than a tile; one more than the 128-column Gram tile), k one more than a workgroup carries at the set's d.
References: the numpy oracle's expected_improvement_with_gradients with the oracle's own do_prior arrays over the point's
cost at the bars of tests/test_sets_refine_gpu.py (value rtol 1e-6 / atol 1e-12, gradient rtol 1e-5 / atol 1e-10), the host
classes for the point-wise kinds at the same bars, and -- bit for bit -- the multi-set sweep on a one-point grid whose prior
arrays are cbo_do_prior_eval's."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

VALUE_BAR = dict(rtol=1e-6, atol=1e-12)
GRAD_BAR = dict(rtol=1e-5, atol=1e-10)
SET_HYPER = dict(variance=1.2, lengthscale=1.1, noise_var=1e-3)


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))
               for u, v in zip(a, b))


class CausalCase:
    """A graph GP (n_g rows, d_in columns), the observed rows, and one causal exploration set over the intervened columns:
    the UNFITTED device model with the do-calculus closures, its DoPrior, and the oracle's posterior of the same model."""

    def __init__(self, n, n_g, d_in, idx, ard=False, seed=0, lo=-2.0, hi=2.0):
        from cbo_with_oop_amd.DoCalculus import DoPrior, do_prior_functions
        from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
        rng = np.random.default_rng(1000 * n + 10 * n_g + seed)
        self.idx = list(idx)
        d = max(idx) + 1
        Xg = rng.uniform(lo, hi, (n_g, d_in))
        yg = np.sin(1.2 * Xg[:, :1]) + 0.3 * (Xg ** 2).sum(1, keepdims=True) / d_in + 0.1 * rng.standard_normal((n_g, 1))
        self.g_hyper = dict(variance=1.4, lengthscale=rng.uniform(0.9, 1.5, d_in) if ard else 1.3, noise_var=1e-2)
        self.observed = rng.uniform(lo, hi, (37, d_in))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            self.graph_gp = HipGaussianProcess(Xg, yg, ard=ard, fix_noise=True, **self.g_hyper)
        self.graph_post = O.fit(Xg, yg, **self.g_hyper)
        self.lo, self.hi = np.full(d, float(lo)), np.full(d, float(hi))
        self.X = rng.uniform(self.lo, self.hi, (n, d))
        self.y = np.sin(1.3 * self.X[:, :1]) + 0.3 * (self.X ** 2).sum(1, keepdims=True) / d + 0.03 * rng.standard_normal((n, 1))
        self.closures = do_prior_functions(self.graph_gp, self.observed, self.idx)
        self.kw = dict(SET_HYPER, mean_function=self.closures[0], variance_adjustment=self.closures[1])
        self.model = HipGaussianProcess(self.X, self.y, fit=False, **self.kw)
        self.prior = DoPrior(self.graph_gp, self.observed, self.idx)
        self.n, self.d, self.rng = n, d, rng
        self.y_best = float(self.y.min()) + 0.1
        self._post = self._twin = None

    def oracle_prior(self, pts):
        return (O.do_prior(self.graph_post, self.observed, self.idx, pts, 0),
                O.do_prior(self.graph_post, self.observed, self.idx, pts, 1))

    @property
    def post(self):
        if self._post is None:
            mX, vX = self.oracle_prior(self.X)
            self._post = O.fit(self.X, self.y, mX, vX, **SET_HYPER)
        return self._post

    @property
    def twin(self):
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
        pts = self.rng.uniform(self.lo, self.hi, (k, self.d))
        grid = np.linspace(self.lo, self.hi, 5)
        for i in range(1, k, 2):
            pts[i] = grid[self.rng.integers(0, 5, self.d), np.arange(self.d)]
        return pts

    def close(self):
        self.prior.close()
        self.model.close()
        if self._twin is not None:
            self._twin.close()
        self.graph_gp.close()


SHAPES = {"n10 d1 g17": dict(n=10, n_g=17, d_in=2, idx=[0, -1]),
          "n16 d2 g129": dict(n=16, n_g=129, d_in=3, idx=[1, -1, 0], ard=True),
          "n17 d3 g17": dict(n=17, n_g=17, d_in=3, idx=[2, 0, 1]),
          "n50 d2 g129": dict(n=50, n_g=129, d_in=2, idx=[0, 1], ard=True)}


@pytest.fixture(scope="module")
def zoo(lib):
    cases = {name: CausalCase(**kw) for name, kw in SHAPES.items()}
    yield cases
    for c in cases.values():
        c.close()


def costs_of(case, variable):
    fix = np.ones(case.d) if variable else 1.0 + np.arange(case.d, dtype=np.float64)
    return fix, np.full(case.d, 1 if variable else 0, dtype=np.int32)


def point_cost(fix, variable, x):
    from cbo_with_oop_amd.utils_functions.causal_optimizer import one_row_cost
    return one_row_cost(fix, variable, x)


def refine_call(lib, cases, starts, costs, kind="EI", y_best=None, task="min", param=0.0, max_rounds=200, sentinel=None,
                priors="own", entry="prior"):
    """cbo_acq_refine_sets_prior (or, entry="plain", cbo_acq_refine_sets): (rc, per set (x, val, grad, rounds, status))."""
    n = len(cases)
    starts = [np.ascontiguousarray(s, dtype=np.float64) for s in starts]
    keep = []
    sets = (lib.CboRefineSet * n)()
    for j, c in enumerate(cases):
        lo, hi = np.ascontiguousarray(c.lo, dtype=np.float64), np.ascontiguousarray(c.hi, dtype=np.float64)
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
    tail = (lib.REFINE_KIND_CODE[kind], lib.dptr(yb), lib.TASK_CODE[task], param, max_rounds, lib.dptr(x), lib.dptr(v),
            lib.dptr(g), rounds.ctypes.data_as(lib.c_int_p), status.ctypes.data_as(lib.c_int_p))
    if entry == "plain":
        rc = lib.load().cbo_acq_refine_sets(n, gps, sets, *tail)
    else:
        if priors == "own":
            priors = [getattr(c, "prior", None) for c in cases]
        handles = (ctypes.c_void_p * n)(*[None if p is None else p._handle for p in priors])
        rc = lib.load().cbo_acq_refine_sets_prior(n, gps, sets, handles, *tail)
    out, r0, o0 = [], 0, 0
    for s in starts:
        k, d = s.shape
        out.append((x[r0:r0 + k * d].reshape(k, d), v[o0:o0 + k], g[r0:r0 + k * d].reshape(k, d), rounds[o0:o0 + k],
                    status[o0:o0 + k]))
        r0, o0 = r0 + k * d, o0 + k
    return rc, out


def one_point_sweep(lib, case, x, cost, kind="EI", task="min", param=0.0):
    """cbo_acq_sweep_sets (_kind) on the one-point grid {x} whose prior arrays are cbo_do_prior_eval's."""
    pts = np.ascontiguousarray(x[None, :])
    pm, pv = case.prior.evaluate(pts)
    pm, pv = np.ascontiguousarray(pm[:, 0]), np.ascontiguousarray(pv[:, 0])
    h = ctypes.c_void_p()
    lib.check(lib.load().cbo_cands_create(case.model._ctx.handle, 1, case.d, lib.dptr(pts), lib.dptr(pm), lib.dptr(pv), 0,
                                          ctypes.byref(h)))
    gps, cds = (ctypes.c_void_p * 1)(case.model._handle), (ctypes.c_void_p * 1)(h)
    yb, c = np.array([case.y_best]), np.array([float(cost)])
    val, idx = np.zeros(1), np.zeros(1, dtype=np.int64)
    if kind == "EI":
        rc = lib.load().cbo_acq_sweep_sets(1, gps, cds, lib.dptr(yb), lib.TASK_CODE[task], param, lib.dptr(c), lib.dptr(val),
                                           idx.ctypes.data_as(lib.c_int64_p))
    else:
        rc = lib.load().cbo_acq_sweep_sets_kind(1, gps, cds, lib.ACQ_KIND_CODE[kind], lib.dptr(yb), lib.TASK_CODE[task],
                                                param, lib.dptr(c), lib.dptr(val), idx.ctypes.data_as(lib.c_int64_p))
    lib.load().cbo_cands_destroy(h)
    lib.check(rc)
    return val[0]


# ---------------------------------------------------------------------------------------------- 1. values and gradients
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_ei_values_and_gradients_at_the_starts(lib, zoo, name, task):
    c = zoo[name]
    k = c.per_block + 1
    pts = c.points(k)
    cost = costs_of(c, task == "max")
    rc, ((x, val, grad, rounds, status),) = refine_call(lib, [c], [pts], [cost], task=task, max_rounds=0)
    lib.check(rc)
    assert np.array_equal(x, pts) and np.all(rounds == 0) and np.all(status != lib.REFINE_DECLINED)
    price = np.array([point_cost(cost[0], cost[1], p) for p in pts])
    mXs, vXs = c.oracle_prior(pts)
    fo, dfo = O.expected_improvement_with_gradients(c.post, pts, c.y_best, mXs, vXs, task=task)
    print(name, task, "value rel", np.max(np.abs(val - fo[:, 0] / price) / np.maximum(np.abs(fo[:, 0] / price), 1e-300)),
          "grad abs", np.max(np.abs(grad - dfo / price[:, None])))
    assert np.allclose(val, fo[:, 0] / price, **VALUE_BAR)
    assert np.allclose(grad, dfo / price[:, None], **GRAD_BAR)
    for i in range(k):
        assert bits(val[i]) == bits(one_point_sweep(lib, c, pts[i], price[i], task=task)), (i, pts[i])
    assert c.model.stale                                           # the models are only read: nothing was fitted


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("kind", ["LCB", "PI", "VAR", "MPEI"])
def test_pointwise_kinds_against_the_host_classes(lib, zoo, kind, task):
    from cbo_with_oop_amd.utils_functions import pointwise_acquisitions as pw
    for name in ("n16 d2 g129", "n17 d3 g17"):
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
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_start_ends_no_lower_inside_the_box_with_the_bits_of_a_fresh_evaluation(lib, zoo, name):
    c = zoo[name]
    seen = set()
    for k, variable in ((1, False), (c.per_block + 1, True)):
        starts, cost = c.points(k), costs_of(c, variable)
        rc, (res0,) = refine_call(lib, [c], [starts], [cost], max_rounds=0)
        lib.check(rc)
        rc, (res,) = refine_call(lib, [c], [starts], [cost])
        lib.check(rc)
        x, val, grad, rounds, status = res
        assert np.all(val >= res0[1]), (val, res0[1])
        assert np.all(x >= c.lo) and np.all(x <= c.hi)
        assert set(status.tolist()) <= {lib.REFINE_PGTOL, lib.REFINE_FTOL, lib.REFINE_STEP, lib.REFINE_MAX_ROUNDS}
        assert np.all(rounds >= 0) and np.all(rounds <= 200)
        rc, (fresh,) = refine_call(lib, [c], [x], [cost], max_rounds=0)
        lib.check(rc)
        assert np.array_equal(bits(fresh[1]), bits(val)) and np.array_equal(bits(fresh[2]), bits(grad))
        for i in range(min(k, 3)):
            assert bits(val[i]) == bits(one_point_sweep(lib, c, x[i], point_cost(cost[0], cost[1], x[i]))), i
        rc, (twice,) = refine_call(lib, [c], [starts], [cost])
        lib.check(rc)
        assert same(res, twice)
        seen |= set(status.tolist())
        print(name, k, "rounds", rounds.tolist(), "status", status.tolist())
    assert lib.REFINE_PGTOL in seen or lib.REFINE_FTOL in seen


def test_one_dimensional_set_ends_where_lockstep_lbfgs_ends(lib):
    """The in-kernel searches against lockstep_lbfgs driven on the host by the max_rounds = 0 entry, from the four best of
    200 grid points: the values agree to rtol 1e-5."""
    from cbo_with_oop_amd.utils_functions.causal_optimizer import lockstep_lbfgs
    c = CausalCase(50, 129, 2, [-1, 0], seed=3, lo=-3.0, hi=3.0)
    cost = costs_of(c, False)

    def fun(X):
        rc, ((_, val, grad, _, _),) = refine_call(lib, [c], [X], [cost], max_rounds=0)
        lib.check(rc)
        return val.copy(), grad.copy()

    grid = np.linspace(-3.0, 3.0, 200)[:, None]
    acq = np.concatenate([fun(grid[i:i + 50])[0] for i in range(0, 200, 50)])
    starts = grid[np.argsort(-acq, kind="stable")[:4]]
    X, F = lockstep_lbfgs(fun, starts, c.lo, c.hi)
    rc, ((x, val, _, rounds, status),) = refine_call(lib, [c], [starts], [cost])
    lib.check(rc)
    print("kernel", val.tolist(), "host", F.tolist(), "rounds", rounds.tolist(), "status", status.tolist())
    assert np.allclose(val, F, rtol=1e-5, atol=0.0)
    c.close()


# ---------------------------------------------------------------------------------------------- 3. a mixed list
class Plain:
    """A non-causal set (small or large)."""

    def __init__(self, n, d, seed):
        from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
        rng = np.random.default_rng(seed)
        self.lo, self.hi, self.d = np.full(d, -2.0), np.full(d, 2.0), d
        X = rng.uniform(self.lo, self.hi, (n, d))
        y = np.sin(1.3 * X[:, :1]) + 0.05 * rng.standard_normal((n, 1))
        self.model = HipGaussianProcess(X, y, fit=False, **SET_HYPER)
        self.y_best, self.prior = float(y.min()) + 0.1, None


def test_a_mixed_list(lib, zoo):
    """A causal set with its prior, a plain set, a causal set WITHOUT a prior and a large model in one call: the plain set's
    outputs are cbo_acq_refine_sets' alone bit for bit, the causal set's its own call's, the other two are declined and
    untouched.  More causal sets than travel by value (nine) give each set the bits of its own call."""
    causal, other = zoo["n16 d2 g129"], zoo["n50 d2 g129"]
    plain, large = Plain(16, 2, 5), Plain(150, 2, 6)
    cases = [causal, plain, other, large]
    rng = np.random.default_rng(8)
    starts = [c.points(3) if isinstance(c, CausalCase) else rng.uniform(c.lo, c.hi, (3, c.d)) for c in cases]
    costs = [costs_of(c, i % 2 == 0) for i, c in enumerate(cases)]
    priors = [causal.prior, None, None, None]
    for max_rounds in (0, 200):
        rc, res = refine_call(lib, cases, starts, costs, max_rounds=max_rounds, sentinel=-77.0, priors=priors)
        lib.check(rc)
        rc, (alone_plain,) = refine_call(lib, [plain], [starts[1]], [costs[1]], max_rounds=max_rounds, entry="plain")
        lib.check(rc)
        rc, (alone_causal,) = refine_call(lib, [causal], [starts[0]], [costs[0]], max_rounds=max_rounds)
        lib.check(rc)
        assert same(res[1], alone_plain) and same(res[0], alone_causal)
        assert np.all(res[0][4] != lib.REFINE_DECLINED) and np.all(res[1][4] != lib.REFINE_DECLINED)
        for i in (2, 3):
            x, val, grad, rounds, status = res[i]
            assert np.all(status == lib.REFINE_DECLINED)
            assert np.all(x == -77.0) and np.all(val == -77.0) and np.all(grad == -77.0) and np.all(rounds == -77)
    # with every prior NULL the call is cbo_acq_refine_sets
    rc, a = refine_call(lib, cases, starts, costs, sentinel=-77.0, priors=[None] * 4)
    lib.check(rc)
    rc, b = refine_call(lib, cases, starts, costs, sentinel=-77.0, entry="plain")
    lib.check(rc)
    assert all(same(u, v) for u, v in zip(a, b)) and np.all(a[0][4] == lib.REFINE_DECLINED)
    # nine causal sets and a plain one: descriptors read from the pinned array
    many = [causal, other, zoo["n10 d1 g17"]] * 3 + [plain]
    st = [c.points(2) if isinstance(c, CausalCase) else starts[1] for c in many]
    cs = [costs_of(c, False) for c in many]
    rc, together = refine_call(lib, many, st, cs, max_rounds=30)
    lib.check(rc)
    for i, c in enumerate(many):
        rc, (alone,) = refine_call(lib, [c], [st[i]], [cs[i]], max_rounds=30)
        lib.check(rc)
        assert same(together[i], alone), i
    # argument errors, before any launch
    rc, res = refine_call(lib, [plain], [starts[1]], [costs[1]], sentinel=-5.0, priors=[causal.prior])
    assert rc == lib.CBO_ERR_INVALID and b"prior" in lib.load().cbo_last_error() and np.all(res[0][4] == -5)
    rc, res = refine_call(lib, [causal], [starts[0]], [costs[0]], sentinel=-5.0, priors=[zoo["n10 d1 g17"].prior])
    assert rc == lib.CBO_ERR_INVALID and b"n_iv" in lib.load().cbo_last_error() and np.all(res[0][4] == -5)
    plain.model.close(); large.model.close()


# ---------------------------------------------------------------------------------------------- 4. the Python layers
def toy_cost(names, cost_type=1):
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions import Cost
    return Cost(CompleteGraph.get_cost_structure(cost_type), names), CompleteGraph.get_cost_structure(cost_type)


def test_refine_sets_takes_causal_sets_only_when_asked(lib, zoo):
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalGradientAcquisitionOptimizer
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    c = zoo["n16 d2 g129"]
    cost, table = toy_cost(["B", "D"], 2)
    box = list(zip(c.lo.tolist(), c.hi.tolist()))
    starts = c.points(3)
    # the default: DECLINED, with the host route's values
    (x0, f0, s0), = refine_sets([c.model], [starts], [box], c.y_best, "min", [cost])
    assert np.all(s0 == lib.REFINE_DECLINED)
    xs, fs = CausalGradientAcquisitionOptimizer(box).refine_batched(CausalExpectedImprovement(c.y_best, "min", c.model) / cost, starts)
    assert np.array_equal(bits(x0), bits(xs)) and np.array_equal(bits(f0), bits(fs))
    # device_prior=True: the launch's own outputs
    (x1, f1, s1), = refine_sets([c.model], [starts], [box], c.y_best, "min", [cost], device_prior=True)
    fix = np.array([float(table[v].args[0]) for v in ["B", "D"]])
    rc, (direct,) = refine_call(lib, [c], [starts], [(fix, np.zeros(2, dtype=np.int32))])
    lib.check(rc)
    assert np.all(s1 != lib.REFINE_DECLINED) and np.array_equal(s1, direct[4])
    assert np.array_equal(bits(x1), bits(direct[0])) and np.array_equal(bits(f1), bits(direct[1]))
    print("device", f1.tolist(), "host route", f0.tolist())
    # closures prior_spec does not recognise: today's route
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    m, v = c.closures
    odd = HipGaussianProcess(c.X, c.y, fit=False, **dict(SET_HYPER, mean_function=lambda a: m(a), variance_adjustment=v))
    (_, _, s2), = refine_sets([odd], [starts], [box], c.y_best, "min", [cost], device_prior=True, host_fallback=False)
    assert np.all(s2 == lib.REFINE_DECLINED)
    odd.close()
    # optimize(refine=True, device=True, device_prior=True) keeps the refined point only if it is not lower
    opt = CausalGradientAcquisitionOptimizer(box, grid_shape=[12, 12])
    acq = CausalExpectedImprovement(c.y_best, "min", c.twin) / cost
    xg, fg = opt.optimize(acq)
    xr, fr = opt.optimize(acq, refine=True, num_starts=4, device=True, device_prior=True)
    assert fr[0, 0] >= fg[0, 0] and np.all(xr[0] >= c.lo) and np.all(xr[0] <= c.hi)
    with pytest.raises(ValueError, match="device=True"):
        opt.optimize(acq, refine=True, device=True)


def test_find_next_y_points_and_the_agent_keep_a_refined_point_only_if_it_is_not_lower(lib, zoo):
    from cbo_with_oop_amd.graphs import CompleteGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import CandidateGrid, find_next_y_points
    cases = [zoo["n16 d2 g129"], zoo["n50 d2 g129"]]
    es = [["B", "D"], ["B", "D"]]
    boxes = [list(zip(c.lo.tolist(), c.hi.tolist())) for c in cases]
    table = dict(CompleteGraph.get_cost_structure(1))
    models = [c.model for c in cases]
    grids = [CandidateGrid(meshgrid_candidates(b, [10, 10]), m) for b, m in zip(boxes, models)]
    y_best = min(c.y_best for c in cases)
    plain = find_next_y_points(models, y_best, es, table, "min", grids)
    host = find_next_y_points(models, y_best, es, table, "min", grids, refine=True, spaces=boxes)
    fine = find_next_y_points(models, y_best, es, table, "min", grids, refine=True, spaces=boxes, device_prior=True)
    for s in range(2):
        assert fine[1][s].shape == (1, 1) and fine[0][s].shape == (1, 2)
        assert fine[1][s][0, 0] >= plain[1][s][0, 0]
        assert all(lo <= v <= hi for v, (lo, hi) in zip(fine[0][s][0], boxes[s]))
        assert host[1][s][0, 0] >= plain[1][s][0, 0]
        print("set", s, "grid", plain[1][s][0, 0], "host route", host[1][s][0, 0], "device", fine[1][s][0, 0])
    with pytest.raises(ValueError, match="refine"):
        find_next_y_points(models, y_best, es, table, "min", grids, device_prior=True)
    for g in grids:
        g.close()

    # the agent: the complete graph's set ['B'] with its causal prior (gp_B), refined on the device
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    from cbo_with_oop_amd.utils_functions.graph_functions import compute_interventions, sample_from_model
    sem = CompleteGraph.define_sem()
    rng = np.random.default_rng(11)
    rows = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(200)]
    obs = {v: np.array([r[v] for r in rows]) for v in rows[0] if not v.startswith("U")}
    init = {k: v[:100] for k, v in obs.items()}
    lo, hi = np.array(CompleteGraph.bounds(["B"])).T
    x = np.random.default_rng(2).uniform(lo, hi, (5, 1))
    data = [(x, compute_interventions(sem, {"B": ""}, x, target_variable="Y"))]
    with pytest.raises(ValueError, match="refine"):
        CBO(CompleteGraph, init, obs, data, exploration_set=[["B"]], causal_prior=True, device_prior=True)
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(CompleteGraph, init, obs, data, exploration_set=[["B"]], num_trials=4, initial_num_obs_samples=100,
                    causal_prior=True, grid_shapes=[[64]], refine=True, device_prior=True)
        assert agent.device_prior is True
        agent.run()
    picked = [c for c in agent.monitor.chosen if c is not None]
    assert picked and all(lo[0] <= p[1][0, 0] <= hi[0] for p in picked)
    # ... and the device route is what its causal model takes
    model = agent.models[0]
    assert model.causal
    cost, _ = toy_cost(["B"], 1)
    start = np.array([[0.5 * (lo[0] + hi[0])]])
    (_, f, s), = refine_sets([model], [start], [CompleteGraph.bounds(["B"])], 0.0, "min", [cost], device_prior=True,
                             host_fallback=False)
    assert np.all(s != lib.REFINE_DECLINED) and np.all(np.isfinite(f))
