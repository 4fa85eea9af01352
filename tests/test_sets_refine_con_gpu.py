"""GPU tests of the gradient refinement under constraints: cbo_acq_refine_sets_constrained
(small_sets_refine_con_kernel, kernels_sets_refine_con.hip) and the Python layers on top.

Shapes are the smallest at which the kernel can go wrong: models of n in {12, 17, 70, 128} observations mixed within a set
(less than a tile, one row into a second tile, more than 64 -- where the sibling kernel's LDS rings would be overwritten by the
reload --, the cap), among them a 12-row objective under a 70-row constraint and a 128-row objective under a 12-row
constraint (the tile count changes between two reloads); d = 1, d = 3 ARD with every model's own lengthscales, d = 8 (one
start per wave); n_con in {1, 3, 8} (nine descriptors exceed the eight that travel by value), senses alternating; k = 17 at
d = 3 (two workgroups).  References: bit for bit the constrained multi-set sweeps on a one-point grid; the host classes
AcquisitionProduct / ConstrainedLogExpectedImprovement over the point's cost; lockstep_lbfgs driven by the device's own
max_rounds = 0 entry."""
import ctypes
import functools
import warnings

import mpmath as mp
import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

NOT_FITTED = -5
LE, GE = 0, 1
VALUE_BAR = dict(rtol=1e-6, atol=1e-12)
GRAD_BAR = dict(rtol=1e-5, atol=1e-10)


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def handles(objs):
    return (ctypes.c_void_p * len(objs))(*[o._handle for o in objs])


def gp(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


class Node:
    """One model of a set: data of its own on the set's box, unfitted (the launch works from resident data); ``twin`` is a
    fitted model on the same data for the host classes."""

    def __init__(self, n, d, seed, noise=1e-3, ard=False, phase=0.0, fit=False, **more):
        rng = np.random.default_rng(100 * n + 10 * d + seed)
        self.X = rng.uniform(-2.0, 2.0, (n, d))
        self.y = (np.sin(1.3 * self.X[:, :1] + phase) + 0.3 * np.cos(self.X + 0.5 * seed).sum(1, keepdims=True)
                  + 0.03 * rng.standard_normal((n, 1)))
        ls = (0.8 + 0.25 * np.arange(d) + 0.1 * seed) if ard else 1.0 + 0.1 * seed
        self.kw = dict(variance=1.2 + 0.1 * seed, lengthscale=ls, noise_var=noise, ard=ard, **more)
        self.model = gp(self.X, self.y, fit=fit, **self.kw)
        self._twin = None

    @property
    def twin(self):
        if self._twin is None:
            self._twin = gp(self.X, self.y, **self.kw)
        return self._twin

    def close(self):
        self.model.close()
        if self._twin is not None:
            self._twin.close()


class ConSet:
    """An objective and its constraints: (node, value, jitter, sense) each, the bound inside the constrained node's range."""

    def __init__(self, d, obj_n, con_ns, seed=0, noise=1e-3, ard=False, values=None):
        self.d = d
        self.obj = Node(obj_n, d, seed, noise, ard)
        self.cons = []
        for k, n in enumerate(con_ns):
            node = Node(n, d, seed + k + 1, noise, ard, phase=0.4 * (k + 1))
            value = (0.5 * (float(node.y.min()) + float(node.y.max())) + 0.1 * k) if values is None else values[k]
            self.cons.append((node, value, 0.0078125 * k, (LE, GE)[k % 2]))
        self.lo, self.hi = np.full(d, -2.0), np.full(d, 2.0)
        self.rng = np.random.default_rng(7 + seed)

    def y_best(self, task):
        return float(self.obj.y.min()) + 0.1 if task == "min" else float(self.obj.y.max()) - 0.1

    def points(self, k):
        return self.rng.uniform(self.lo, self.hi, (k, self.d))

    def nodes(self):
        return [self.obj] + [c[0] for c in self.cons]

    def pofs(self, twins=True):
        from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility
        return [ProbabilityOfFeasibility(n.twin if twins else n.model, jitter=j, max_value=v, sense=("<=", ">=")[s])
                for n, v, j, s in self.cons]

    def host(self, log_form, task, jitter, cost):
        """The host class over ``cost`` on the fitted twins."""
        from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement
        from cbo_with_oop_amd.utils_functions.constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement
        from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement
        if log_form:
            return ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(self.y_best(task), task, self.obj.twin, jitter),
                                                     self.pofs()) / cost
        return AcquisitionProduct([CausalExpectedImprovement(self.y_best(task), task, self.obj.twin, jitter)] + self.pofs()) / cost

    def close(self):
        for n in self.nodes():
            n.close()


def fixed_cost(d):
    return 1.0 + np.arange(d, dtype=np.float64), np.zeros(d, dtype=np.int32)


def variable_cost(d):
    return np.ones(d), np.ones(d, dtype=np.int32)


def point_cost(cost, x):
    from cbo_with_oop_amd.utils_functions.causal_optimizer import one_row_cost
    return one_row_cost(cost[0], cost[1], x)


def graph_cost(cost):
    """The ``Cost`` object of a (fix, variable) pair: what ``cost_structure`` reads back."""
    from cbo_with_oop_amd import graphs
    from cbo_with_oop_amd.utils_functions import Cost
    names = [f"V{k}" for k in range(len(cost[0]))]
    return Cost({n: functools.partial(graphs.cost, float(f), bool(v)) for n, f, v in zip(names, cost[0], cost[1])}, names)


def refine_con(lib, sets, starts, costs, log_form, task="min", jitter=0.0, max_rounds=200, sentinel=None,
               drop_constraints=False):
    """cbo_acq_refine_sets_constrained itself: (rc, per set (x, val, grad, rounds, status))."""
    n = len(sets)
    starts = [np.ascontiguousarray(s, dtype=np.float64) for s in starts]
    keep = []
    rs = (lib.CboRefineSet * n)()
    for j, st in enumerate(sets):
        lo, hi = np.ascontiguousarray(st.lo), np.ascontiguousarray(st.hi)
        fix, variable = (np.ascontiguousarray(costs[j][0], dtype=np.float64), np.ascontiguousarray(costs[j][1], dtype=np.int32))
        keep += [lo, hi, fix, variable]
        rs[j].k = starts[j].shape[0]
        rs[j].starts = starts[j].ctypes.data_as(lib.c_double_p)
        rs[j].lo, rs[j].hi = lo.ctypes.data_as(lib.c_double_p), hi.ctypes.data_as(lib.c_double_p)
        rs[j].cost_fix, rs[j].cost_variable = fix.ctypes.data_as(lib.c_double_p), variable.ctypes.data_as(lib.c_int_p)
    rows, total = sum(s.size for s in starts), sum(s.shape[0] for s in starts)
    fill = 0.0 if sentinel is None else sentinel
    x, g, v = np.full(rows, fill), np.full(rows, fill), np.full(total, fill)
    rounds, status = np.full(total, int(fill), dtype=np.int32), np.full(total, int(fill), dtype=np.int32)
    yb = np.array([st.y_best(task) for st in sets], dtype=np.float64)
    cons = [] if drop_constraints else [c for st in sets for c in st.cons]
    n_con = np.array([0 if drop_constraints else len(st.cons) for st in sets], dtype=np.int32)
    none = len(cons) == 0
    values = np.array([c[1] for c in cons] or [0.0], dtype=np.float64)
    jitters = np.array([c[2] for c in cons] or [0.0], dtype=np.float64)
    senses = np.array([c[3] for c in cons] or [0], dtype=np.int32)
    rc = lib.load().cbo_acq_refine_sets_constrained(
        n, handles([st.obj.model for st in sets]), rs, int(log_form), lib.dptr(yb), lib.TASK_CODE[task],
        float(jitter), n_con.ctypes.data_as(lib.c_int_p), None if none else handles([c[0].model for c in cons]),
        None if none else lib.dptr(values), None if none else lib.dptr(jitters),
        None if none else senses.ctypes.data_as(lib.c_int_p), max_rounds, lib.dptr(x), lib.dptr(v), lib.dptr(g),
        rounds.ctypes.data_as(lib.c_int_p), status.ctypes.data_as(lib.c_int_p))
    out, r0, o0 = [], 0, 0
    for s in starts:
        k, d = s.shape
        out.append((x[r0:r0 + k * d].reshape(k, d), v[o0:o0 + k], g[r0:r0 + k * d].reshape(k, d), rounds[o0:o0 + k],
                    status[o0:o0 + k]))
        r0, o0 = r0 + k * d, o0 + k
    return rc, out


def one_point_sweep(lib, st, x, cost, log_form, task, jitter):
    """The constrained multi-set sweep's value for the one-point grid {x} with costs[i] = cost."""
    from cbo_with_oop_amd import CandidateGrid
    pts = np.ascontiguousarray(x[None, :])
    grids = [CandidateGrid(pts, n.model) for n in st.nodes()]
    n_con = np.array([len(st.cons)], dtype=np.int32)
    values = np.array([c[1] for c in st.cons], dtype=np.float64)
    jitters = np.array([c[2] for c in st.cons], dtype=np.float64)
    senses = np.array([c[3] for c in st.cons], dtype=np.int32)
    val, idx = np.zeros(1), np.zeros(1, dtype=np.int64)
    call = lib.load().cbo_acq_sweep_sets_constrained_log if log_form else lib.load().cbo_acq_sweep_sets_constrained
    rc = call(1, handles([st.obj.model]), handles(grids[:1]), lib.dptr(np.array([st.y_best(task)])), lib.TASK_CODE[task],
              float(jitter), lib.dptr(np.array([float(cost)])), n_con.ctypes.data_as(lib.c_int_p),
              handles([c[0].model for c in st.cons]), handles(grids[1:]), lib.dptr(values), lib.dptr(jitters),
              senses.ctypes.data_as(lib.c_int_p), lib.dptr(val), idx.ctypes.data_as(lib.c_int64_p))
    for g in grids:
        g.close()
    lib.check(rc)
    return val[0]


def unfitted(lib, st):
    out = np.empty(1)
    return all(n.model.stale and lib.load().cbo_gp_log_marginal(n.model._handle, lib.dptr(out)) == NOT_FITTED
               for n in st.nodes())


SETS = {"d1 n12 under n70": dict(d=1, obj_n=12, con_ns=[70]),
        "d1 n128 under n12": dict(d=1, obj_n=128, con_ns=[12], seed=1),
        "d3 ard n17 under n70 n12 n128": dict(d=3, obj_n=17, con_ns=[70, 12, 128], ard=True, seed=2),
        "d8 n70 under eight": dict(d=8, obj_n=70, con_ns=[12, 17, 70, 128, 12, 17, 70, 12], seed=3)}
STARTS = {"d1 n12 under n70": 5, "d1 n128 under n12": 5, "d3 ard n17 under n70 n12 n128": 17, "d8 n70 under eight": 5}


@pytest.fixture(scope="module")
def zoo(lib):
    built = {name: ConSet(**kw) for name, kw in SETS.items()}
    yield built
    for st in built.values():
        st.close()


# ------------------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("log_form", [False, True])
@pytest.mark.parametrize("name", list(SETS))
def test_values_at_the_starts_are_the_constrained_sweeps_bits(lib, zoo, name, log_form):
    """max_rounds = 0: val_out at a start is bit for bit cbo_acq_sweep_sets_constrained (_log) on a one-point grid there with
    costs[i] = c(x), for both tasks under a variable and a fixed cost; the models are unfitted and stay unfitted."""
    st = zoo[name]
    pts = st.points(STARTS[name])
    for task, cost in (("min", variable_cost(st.d)), ("max", fixed_cost(st.d))):
        rc, ((x, val, grad, rounds, status),) = refine_con(lib, [st], [pts], [cost], log_form, task, 0.015625, max_rounds=0)
        lib.check(rc)
        assert np.array_equal(x, pts) and np.all(rounds == 0)
        assert set(status.tolist()) <= {lib.REFINE_PGTOL, lib.REFINE_MAX_ROUNDS}
        for i in range(len(pts)):
            want = one_point_sweep(lib, st, pts[i], point_cost(cost, pts[i]), log_form, task, 0.015625)
            assert bits(val[i])[0] == bits(want)[0], (task, i, pts[i], val[i], want)
    assert unfitted(lib, st)


@pytest.mark.parametrize("log_form", [False, True])
def test_sets_without_constraints_return_the_unconstrained_calls_bits(lib, zoo, log_form):
    """Every n_con = 0: all five outputs are cbo_acq_refine_sets' (kind 0) / cbo_acq_refine_sets_logei's, bit for bit, after a
    whole search; the con_* arrays are NULL."""
    sets = [zoo["d1 n12 under n70"], zoo["d3 ard n17 under n70 n12 n128"]]
    starts = [st.points(4) for st in sets]
    costs = [variable_cost(st.d) for st in sets]
    rc, got = refine_con(lib, sets, starts, costs, log_form, "min", 0.0, sentinel=-77.0, drop_constraints=True)
    lib.check(rc)
    n = len(sets)
    rs = (lib.CboRefineSet * n)()
    keep = []
    for j, st in enumerate(sets):
        fix, variable = costs[j]
        keep += [np.ascontiguousarray(starts[j]), np.ascontiguousarray(st.lo), np.ascontiguousarray(st.hi)]
        rs[j].k = starts[j].shape[0]
        rs[j].starts = keep[-3].ctypes.data_as(lib.c_double_p)
        rs[j].lo, rs[j].hi = keep[-2].ctypes.data_as(lib.c_double_p), keep[-1].ctypes.data_as(lib.c_double_p)
        rs[j].cost_fix, rs[j].cost_variable = fix.ctypes.data_as(lib.c_double_p), variable.ctypes.data_as(lib.c_int_p)
    rows, total = sum(s.size for s in starts), sum(s.shape[0] for s in starts)
    x, g, v = np.full(rows, -77.0), np.full(rows, -77.0), np.full(total, -77.0)
    rounds, status = np.full(total, -77, dtype=np.int32), np.full(total, -77, dtype=np.int32)
    yb = np.array([st.y_best("min") for st in sets])
    tail = (200, lib.dptr(x), lib.dptr(v), lib.dptr(g), rounds.ctypes.data_as(lib.c_int_p), status.ctypes.data_as(lib.c_int_p))
    gps = handles([st.obj.model for st in sets])
    if log_form:
        lib.check(lib.load().cbo_acq_refine_sets_logei(n, gps, rs, lib.dptr(yb), 0, 0.0, *tail))
    else:
        lib.check(lib.load().cbo_acq_refine_sets(n, gps, rs, 0, lib.dptr(yb), 0, 0.0, *tail))
    flat = lambda k: np.concatenate([np.ravel(r[k]) for r in got])      # noqa: E731
    assert np.array_equal(bits(flat(0)), bits(x)) and np.array_equal(bits(flat(1)), bits(v))
    assert np.array_equal(bits(flat(2)), bits(g)) and np.array_equal(flat(3), rounds) and np.array_equal(flat(4), status)
    assert np.all(status != lib.REFINE_DECLINED)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))
               for u, v in zip(a, b))


@pytest.mark.parametrize("log_form", [False, True])
def test_a_mixed_call_returns_what_the_single_set_calls_return(lib, zoo, log_form):
    """A constrained set, an unconstrained one (an empty list) and another constrained one of another dimension in one call:
    per set the single-set call's five outputs, bit for bit, after whole searches; a second call gives the same bits."""

    class Plain:
        def __init__(self, st):
            self.obj, self.cons, self.d, self.lo, self.hi, self.y_best = st.obj, [], st.d, st.lo, st.hi, st.y_best
    sets = [zoo["d1 n12 under n70"], Plain(zoo["d1 n128 under n12"]), zoo["d3 ard n17 under n70 n12 n128"]]
    starts = [sets[0].points(3), zoo["d1 n128 under n12"].points(4), sets[2].points(17)]
    costs = [variable_cost(1), fixed_cost(1), variable_cost(3)]
    alone = []
    for j in range(3):
        rc, (res,) = refine_con(lib, [sets[j]], [starts[j]], [costs[j]], log_form, "min", 0.0, sentinel=-77.0)
        lib.check(rc)
        alone.append(res)
    for attempt in ("the call", "the same call again"):
        rc, res = refine_con(lib, sets, starts, costs, log_form, "min", 0.0, sentinel=-77.0)
        lib.check(rc)
        for j in range(3):
            assert same(res[j], alone[j]), (attempt, j)
            assert np.all(res[j][4] != lib.REFINE_DECLINED)


# ------------------------------------------------------------------------------------------------------------ 2. gradients
@pytest.fixture(scope="module")
def noisy(lib):
    """Models with noise 1e-2 (§4x's conditioning argument): d = 1 with one constraint, d = 3 with three."""
    built = {"d1": ConSet(1, 12, [17], seed=4, noise=1e-2), "d3": ConSet(3, 17, [12, 70, 17], seed=5, noise=1e-2)}
    yield built
    for st in built.values():
        st.close()


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("which", ["d1", "d3"])
def test_product_form_against_the_host_class(lib, noisy, which, task):
    """Value and gradient at the starts against AcquisitionProduct([...]) / cost's evaluate_with_gradients at the point's own
    cost, at the project's bars (value rtol 1e-6 / atol 1e-12, gradient rtol 1e-5 / atol 1e-10)."""
    from cbo_with_oop_amd.utils_functions.causal_optimizer import _values_and_gradients
    st = noisy[which]
    pts, cost = st.points(6), variable_cost(st.d)
    rc, ((x, val, grad, rounds, status),) = refine_con(lib, [st], [pts], [cost], False, task, 0.0078125, max_rounds=0)
    lib.check(rc)
    f, df = _values_and_gradients(st.host(False, task, 0.0078125, graph_cost(cost)), pts)
    print(f"{which} {task}: values {val.tolist()} host {f.tolist()}; worst |d grad| {np.abs(grad - df).max():.3e}")
    assert np.allclose(val, f, **VALUE_BAR) and np.allclose(grad, df, **GRAD_BAR)
    assert np.any(val != 0.0)


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("which", ["d1", "d3"])
def test_log_form_against_the_host_class_inside_the_range(lib, noisy, which, task):
    """Bounds inside the constrained nodes' ranges (|u| <= 30): the gradient within 1e-9 of ConstrainedLogExpectedImprovement's,
    relative to the gradient's largest component at that start (test_logei_gpu.py's bar); the value at rtol 1e-12."""
    from cbo_with_oop_amd.utils_functions.causal_optimizer import _values_and_gradients
    st = noisy[which]
    pts, cost = st.points(6), variable_cost(st.d)
    rc, ((x, val, grad, rounds, status),) = refine_con(lib, [st], [pts], [cost], True, task, 0.0078125, max_rounds=0)
    lib.check(rc)
    f, df = _values_and_gradients(st.host(True, task, 0.0078125, graph_cost(cost)), pts)
    rel = np.max(np.abs(grad - df), axis=1) / np.max(np.abs(df), axis=1)
    print(f"{which} {task}: gradient against the host class, worst relative {rel.max():.3e}; values", val.tolist())
    assert rel.max() <= 1e-9
    assert np.allclose(val, f, rtol=1e-12, atol=0.0)


FD_STEP = 2.0 ** -8
# The far bounds: 4 x the worst relative differences measured on an MI355X over the cases of
# test_log_form_with_a_bound_far_outside_the_range, relative to the gradient's largest component (1e7): |device - D_h| with D_h
# the central difference of the mpmath reference -- 1.600e-04, all of it the differences' own truncation (the estimate
# |D_2h - D_h| / 3 is 1.599e-04 and the host class sits at the same 1.600e-04 from D_h) -- and |device - host class|, 1.295e-08.
# DESIGN.md §4ab records both and the Richardson-extrapolated figure the test prints.
FAR_MEASURED_AGAINST_DIFFERENCES = 1.600e-4
FAR_MEASURED_AGAINST_HOST = 1.295e-8


def mp_log_value(st, pts, task, jitter):
    """log EI + sum log PoF at 60 digits from each twin's own ``predict`` doubles (cost 1)."""
    mv = [n.twin.predict(np.ascontiguousarray(pts)) for n in st.nodes()]
    out = []
    with mp.workdps(60):
        for i in range(len(pts)):
            mean, s = mp.mpf(float(mv[0][0][i, 0])), mp.sqrt(mp.mpf(float(mv[0][1][i, 0])))
            yb = mp.mpf(st.y_best(task))
            u = (yb - (mean + mp.mpf(jitter))) / s if task == "min" else ((mean - mp.mpf(jitter)) - yb) / s
            total = mp.log(mp.npdf(u) + u * mp.ncdf(u)) + mp.log(s)
            for (node, value, jit, sense), (cm, cv) in zip(st.cons, mv[1:]):
                uc = (mp.mpf(float(value)) - (mp.mpf(float(cm[i, 0])) + mp.mpf(float(jit)))) / mp.sqrt(mp.mpf(float(cv[i, 0])))
                total += mp.log(mp.ncdf(uc if sense == LE else -uc))
            out.append(total)
    return out


def test_log_form_with_a_bound_far_outside_the_range(lib):
    """A bound 1e3 below the constrained node's data with noise 1e-2: u of order -1e3 .. -1e4, so rho(u) ~ |u| and the
    constraint's gradient term rho du is of order 1e4 .. 1e6 -- no project bar covers it.  The device is measured against
    central differences D_h of the mpmath reference over the twins' predictions (h = 2^-8, §4x's step) and against the host
    class.  The differences' own error, per component, relative to the gradient's largest: truncation |D_2h - D_h| / 3
    (§4x's estimate, printed); rounding: the reference is exact in the doubles ``predict`` returns, which carry the solve's
    error -- mean to 2e-13 and sd to 1.3e-11 relative (§4x: condition number <= 2e3) -- so u = (value - mean) / sd, of size
    |u|, moves by |u| 1.3e-11 + 2e-13 / sd and log Phi(u) ~ -u^2 / 2 by |u| times that: 1.3e-11 u^2 per value, two values over
    2 h = 2^-7, against a gradient of size |u| |du| with |du| ~ |u| |d sd| / sd: relative 2 x 1.3e-11 x 2^7 / |d log sd| ~
    3.3e-9 / |d log sd|, a few 1e-8 where the standard deviation moves at all.  The bound asserted is 4 x the worst measured
    difference (the convention of §4aa's accuracy record)."""
    from cbo_with_oop_amd.utils_functions.causal_optimizer import _values_and_gradients
    worst_fd, worst_host = 0.0, 0.0
    for d, ns, seed in ((1, [17], 6), (3, [12, 70], 7)):
        probe = ConSet(d, 12, ns, seed=seed, noise=1e-2)
        values = []
        for k, (node, _, _, sense) in enumerate(probe.cons):
            values.append(float(node.y.min()) - 1e3 if sense == LE else float(node.y.max()) + 1e3)
        probe.close()
        st = ConSet(d, 12, ns, seed=seed, noise=1e-2, values=values)
        pts, cost = st.points(4), fixed_cost(d)
        rc, ((x, val, grad, rounds, status),) = refine_con(lib, [st], [pts], [cost], True, "min", 0.0, max_rounds=0)
        lib.check(rc)
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
        f, df = _values_and_gradients(st.host(True, "min", 0.0, graph_cost(cost)), pts)
        d_h, d_2h = np.empty_like(grad), np.empty_like(grad)
        for j in range(d):
            e = np.zeros(d)
            e[j] = FD_STEP
            fp, fm = mp_log_value(st, pts + e, "min", 0.0), mp_log_value(st, pts - e, "min", 0.0)
            fpp, fmm = mp_log_value(st, pts + 2 * e, "min", 0.0), mp_log_value(st, pts - 2 * e, "min", 0.0)
            d_h[:, j] = [float((a - b) / (2 * FD_STEP)) for a, b in zip(fp, fm)]
            d_2h[:, j] = [float((a - b) / (4 * FD_STEP)) for a, b in zip(fpp, fmm)]
        scale = np.max(np.abs(d_h), axis=1, keepdims=True)
        rel_fd = np.abs(grad - d_h) / scale
        rel_host = np.abs(grad - df) / scale
        host_fd = np.abs(df - d_h) / scale
        trunc = np.abs(d_2h - d_h) / 3.0 / scale
        richardson = (4.0 * d_h - d_2h) / 3.0                       # (the h^2 term removed: what is left is O(h^4) and rounding)
        print(f"far d{d}: gradient scale {scale.ravel().tolist()}\n  device - D_h {rel_fd.max():.3e}  device - host "
              f"{rel_host.max():.3e}  host - D_h {host_fd.max():.3e}  truncation estimate {trunc.max():.3e}\n  against the "
              f"extrapolated differences: device {(np.abs(grad - richardson) / scale).max():.3e}  host "
              f"{(np.abs(df - richardson) / scale).max():.3e}")
        worst_fd, worst_host = max(worst_fd, float(rel_fd.max())), max(worst_host, float(rel_host.max()))
        st.close()
    print(f"far: worst relative difference against the differences {worst_fd:.3e}, against the host class {worst_host:.3e}")
    assert worst_fd <= 4.0 * FAR_MEASURED_AGAINST_DIFFERENCES and worst_host <= 4.0 * FAR_MEASURED_AGAINST_HOST


# ------------------------------------------------------------------------------------------------------------ 3. searches
@pytest.mark.parametrize("log_form", [False, True])
@pytest.mark.parametrize("name", ["d1 n12 under n70", "d3 ard n17 under n70 n12 n128", "d8 n70 under eight"])
def test_every_start_ends_no_lower_inside_the_box_at_a_point_priced_the_same(lib, zoo, name, log_form):
    """A whole search per start: it ends not below its start and inside the box; value and gradient are bit for bit those of a
    fresh max_rounds = 0 evaluation at the end point; a second call gives the same bits.  The d = 3 and d = 8 sets carry a
    128-row constraint and search long enough to wrap the rings (more than twice their 8 pairs in rounds -- the log form at
    d = 8, both forms at d = 3): they end with a legal status."""
    st = zoo[name]
    pts, cost = st.points(STARTS[name]), variable_cost(st.d)
    rc, (res0,) = refine_con(lib, [st], [pts], [cost], log_form, "min", 0.0, max_rounds=0)
    lib.check(rc)
    rc, (res,) = refine_con(lib, [st], [pts], [cost], log_form, "min", 0.0)
    lib.check(rc)
    x, val, grad, rounds, status = res
    print(f"{name} log={log_form}: rounds {rounds.tolist()} status {status.tolist()}")
    legal = {lib.REFINE_PGTOL, lib.REFINE_FTOL, lib.REFINE_STEP, lib.REFINE_MAX_ROUNDS}
    assert set(status.tolist()) <= legal
    assert np.all(val >= res0[1]) and np.all(x >= st.lo) and np.all(x <= st.hi)
    rc, (again,) = refine_con(lib, [st], [pts], [cost], log_form, "min", 0.0)
    lib.check(rc)
    assert same(res, again)
    rc, (fresh,) = refine_con(lib, [st], [x], [cost], log_form, "min", 0.0, max_rounds=0)
    lib.check(rc)
    assert np.array_equal(bits(fresh[1]), bits(val)) and np.array_equal(bits(fresh[2]), bits(grad))
    # (the product of nine factors at a random point of the d = 8 box is below the search's pgtol: those searches end at once)
    if name == "d3 ard n17 under n70 n12 n128" or (name == "d8 n70 under eight" and log_form):
        assert rounds.max() > 2 * 8, rounds.tolist()
    assert unfitted(lib, st)


@pytest.mark.parametrize("log_form", [False, True])
def test_one_dimensional_sets_end_where_lockstep_lbfgs_ends(lib, zoo, log_form):
    """d = 1: the end value agrees with ``lockstep_lbfgs`` driven by the device's own max_rounds = 0 entry at rtol 1e-5
    (§4q's bar)."""
    from cbo_with_oop_amd.utils_functions.causal_optimizer import lockstep_lbfgs
    st = zoo["d1 n128 under n12"]
    pts, cost = st.points(5), variable_cost(1)

    def fun(X):
        rc, ((_, v, g, _, _),) = refine_con(lib, [st], [np.ascontiguousarray(X)], [cost], log_form, "min", 0.0, max_rounds=0)
        lib.check(rc)
        return v.copy(), g.copy()
    want_x, want_f = lockstep_lbfgs(fun, pts, st.lo, st.hi)
    rc, ((x, val, _, rounds, status),) = refine_con(lib, [st], [pts], [cost], log_form, "min", 0.0)
    lib.check(rc)
    print(f"log={log_form}: device {val.tolist()} lockstep {want_f.tolist()} rounds {rounds.tolist()}")
    assert np.allclose(val, want_f, rtol=1e-5, atol=1e-12)


def test_the_dead_region(lib):
    """§4aa's set (noise 1e-10, a bound -1e6 no point can meet): EI prod PoF and its gradient are exact zeros, the product
    form returns the start after 0 rounds with value 0.0; the log form has a value and a gradient, moves and ends higher."""
    st = ConSet(1, 40, [25, 33], seed=8, noise=1e-10, values=[0.3, -1e6])
    st.cons = [(n, v, j, LE) for n, v, j, _ in st.cons]
    start, cost = np.array([[0.7]]), fixed_cost(1)
    rc, ((x0, v0, g0, r0, s0),) = refine_con(lib, [st], [start], [cost], False, "min", 0.0)
    lib.check(rc)
    print("product form:", v0.tolist(), g0.tolist(), r0.tolist(), s0.tolist())
    assert np.array_equal(x0, start) and r0[0] == 0 and v0[0] == 0.0 and g0[0, 0] == 0.0 and s0[0] == lib.REFINE_PGTOL
    rc, ((_, v_start, g_start, _, _),) = refine_con(lib, [st], [start], [cost], True, "min", 0.0, max_rounds=0)
    lib.check(rc)
    rc, ((x, v, g, r, s),) = refine_con(lib, [st], [start], [cost], True, "min", 0.0)
    lib.check(rc)
    print("log form: start", v_start.tolist(), g_start.tolist(), "end", x.tolist(), v.tolist(), r.tolist(), s.tolist())
    assert np.isfinite(v_start[0]) and g_start[0, 0] != 0.0
    assert x[0, 0] != start[0, 0] and st.lo[0] <= x[0, 0] <= st.hi[0] and r[0] > 0 and v[0] > v_start[0]
    assert s[0] not in (lib.REFINE_NAN_START, lib.REFINE_DECLINED)
    st.close()


# ------------------------------------------------------------------------------------------------------------ 4. routing
def test_ineligible_sets_are_declined_between_eligible_neighbours_and_answered_by_the_host_route(lib, zoo):
    """A causal objective, a causal constraint, a 129-row constraint and an fp32 constraint, each between eligible
    neighbours: DECLINED with nothing else written, the neighbours' outputs their own calls' bit for bit; ``refine_sets``
    answers each declined set with ``refine_batched``'s own result.  A fitted neighbour keeps its likelihood, its cached
    sweep and its kept solution."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.utils_functions import CausalGradientAcquisitionOptimizer
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    from test_logei_gpu import mean_f, var_f
    good = zoo["d1 n12 under n70"]
    prior = dict(mean_function=mean_f, variance_adjustment=var_f)

    def variant(obj=None, con=None):
        st = ConSet(1, 12, [17], seed=9)
        if obj is not None:
            st.obj.close()
            st.obj = obj
        if con is not None:
            st.cons[0][0].close()
            st.cons[0] = (con,) + st.cons[0][1:]
        return st
    bad = [variant(obj=Node(12, 1, 20, **prior)), variant(con=Node(17, 1, 21, **prior)), variant(con=Node(129, 1, 22)),
           variant(con=Node(17, 1, 23, dtype="f32"))]
    # the fitted neighbour: a fitted objective with a kept solution and a cached sweep
    fitted = ConSet(1, 12, [17], seed=10)
    fitted.obj.model.close()
    fitted.obj.model = gp(fitted.obj.X, fitted.obj.y, **fitted.obj.kw)
    grid = CandidateGrid(fitted.points(40), fitted.obj.model, keep_solution=True)
    ei = CausalExpectedImprovement(0.1, "min", fitted.obj.model)
    before = ei.sweep(grid, cost=1.0, want_acq=True)
    lml_before, lml_after = np.empty(1), np.empty(1)
    assert lib.load().cbo_gp_log_marginal(fitted.obj.model._handle, lib.dptr(lml_before)) == 0

    sets = [good, bad[0], fitted, bad[1], good, bad[2], fitted, bad[3], good]
    starts = [st.points(3) for st in sets]
    costs = [variable_cost(1) for _ in sets]
    for log_form in (False, True):
        alone = {}
        for j in (0, 2, 4, 6, 8):
            rc, (alone[j],) = refine_con(lib, [sets[j]], [starts[j]], [costs[j]], log_form, "min", 0.0, sentinel=-77.0)
            lib.check(rc)
        rc, res = refine_con(lib, sets, starts, costs, log_form, "min", 0.0, sentinel=-77.0)
        lib.check(rc)
        for j, (x, val, grad, rounds, status) in enumerate(res):
            if j % 2:
                assert np.all(status == lib.REFINE_DECLINED), j
                assert np.all(x == -77.0) and np.all(val == -77.0) and np.all(grad == -77.0) and np.all(rounds == -77)
            else:
                assert same(res[j], alone[j]) and np.all(status != lib.REFINE_DECLINED), j
        # refine_sets: the declined sets through refine_batched, inside the same call
        kind = ("LOGCEI", 0.0) if log_form else ("EI", None)
        models = [st.obj.model for st in sets]
        boxes = [list(zip(st.lo.tolist(), st.hi.tolist())) for st in sets]
        gcosts = [graph_cost(c) for c in costs]
        y_best = good.y_best("min")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = refine_sets(models, starts, boxes, y_best, "min", gcosts, kind=kind,
                              constraints=[st.pofs(twins=False) for st in sets])
            for j in (1, 3, 5, 7):
                from cbo_with_oop_amd.utils_functions.causal_optimizer import _constrained_acquisition
                acq = _constrained_acquisition(kind, models[j], y_best, "min", gcosts[j], sets[j].pofs(twins=False))
                wx, wf = CausalGradientAcquisitionOptimizer(boxes[j]).refine_batched(acq, starts[j])
                assert np.all(out[j][2] == lib.REFINE_DECLINED)
                assert np.array_equal(bits(out[j][0]), bits(wx)) and np.array_equal(bits(out[j][1]), bits(wf)), j
        for j in (0, 2, 4, 6, 8):
            assert np.all(out[j][2] != lib.REFINE_DECLINED), j
    assert lib.load().cbo_gp_log_marginal(fitted.obj.model._handle, lib.dptr(lml_after)) == 0 and not fitted.obj.model.stale
    assert bits(lml_after)[0] == bits(lml_before)[0]
    after = ei.sweep(grid, cost=1.0, want_acq=True)
    assert np.array_equal(bits(before["acq"]), bits(after["acq"])) and before["best_idx"] == after["best_idx"]
    grid.close()
    assert unfitted(lib, good)
    for st in bad + [fitted]:
        st.close()


def test_a_constraint_that_is_not_positive_definite_declines_its_set_alone(lib, zoo):
    """The jitter fixture (duplicate rows under a negative noise) as a set's constraint model, between two ordinary sets: the
    set declines in the launch with nothing else written, the neighbours' outputs are their own calls' bit for bit."""
    f = load_fixture("jitter_ladder")
    first, last = zoo["d1 n12 under n70"], zoo["d1 n128 under n12"]
    mid = ConSet(1, 12, [17], seed=11)
    mid.cons[0][0].model.close()
    mid.cons[0][0].model = gp(f["X"], f["y"], fit=False, variance=float(f["variance"]), lengthscale=f["lengthscale_arg"],
                              noise_var=float(f["noise_var"]))
    sets = [first, mid, last]
    starts = [st.points(3) for st in sets]
    costs = [variable_cost(1)] * 3
    for log_form in (False, True):
        alone = []
        for j in (0, 2):
            rc, (r,) = refine_con(lib, [sets[j]], [starts[j]], [costs[j]], log_form, "min", 0.0, sentinel=-77.0)
            lib.check(rc)
            alone.append(r)
        rc, res = refine_con(lib, sets, starts, costs, log_form, "min", 0.0, sentinel=-77.0)
        lib.check(rc)
        assert same(res[0], alone[0]) and same(res[2], alone[1])
        x, val, grad, rounds, status = res[1]
        assert np.all(status == lib.REFINE_DECLINED) and np.all(x == -77.0) and np.all(val == -77.0) and np.all(rounds == -77)
    mid.close()


# ------------------------------------------------------------------------------------------------------------ 5. top layers
@pytest.mark.parametrize("acquisition", ["EI", "LOGCEI"])
@pytest.mark.parametrize("cost_type", [1, 4])
def test_find_next_y_points_refines_every_constrained_winner(lib, cost_type, acquisition):
    """The toy graph's two sets under one constraint each: ``refine_constrained=True`` never returns a lower value than
    without it, and returns the per-set ``optimize(acquisition / Cost, refine=True, device=True)`` result."""
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost,
                                                  ProbabilityOfFeasibility, find_next_y_points)
    from cbo_with_oop_amd.utils_functions.constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement
    from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement
    rng = np.random.default_rng(3)
    es = ToyGraph.get_exploration_set("MIS")
    xs = [rng.uniform(-5, 5, (14, 1)), rng.uniform(-5, 20, (14, 1))]
    ys = [ToyGraph.target_do_x(xs[0]), ToyGraph.target_do_z(xs[1])]
    cs = [np.sin(0.4 * x) + 0.1 * x for x in xs]
    kw = dict(variance=1.0, lengthscale=1.5, noise_var=1e-3)
    models = [gp(x, y, fit=False, **kw) for x, y in zip(xs, ys)]
    con_models = [gp(x, c, fit=False, **kw) for x, c in zip(xs, cs)]
    spaces = [ToyGraph.bounds(s) for s in es]
    costs = ToyGraph.get_cost_structure(cost_type)
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    grids = [CandidateGrid(meshgrid_candidates(sp, [9]), m) for sp, m in zip(spaces, models)]
    constraints = [[ProbabilityOfFeasibility(cm, max_value=0.4)] for cm in con_models]
    y_best = min(float(y.min()) for y in ys) + 0.2
    args = (models, y_best, es, costs, "min", grids)
    x_grid, y_grid = find_next_y_points(*args, acquisition=acquisition, constraints=constraints)
    x_ref, y_ref = find_next_y_points(*args, acquisition=acquisition, refine_constrained=True, spaces=spaces,
                                      constraints=constraints)
    for s in range(2):
        assert y_ref[s][0, 0] >= y_grid[s][0, 0]
        if acquisition == "EI":
            num = AcquisitionProduct([CausalExpectedImprovement(y_best, "min", models[s])] + constraints[s])
        else:
            num = ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(y_best, "min", models[s]), constraints[s])
        opt = CausalGradientAcquisitionOptimizer(spaces[s], grid_shape=[9])
        x_one, f_one = opt.optimize(num / Cost(costs, es[s]), refine=True, device=True)
        print(f"{acquisition} cost {cost_type} set {s}: grid {x_grid[s].tolist()} {y_grid[s].tolist()} refined "
              f"{x_ref[s].tolist()} {y_ref[s].tolist()} optimize {x_one.tolist()} {f_one.tolist()}")
        assert np.allclose(x_ref[s], x_one, rtol=0, atol=1e-12) and np.isclose(y_ref[s][0, 0], f_one[0, 0], rtol=1e-12, atol=1e-300)
    for o in grids + models + con_models:
        o.close()


def test_the_agent_intervenes_off_the_grid_under_constraints(lib):
    """CBO(acquisition="LOGCEI", constraints={"C": ("<=", 2.0)}, refine_constrained=True) for four trials: at least one
    intervention is off the grid and ``feasible`` is recorded."""
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import CompleteGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions.graph_functions import compute_interventions, sample_from_model
    sem = CompleteGraph.define_sem()
    rng = np.random.default_rng(11)
    rows = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(60)]
    obs = {v: np.array([r[v] for r in rows]) for v in rows[0] if not v.startswith("U")}
    init = {k: v[:40] for k, v in obs.items()}
    es = [["B"], ["D"], ["B", "D"]]
    shapes = [[16], [16], [6, 6]]
    data = []
    for s_ in es:
        lo, hi = np.array(CompleteGraph.bounds(s_)).T
        x = rng.uniform(lo, hi, (5, len(s_)))
        data.append((x, compute_interventions(sem, {v: "" for v in s_}, x, target_variable="Y")))
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(CompleteGraph, init, obs, data, exploration_set=es, num_trials=4, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=shapes, acquisition="LOGCEI",
                    constraints={"C": ("<=", 2.0)}, refine_constrained=True)
        assert agent.refine_constrained is True and agent.refine is False
        mon = agent.run()
    assert len(mon.feasible) == 4
    chosen = [c for c in mon.chosen if c is not None]
    assert chosen and all(f is not None for f, k in zip(mon.feasible, mon.type_trial) if k == 1)
    off = 0
    for picked_set, picked_x in chosen:
        j = es.index(list(picked_set))
        grid = meshgrid_candidates(CompleteGraph.bounds(es[j]), shapes[j])
        lo, hi = np.array(CompleteGraph.bounds(es[j])).T
        assert np.all(picked_x >= lo) and np.all(picked_x <= hi)
        off += int(np.min(np.abs(grid - np.asarray(picked_x).reshape(1, -1)).max(1)) > 1e-9)
    print("interventions:", [(list(a), np.asarray(b).tolist()) for a, b in chosen], "off the grid:", off)
    assert off >= 1
