"""Per-candidate intervention costs, what needs no GPU: ``PointwiseCost`` against ``one_row_cost``, the quotient
rule of both quotients against central differences of their own values on a stub model, the argument checks of the Python
layers and of the library, the pins of the ABI, and the arg-max example of the design section on a numpy restatement."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import scipy.special as sp

from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib, graphs
from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, Cost, PointCostQuotient, PointwiseCost,
                                               ProbabilityOfFeasibility, find_next_y_point, find_next_y_points)
from cbo_with_oop_amd.utils_functions.causal_optimizer import (CausalGradientAcquisitionOptimizer, _values_and_gradients,
                                                                one_row_cost, refine_sets)
from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement, CausalProbabilityOfImprovement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cbo_cands_set_cost", "cbo_cands_get_cost", "cbo_cands_clear_cost", "cbo_acq_sweep_pointcost",
               "cbo_acq_sweep_sets_pointcost", "cbo_acq_refine_sets_pointcost")


def table(*entries):
    names = ["X", "Z", "W"][:len(entries)]
    return {n: functools.partial(graphs.cost, f, v) for n, (f, v) in zip(names, entries)}, names


def test_pointwise_cost_is_one_row_cost_row_by_row_and_its_gradient_is_the_sign():
    rng = np.random.default_rng(0)
    for entries in (((1, True),), ((2, True), (3, False), (0.5, True))):
        funcs, names = table(*entries)
        cost = PointwiseCost(funcs, names)
        x = rng.uniform(-5, 5, (17, len(names)))
        x[3, 0] = 0.0
        x[5] = -np.abs(x[5])
        got = cost.evaluate(x)
        assert got.shape == (17, 1)
        fix = np.array([float(f) for f, _ in entries])
        variable = np.array([1 if v else 0 for _, v in entries], dtype=np.int32)
        assert cost.fix.tolist() == fix.tolist() and cost.variable.tolist() == variable.tolist()
        for i in range(17):
            assert got[i, 0] == one_row_cost(fix, variable, x[i])
            # ... which is Cost.evaluate of the one-row batch
            assert got[i, 0] == float(Cost(funcs, names).evaluate(x[i:i + 1]))
        c, dc = cost.evaluate_with_gradients(x)
        assert c.tobytes() == got.tobytes() and dc.shape == x.shape
        assert np.array_equal(dc, variable[None, :] * np.sign(x))
        assert dc[3, 0] == 0.0                                         # sign(0) = 0
    nan = PointwiseCost(*table((1, True))).evaluate(np.array([[np.nan]]))
    assert np.isnan(nan[0, 0])


def test_a_cost_the_structure_does_not_recognise_is_refused():
    with pytest.raises(ValueError, match="PointwiseCost"):
        PointwiseCost({"X": lambda col: 1.0}, ["X"])
    with pytest.raises(ValueError, match="PointwiseCost"):
        PointwiseCost({"X": functools.partial(graphs.cost, 1)}, ["X"])
    with pytest.raises(ValueError, match="positive"):
        PointwiseCost(*table((0, True)))


class StubModel:
    """A smooth posterior with known gradients: mean = sin x0 + x1 / 2, variance = 0.3 + 0.2 cos(x0 x1)^2."""
    causal = False

    def predict(self, x):
        x = np.asarray(x)
        return (np.sin(x[:, :1]) + 0.5 * x[:, 1:2]), 0.3 + 0.2 * np.cos(x[:, :1] * x[:, 1:2]) ** 2

    def get_prediction_gradients(self, x):
        x = np.asarray(x)
        dm = np.hstack([np.cos(x[:, :1]), np.full((x.shape[0], 1), 0.5)])
        p = x[:, :1] * x[:, 1:2]
        g = -0.4 * np.cos(p) * np.sin(p)
        return dm, np.hstack([g * x[:, 1:2], g * x[:, :1]])


def host_value(quotient, x):
    """The quotient's own value from its numerator's host formula (the device-free half of ``evaluate_with_gradients``)."""
    return quotient.evaluate_with_gradients(x)[0]


@pytest.mark.parametrize("log_form", [False, True])
@pytest.mark.parametrize("task", ["min", "max"])
def test_the_quotient_rule_against_central_differences(log_form, task):
    funcs, names = table((2, True), (3, False))
    cost = PointwiseCost(funcs, names)
    model = StubModel()
    num = (CausalLogExpectedImprovement(0.4, task, model) if log_form else CausalExpectedImprovement(0.4, task, model))
    if log_form:
        num._posterior_and_gradients = lambda x: _posterior(model, x)
    q = num / cost
    assert type(q) is PointCostQuotient and q.is_log is log_form and q.has_gradients and q.pointwise_cost
    X = np.array([[0.7, -1.2], [-1.5, 0.4], [2.0, 1.0], [-0.3, -0.8]])
    f, df = q.evaluate_with_gradients(X)
    assert f.shape == (4, 1) and df.shape == (4, 2)
    h = 1e-6
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        fd = (host_value(q, X + e) - host_value(q, X - e))[:, 0] / (2 * h)
        assert np.allclose(df[:, k], fd, rtol=2e-7, atol=2e-9), (k, df[:, k], fd)
    # the true cost gradient is in it: with the reference's zero gradient column 0 (the variable one) would differ
    c, dc = cost.evaluate_with_gradients(X)
    assert np.all(dc[:, 0] != 0.0) and np.all(dc[:, 1] == 0.0)
    nf, ndf = num.evaluate_with_gradients(X)
    zero_rule = ndf if log_form else ndf / c
    assert np.allclose(df[:, 1], zero_rule[:, 1], rtol=1e-14) and not np.allclose(df[:, 0], zero_rule[:, 0], rtol=1e-3)
    # the lockstep searches take the quotient's own rows
    vals, grads = _values_and_gradients(q, X)
    assert vals.tobytes() == f[:, 0].tobytes() and grads.tobytes() == df.tobytes()
    # at x_k = 0 of a variable column the cost's derivative is 0
    X0 = np.array([[0.0, 0.5]])
    _, d0 = q.evaluate_with_gradients(X0)
    n0f, n0d = num.evaluate_with_gradients(X0)
    c0 = cost.evaluate(X0)
    assert np.allclose(d0, n0d if log_form else n0d / c0, rtol=1e-15)


def _posterior(model, x):
    mean, var = model.predict(x)
    sd = np.sqrt(var)
    dm, dv = model.get_prediction_gradients(x)
    return mean, sd, dm, dv / (2 * sd)


def test_only_the_ei_and_its_logarithm_divide_by_a_pointwise_cost():
    cost = PointwiseCost(*table((1, True)))
    with pytest.raises(ValueError, match="PointwiseCost"):
        PointCostQuotient(CausalProbabilityOfImprovement(0.0, "min", None), cost)
    with pytest.raises(ValueError, match="PointwiseCost"):
        PointCostQuotient(CausalExpectedImprovement(0.0, "min", None), Cost(*table((1, True))))
    with pytest.raises(ValueError, match="batch"):
        (CausalExpectedImprovement(0.0, "min", None) / cost).sweep_batch(None, 2)


def test_refused_combinations_raise_before_the_library_is_loaded(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the object was asked for {name!r}")

    class Model:
        def __init__(self, handle):
            self._handle = ctypes.c_void_p(handle)
            self.small, self.stale, self.causal, self.input_dim = True, True, False, 1

    obj = Untouchable()
    models = [Model(11), Model(12)]
    boxes = [[(-1.0, 1.0)], [(-2.0, 2.0)]]
    good, _ = table((1, True), (1, True))
    sweep = lambda **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], good, "min", [obj, obj],      # noqa: E731
                                            cost_mode="pointwise", **kw)
    for name in ("LCB", "PI", "MPEI", "VAR"):
        with pytest.raises(ValueError, match="acquisition"):
            sweep(acquisition=name)
    with pytest.raises(ValueError, match="acquisition"):
        sweep(acquisition="MES", acquisition_param=(4, 50), spaces=boxes)
    for acquisition in ("EI", "LOGEI"):
        with pytest.raises(ValueError, match="constraints"):
            sweep(acquisition=acquisition, constraints=[[ProbabilityOfFeasibility(obj)], []])
        with pytest.raises(ValueError, match="hyper"):
            sweep(acquisition=acquisition, hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
        with pytest.raises(ValueError, match="batch"):
            sweep(acquisition=acquisition, batch_size=2)
        with pytest.raises(ValueError, match="device_prior"):
            sweep(acquisition=acquisition, refine=True, spaces=boxes, device_prior=True)
        with pytest.raises(ValueError, match="raw"):
            sweep(acquisition=acquisition, raw=True)
        with pytest.raises(ValueError, match="spaces"):
            sweep(acquisition=acquisition, refine=True)
        with pytest.raises(ValueError, match="PointwiseCost"):
            find_next_y_points(models, 0.0, [["X"], ["Z"]], {"X": abs, "Z": abs}, "min", [obj, obj], acquisition=acquisition,
                               cost_mode="pointwise")
    with pytest.raises(ValueError, match="cost_mode"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], good, "min", [obj, obj], cost_mode="point")
    # the single-set function
    single = lambda **kw: find_next_y_point(obj, obj, 0.0, ["X"], good, cost_mode="pointwise", **kw)      # noqa: E731
    with pytest.raises(ValueError, match="acquisition"):
        single(acquisition="LCB")
    with pytest.raises(ValueError, match="constraints"):
        single(constraints=[ProbabilityOfFeasibility(obj)])
    with pytest.raises(ValueError, match="hyper"):
        single(hyper_samples=4)
    with pytest.raises(ValueError, match="batch"):
        single(batch_size=2)
    with pytest.raises(ValueError, match="PointwiseCost"):
        find_next_y_point(obj, obj, 0.0, ["X"], {"X": abs}, cost_mode="pointwise")
    with pytest.raises(ValueError, match="cost_mode"):
        find_next_y_point(obj, obj, 0.0, ["X"], good, cost_mode=None)
    # the path and the agent
    path = lambda **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], good, "min", [obj, obj], [obj, obj], boxes,  # noqa: E731
                                                      comm=None, cost_mode="pointwise", **kw)
    col = np.zeros((3, 1))
    with pytest.raises(ValueError, match="acquisition"):
        path(acquisition="PI")
    with pytest.raises(ValueError, match="constraints"):
        path(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    with pytest.raises(ValueError, match="hyper"):
        path(hyper_samples=4)
    with pytest.raises(ValueError, match="batch"):
        path(batch_size=3)
    with pytest.raises(ValueError, match="device_prior"):
        path(refine=True, device_prior=True)
    with pytest.raises(ValueError, match="PointwiseCost"):
        cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], {"X": abs, "Z": abs}, "min", [obj, obj], [obj, obj], boxes,
                                      comm=None, cost_mode="pointwise")
    assert path().cost_mode == "pointwise" and path(acquisition="LOGEI", refine=True).cost_mode == "pointwise"

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], good, "min", [obj, obj], [obj, obj], boxes, comm=Two(),
                                          cost_mode="pointwise")
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data,      # noqa: E731
                                       cost_mode="pointwise", **kw)
    with pytest.raises(ValueError, match="acquisition"):
        make(acquisition="VAR")
    with pytest.raises(ValueError, match="batch"):
        make(batch_size=3)
    with pytest.raises(ValueError, match="hyper"):
        make(hyper_samples=5)
    with pytest.raises(ValueError, match="constraints"):
        make(constraints={"C": ("<=", 1.0)})
    with pytest.raises(ValueError, match="device_prior"):
        make(refine=True, device_prior=True)
    # refine_sets and the optimiser
    cost = Cost(*table((1, True)))
    with pytest.raises(ValueError, match="device_prior"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [cost], device_prior=True, cost_mode="pointwise")
    with pytest.raises(ValueError, match="acquisition"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [cost], kind=("LCB", 1.0), cost_mode="pointwise")
    with pytest.raises(ValueError, match="PointwiseCost"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [Cost({"X": abs}, ["X"])], cost_mode="pointwise")
    opt = CausalGradientAcquisitionOptimizer(boxes[0], grid_shape=[5])
    with pytest.raises(ValueError, match="cost_mode"):
        opt.optimize(CausalExpectedImprovement(0.0, "min", None) / cost, refine=True, device=True, cost_mode="pointwise")
    with pytest.raises(ValueError, match="cost_mode"):
        opt.optimize(CausalExpectedImprovement(0.0, "min", None) / PointwiseCost(*table((1, True))), refine=True, device=True)


def test_every_default_is_todays():
    for fn in (find_next_y_point, find_next_y_points, refine_sets, CausalGradientAcquisitionOptimizer.optimize,
               cbo_module.CBOAcquisitionPath.__init__, cbo_module.CBO.__init__):
        assert inspect.signature(fn).parameters["cost_mode"].default == "batch", fn
    built = CausalExpectedImprovement(0.0, "min", None) / Cost(*table((1, True)))
    assert type(built).__name__ == "AcquisitionQuotient"
    built = CausalLogExpectedImprovement(0.0, "min", None) / Cost(*table((1, True)))
    assert type(built).__name__ == "LogAcquisitionQuotient"


def test_the_kind_tables_and_the_abi_version_are_what_they_were():
    assert _lib.ACQ_KIND_CODE == {"LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.REFINE_KIND_CODE == {"EI": 0, "LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_the_entry_points_are_declared_exported_and_prototyped(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cbo_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, f"{name} not declared in include/cbo_hip.h"
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(decl.group(1).split(","))
    assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"


def test_the_sweeps_are_their_siblings_argument_lists_with_log_form_and_without_cost():
    sig = _lib.SIGNATURES
    single = list(sig["cbo_acq_sweep_logei"][1])
    single.pop(5)                                   # cost
    single.insert(2, ctypes.c_int)                  # log_form
    assert list(sig["cbo_acq_sweep_pointcost"][1]) == single
    sets = list(sig["cbo_acq_sweep_sets_logei"][1])
    sets.pop(6)                                     # costs
    sets.insert(3, ctypes.c_int)
    assert list(sig["cbo_acq_sweep_sets_pointcost"][1]) == sets
    refine = list(sig["cbo_acq_refine_sets_logei"][1])
    refine.insert(3, ctypes.c_int)
    assert list(sig["cbo_acq_refine_sets_pointcost"][1]) == refine


def test_the_library_refuses_null_handles_and_bad_scalars():
    lib = _lib.load()
    out, ints = np.zeros(4), np.zeros(4, dtype=np.int32)
    idx = np.zeros(4, dtype=np.int64)
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)      # noqa: E731
    refused = lambda rc, word: rc == _lib.CBO_ERR_INVALID and word in lib.cbo_last_error()      # noqa: E731

    def single(log_form=0, y_best=0.5, task=0, jitter=0.0):
        return lib.cbo_acq_sweep_pointcost(None, None, log_form, y_best, task, jitter, None, None, None, None, None)

    def sets(n_sets=1, log_form=0, y_best=0.5, task=0, jitter=0.0, y=True):
        return lib.cbo_acq_sweep_sets_pointcost(n_sets, None, None, log_form, _lib.dptr(np.array([y_best])) if y else None,
                                                task, jitter, _lib.dptr(out), idx.ctypes.data_as(_lib.c_int64_p))

    def refine(n_sets=1, log_form=0, y_best=0.5, task=0, jitter=0.0, y=True):
        return lib.cbo_acq_refine_sets_pointcost(n_sets, None, None, log_form, _lib.dptr(np.array([y_best])) if y else None,
                                                 task, jitter, 10, _lib.dptr(out), _lib.dptr(out), _lib.dptr(out), ip(ints),
                                                 ip(ints))

    assert refused(single(), b"NULL") and refused(sets(), b"argument") and refused(refine(), b"NULL")
    for call in (single, sets, refine):
        for log_form in (0, 1):
            assert refused(call(log_form=log_form, y_best=np.nan), b"y_best"), call.__name__
            assert refused(call(log_form=log_form, y_best=np.inf), b"y_best"), call.__name__
            assert refused(call(log_form=log_form, jitter=np.inf), b"jitter"), call.__name__
            assert refused(call(log_form=log_form, jitter=np.nan), b"jitter"), call.__name__
            assert refused(call(log_form=log_form, task=2), b"task") and refused(call(log_form=log_form, task=-1), b"task")
        assert refused(call(log_form=2), b"log_form") and refused(call(log_form=-1), b"log_form"), call.__name__
    assert refused(sets(n_sets=0), b"n_sets") and refused(sets(y=False), b"y_best")
    assert refused(refine(n_sets=0), b"n_sets") and refused(refine(y=False), b"y_best")
    one, flag = np.array([1.0]), np.array([1], dtype=np.int32)
    assert refused(lib.cbo_cands_set_cost(None, _lib.dptr(one), ip(flag)), b"NULL")
    assert refused(lib.cbo_cands_get_cost(None, _lib.dptr(out)), b"NULL")
    assert refused(lib.cbo_cands_clear_cost(None), b"NULL")
    # the siblings keep refusing the internal kind codes
    for kind in (8, 9):
        assert lib.cbo_acq_sweep_kind(None, None, kind, 0.5, 0, 0.0, 1.0, None, None, None, None, None) == _lib.CBO_ERR_INVALID
        assert b"kind" in lib.cbo_last_error()
        gps = (ctypes.c_void_p * 1)(None)
        sets_arr = (_lib.CboRefineSet * 1)()
        y = _lib.dptr(np.array([0.5]))
        assert lib.cbo_acq_refine_sets(1, gps, sets_arr, kind, y, 0, 0.0, 10, _lib.dptr(out), _lib.dptr(out), _lib.dptr(out),
                                       ip(ints), ip(ints)) == _lib.CBO_ERR_INVALID
        assert b"kind" in lib.cbo_last_error()


# ---- the arg-max example of DESIGN.md §4y: a numpy restatement of the posterior and of EI

def _posterior_numpy(X, Y, grid, variance=1.0, lengthscale=1.0, noise=1e-4):
    def k(a, b):
        return variance * np.exp(-0.5 * ((a[:, None, 0] - b[None, :, 0]) / lengthscale) ** 2)
    L = np.linalg.cholesky(k(X, X) + noise * np.eye(len(X)))
    V = np.linalg.solve(L, k(X, grid))
    mean = V.T @ np.linalg.solve(L, Y[:, 0])
    var = np.clip(variance - np.sum(V * V, axis=0), 1e-15, None) + noise
    return mean, var


def ei_numpy(mean, var, y_best):
    s = np.sqrt(var)
    u = (y_best - mean) / s
    return s * (u * sp.ndtr(u) + np.exp(-u * u / 2) * 0.3989422804014327)


def example(n, seed):
    X = np.random.default_rng(seed).uniform(-5, 20, (n, 1))
    Y = np.cos(X) - np.exp(-X / 20)
    grid = np.linspace(-5, 20, 200)[:, None]
    return X, Y, grid


@pytest.mark.parametrize("n, seed, plain, priced", [(12, 7, 65, 64), (17, 3, 14, 15), (50, 7, 14, 15)])
def test_the_argmax_moves_when_every_candidate_is_priced_at_its_own_cost(n, seed, plain, priced):
    X, Y, grid = example(n, seed)
    ei = ei_numpy(*_posterior_numpy(X, Y, grid), float(Y.min()))
    cost = PointwiseCost(*table((1, True))).evaluate(grid)[:, 0]
    assert cost.tolist() == (1.0 + np.abs(grid[:, 0])).tolist()
    assert int(np.argmax(ei)) == plain and int(np.argmax(ei / cost)) == priced
    if (n, seed) == (12, 7):
        q = np.sort(ei / cost)
        assert (q[-1] - q[-2]) / q[-1] > 1e-2                          # 1.8e-2: nothing a rounding could turn
