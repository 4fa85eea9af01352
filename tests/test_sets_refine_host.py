"""CPU tests of the gradient refinement of every set in one launch: the search logic of
csrc/refine_search.h driven on the host by tests/support/refine_search_sim.cpp (g++, no HIP) against ``lockstep_lbfgs``,
the entry point's declaration and binding, the argument checks of the Python layers, and the cost helper."""
import ctypes
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility, find_next_y_points
from cbo_with_oop_amd.utils_functions.causal_optimizer import (cost_structure, lockstep_lbfgs, one_row_cost,
                                                                refine_sets)
from cbo_with_oop_amd.utils_functions.cost_functions import Cost

CODES = (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP, _lib.REFINE_MAX_ROUNDS, _lib.REFINE_NAN_START)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """run(d, lo, hi, x0, kind, extra, max_rounds=200, nan_round=0) -> (evaluated points [(x, value, accepted)], status,
    rounds, value, x, gradient) of one search of the state machine, every number exchanged as a hexadecimal float."""
    exe = tmp_path_factory.mktemp("refine_sim") / "refine_search_sim"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbo_with_oop_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "refine_search_sim.cpp"), "-o", str(exe)])
    hexes = lambda a: " ".join(float(v).hex() for v in np.ravel(a))                                  # noqa: E731

    def run(d, lo, hi, x0, kind, extra="", max_rounds=200, nan_round=0):
        text = f"{d} {max_rounds} {nan_round}\n{hexes(lo)}\n{hexes(hi)}\n{hexes(x0)}\n{kind} {extra}\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.returncode, out.stderr)
        points, end = [], None
        for line in out.stdout.splitlines():
            tok = line.split()
            if tok[0] == "P":
                v = [float.fromhex(t) for t in tok[1:-1]]
                points.append((np.array(v[:d]), v[d], tok[-1] == "1"))
            else:
                v = [float.fromhex(t) for t in tok[3:]]
                end = (int(tok[1]), int(tok[2]), v[0], np.array(v[1:1 + d]), np.array(v[1 + d:1 + 2 * d]))
        return (points,) + end
    run.hexes = hexes
    return run


# dyadic centres, starts and boxes: every product, sum and quotient of the searches below is exact in binary64
QUADRATICS = [
    (1, [0.5], [-3.5], [-4.0], [4.0]),                      # |pg| = 4: first step 1/4, then the Newton step
    (1, [0.25], [0.75], [-1.0], [1.0]),                     # |pg| <= 1: the first step lands on the optimum
    (1, [6.0], [1.0], [-4.0], [4.0]),                       # the optimum beyond the upper bound
    (2, [0.5, -1.25], [4.5, 2.75], [-8.0, -8.0], [8.0, 8.0]),
    (2, [3.0, -6.0], [0.0, 0.0], [-2.0, -2.0], [2.0, 2.0]),  # beyond a corner
    (2, [0.25, 9.0], [-3.75, 1.0], [-4.0, -4.0], [4.0, 4.0]),   # one coordinate free, one clipped
]


@pytest.mark.parametrize("d,c,x0,lo,hi", QUADRATICS)
def test_the_state_machine_follows_lockstep_lbfgs_round_for_round_on_a_dyadic_quadratic(sim, d, c, x0, lo, hi):
    c = np.array(c)
    trials = []

    def fun(X):
        trials.append(X[0].copy())
        return -0.5 * ((X - c) ** 2).sum(1), -(X - c)

    X, F = lockstep_lbfgs(fun, np.array([x0]), np.array(lo), np.array(hi))
    points, status, rounds, value, x, grad = sim(d, lo, hi, x0, "quad", sim.hexes(c))
    assert len(points) == len(trials) and rounds == len(trials) - 1
    for (p, v, _), t in zip(points, trials):
        assert np.array_equal(p, t)                         # the same point evaluated in every round, to the bit
        assert v == -0.5 * ((t - c) ** 2).sum()
    assert np.array_equal(x, X[0]) and value == F[0]
    assert status == _lib.REFINE_PGTOL
    assert np.array_equal(grad, -(x - c))


def test_an_optimum_outside_the_box_ends_on_the_bound_with_zero_projected_gradient(sim):
    for d, c, x0, lo, hi in QUADRATICS[2:3] + QUADRATICS[4:]:
        _, status, _, _, x, grad = sim(d, lo, hi, x0, "quad", sim.hexes(c))
        lo, hi, c = np.array(lo), np.array(hi), np.array(c)
        assert np.array_equal(x, np.clip(c, lo, hi)) and status == _lib.REFINE_PGTOL
        # (the gradient of the maximised function: what points out of the box at an active bound is projected away)
        pg = np.where(((x >= hi) & (grad > 0)) | ((x <= lo) & (grad < 0)), 0.0, grad)
        assert np.all(pg == 0.0) and np.any(grad != 0.0)
    # a start already on the active bound stays there without a round
    points, status, rounds, _, x, _ = sim(1, [-4.0], [4.0], [4.0], "quad", sim.hexes([6.0]))
    assert (status, rounds, len(points)) == (_lib.REFINE_PGTOL, 0, 1) and x[0] == 4.0


def test_the_multi_modal_function_of_the_lockstep_test(sim):
    """tests/test_host_logic.py's function and starts: values never decrease from accepted point to accepted point, the end
    point lies in the box, the status is one of the codes, a PGTOL end has a projected gradient of at most 1e-5 -- and the
    end value is lockstep_lbfgs's own (the same iteration in another language: libm's exp is the only difference)."""
    rng = np.random.default_rng(0)
    C, W = rng.uniform(-3, 3, (6, 2)), rng.uniform(0.5, 2, 6)

    def fun(X):
        dd = X[:, None, :] - C[None]
        e = W * np.exp(-0.5 * (dd ** 2).sum(-1))
        return e.sum(1), -(e[:, :, None] * dd).sum(1)

    lo, hi = np.array([-3.0, -2.0]), np.array([3.0, 2.5])
    x0 = rng.uniform(lo, hi, (8, 2))
    X, F = lockstep_lbfgs(fun, x0, lo, hi)
    extra = f"6 {sim.hexes(C)} {sim.hexes(W)}"
    seen = set()
    for i in range(8):
        points, status, rounds, value, x, grad = sim(2, lo, hi, x0[i], "gauss", extra)
        assert status in CODES and status != _lib.REFINE_NAN_START and rounds <= 200
        seen.add(status)
        assert np.all(x >= lo) and np.all(x <= hi)
        # the accepted points -- the start, then every trial that passed the Armijo test -- never decrease in value, and
        # the search ends on the last of them (a rejected trial may lie above or below: it is not looked at)
        accepted = [(p, v) for p, v, ok in points if ok]
        assert points[0][2] and len(accepted) >= 1
        assert all(b[1] >= a[1] for a, b in zip(accepted, accepted[1:]))
        assert value == accepted[-1][1] and np.array_equal(x, accepted[-1][0]) and value >= points[0][1]
        assert np.isclose(value, fun(x[None])[0][0], rtol=1e-14)
        if status == _lib.REFINE_PGTOL:
            pg = np.where(((x >= hi) & (grad > 0)) | ((x <= lo) & (grad < 0)), 0.0, grad)
            assert np.max(np.abs(pg)) <= 1e-5
        assert np.isclose(value, F[i], rtol=1e-9), (i, value, F[i])
    assert _lib.REFINE_PGTOL in seen or _lib.REFINE_FTOL in seen
    # a bounded number of rounds ends a search that has not converged
    _, status, rounds, _, _, _ = sim(2, lo, hi, x0[0], "gauss", extra, max_rounds=2)
    assert (status, rounds) == (_lib.REFINE_MAX_ROUNDS, 2)
    points, status, rounds, _, x, _ = sim(2, lo, hi, x0[0], "gauss", extra, max_rounds=0)
    assert status == _lib.REFINE_MAX_ROUNDS and rounds == 0 and len(points) == 1 and np.array_equal(x, x0[0])


def test_non_finite_values(sim):
    # a NaN trial value is an Armijo failure: the next trial is half as far from the accepted point, which has not moved
    c, x0, lo, hi = [0.5], [-3.5], [-4.0], [4.0]
    clean = sim(1, lo, hi, x0, "quad", sim.hexes(c))[0]
    points, status, rounds, value, x, _ = sim(1, lo, hi, x0, "quad", sim.hexes(c), nan_round=1)
    assert np.isnan(points[1][1]) and points[1][0] == clean[1][0]
    assert points[0][2] and not points[1][2] and points[2][2]      # the start and the halved step accepted, the NaN trial not
    assert points[2][0][0] - x0[0] == 0.5 * (points[1][0][0] - x0[0])
    assert status == _lib.REFINE_PGTOL and x[0] == 0.5 and value == 0.0 and rounds == len(points) - 1
    # a NaN start: the start comes back, no round is spent
    points, status, rounds, value, x, _ = sim(2, [-1.0, -1.0], [1.0, 1.0], [0.25, 2.0], "nan")
    assert status == _lib.REFINE_NAN_START and rounds == 0 and len(points) == 1
    assert np.array_equal(x, [0.25, 1.0]) and np.isnan(value)       # (the start, clipped to the box)
    # NaN at every trial after a finite start: the step halves until t max|d| < 1e-14, the start is kept
    points, status, rounds, value, x, _ = sim(1, lo, hi, x0, "quad", sim.hexes(c), max_rounds=1000, nan_round=-1)
    assert status == _lib.REFINE_STEP and x[0] == x0[0] and value == -8.0
    steps = [p[0][0] - x0[0] for p in points[1:61]]
    assert all(b == 0.5 * a for a, b in zip(steps, steps[1:]) if b != 0.0)
    assert rounds == len(points) - 1 and 40 <= rounds <= 60            # 1/4 * 4 * 2^-r < 1e-14 at r = 47


def test_the_header_is_plain_cxx_and_states_the_reference_constants():
    text = open(os.path.join(ROOT, "cbo_with_oop_amd", "csrc", "refine_search.h")).read()
    assert "hip/" not in text and "#include \"cbo_hip.h\"" in text
    for word in ("kRefineHistory = 8", "kRefinePgtol = 1e-5", "kRefineFtol = 2.2e-9", "kRefineC1 = 1e-4",
                 "kRefineMinStep = 1e-14", "kRefineCurvature = 1e-12", "__host__ __device__"):
        assert word in text, word


def test_the_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+cbo_acq_refine_sets\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, "cbo_acq_refine_sets not declared in include/cbo_hip.h"
    assert len(decl.group(1).split(",")) == 13
    assert re.search(r"typedef\s+struct\s+cbo_refine_set\s*\{", text)
    assert hasattr(_lib.load(), "cbo_acq_refine_sets"), "not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES["cbo_acq_refine_sets"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert [n for n, _ in _lib.CboRefineSet._fields_] == ["k", "starts", "lo", "hi", "cost_fix", "cost_variable"]
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5
    assert _lib.REFINE_MAX_STARTS == 64 and re.search(r"#define\s+CBO_REFINE_MAX_STARTS\s+64\b", text)
    assert _lib.REFINE_ROUNDS_LIMIT == 1000 and re.search(r"#define\s+CBO_REFINE_ROUNDS_LIMIT\s+1000\b", text)
    enum = re.search(r"enum\s*\{\s*CBO_REFINE_PGTOL\s*=\s*0,\s*CBO_REFINE_FTOL\s*=\s*1,\s*CBO_REFINE_STEP\s*=\s*2,\s*"
                     r"CBO_REFINE_MAX_ROUNDS\s*=\s*3,\s*CBO_REFINE_NAN_START\s*=\s*4,\s*CBO_REFINE_DECLINED\s*=\s*5\s*\}", text)
    assert enum
    assert (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP, _lib.REFINE_MAX_ROUNDS, _lib.REFINE_NAN_START,
            _lib.REFINE_DECLINED) == (0, 1, 2, 3, 4, 5)
    assert sorted(_lib.REFINE_STATUS_NAME) == [0, 1, 2, 3, 4, 5]
    assert _lib.REFINE_KIND_CODE == {"EI": 0, "LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}


def test_the_library_refuses_bad_scalars_before_it_touches_a_handle():
    lib = _lib.load()
    out = np.zeros(4)
    ints = np.zeros(4, dtype=np.int32)
    call = lambda n_sets=1, kind=0, task=0, param=0.0, max_rounds=10, y=True: lib.cbo_acq_refine_sets(    # noqa: E731
        n_sets, None, None, kind, _lib.dptr(np.array([0.5])) if y else None, task, param, max_rounds, _lib.dptr(out),
        _lib.dptr(out), _lib.dptr(out), ints.ctypes.data_as(_lib.c_int_p), ints.ctypes.data_as(_lib.c_int_p))
    assert call(n_sets=0) == _lib.CBO_ERR_INVALID and b"n_sets" in lib.cbo_last_error()
    assert call() == _lib.CBO_ERR_INVALID and b"NULL" in lib.cbo_last_error()
    assert call(y=False) == _lib.CBO_ERR_INVALID


def test_python_argument_checks_fire_before_a_device_or_a_grid_is_touched(monkeypatch):
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

    assert inspect.signature(find_next_y_points).parameters["refine"].default is False
    obj = Untouchable()
    models = [Model(11), Model(12)]
    boxes = [[(-1.0, 1.0)], [(-2.0, 2.0)]]
    sweep = lambda **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], refine=True, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="spaces"):
        sweep()
    with pytest.raises(ValueError, match="spaces"):
        sweep(spaces=boxes[:1])
    with pytest.raises(ValueError, match="no gradients"):
        sweep(spaces=boxes, acquisition="MES")
    with pytest.raises(ValueError, match="constraints"):
        sweep(spaces=boxes, constraints=[[ProbabilityOfFeasibility(obj)], []])
    with pytest.raises(ValueError, match="hyper_samples"):
        sweep(spaces=boxes, hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
    with pytest.raises(ValueError, match="batch_size"):
        sweep(spaces=boxes, batch_size=2)
    with pytest.raises(ValueError, match="raw"):
        sweep(spaces=boxes, raw=True)
    # the path and the agent
    path = lambda spaces=boxes, **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj],     # noqa: E731
                                                                     [obj, obj], spaces, comm=None, refine=True, **kw)
    with pytest.raises(ValueError, match="spaces"):
        path(spaces=boxes[:1])
    with pytest.raises(ValueError, match="no gradients"):
        path(acquisition="MES")
    col = np.zeros((3, 1))
    with pytest.raises(ValueError, match="constraints"):
        path(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    with pytest.raises(ValueError, match="hyper_samples"):
        path(hyper_samples=4)
    with pytest.raises(ValueError, match="batch_size"):
        path(batch_size=3)
    assert path().refine is True and path(acquisition="LCB", acquisition_param=2.0).refine is True

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes, comm=Two(),
                                          refine=True)
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        assert inspect.signature(cls.__init__).parameters["refine"].default is False
    plain = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], [obj, obj], comm=None)
    assert plain.refine is False
    # refine_sets' own checks
    cost = Cost({"X": functools.partial(__import__("cbo_with_oop_amd").graphs.cost, 1, False)}, ["X"])
    for kw, word in ((dict(kind=("MES", (10, 5))), "acquisition"), (dict(max_rounds=1001), "max_rounds"),
                     (dict(max_rounds=-1), "max_rounds")):
        with pytest.raises(ValueError, match=word):
            refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [cost], **kw)
    with pytest.raises(ValueError, match="task"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "most", [cost])
    with pytest.raises(ValueError, match="starts"):
        refine_sets(models[:1], [np.zeros((65, 1))], boxes[:1], 0.0, "min", [cost])
    with pytest.raises(ValueError, match="finite"):
        refine_sets(models[:1], [np.array([[np.nan]])], boxes[:1], 0.0, "min", [cost])
    with pytest.raises(ValueError, match="bounds"):
        refine_sets(models[:1], [np.zeros((1, 1))], [[(1.0, -1.0)]], 0.0, "min", [cost])
    zero = Cost({"X": functools.partial(__import__("cbo_with_oop_amd").graphs.cost, 0, True)}, ["X"])
    with pytest.raises(ValueError, match="positive cost"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [zero])


def test_the_agent_refuses_refinement_it_cannot_run_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="no gradients"):
        make(refine=True, acquisition="MES")
    with pytest.raises(ValueError, match="batch_size"):
        make(refine=True, batch_size=3)
    with pytest.raises(ValueError, match="hyper_samples"):
        make(refine=True, hyper_samples=5)
    with pytest.raises(ValueError, match="constraints"):
        make(refine=True, constraints={"C": ("<=", 1.0)})
    assert make(refine=True).refine is True and make().refine is False


def test_the_cost_helper_recognises_the_four_cost_types_and_nothing_else():
    from cbo_with_oop_amd import graphs
    for graph in (graphs.ToyGraph, graphs.CompleteGraph, graphs.CoralGraph):
        for type_cost in (1, 2, 3, 4):
            table = graph.get_cost_structure(type_cost)
            for es in graph.get_exploration_set("MIS"):
                got = cost_structure(Cost(table, es))
                assert got is not None, (graph.__name__, type_cost, es)
                fix, variable = got
                assert fix.dtype == np.float64 and variable.dtype == np.int32 and fix.shape == variable.shape == (len(es),)
                assert list(variable) == [1 if type_cost in (3, 4) else 0] * len(es)
                assert list(fix) == [float(table[v].args[0]) for v in es]
    assert cost_structure(Cost({"X": lambda col: 1.0}, ["X"])) is None
    table = graphs.ToyGraph.get_cost_structure(1)
    mixed = dict(table)
    mixed["Z"] = lambda col: 2.0
    assert cost_structure(Cost(mixed, ["X"])) is not None and cost_structure(Cost(mixed, ["X", "Z"])) is None
    assert cost_structure(Cost({"X": functools.partial(graphs.cost, 1)}, ["X"])) is None             # variable not bound
    assert cost_structure(Cost({"X": functools.partial(np.sum)}, ["X"])) is None
    assert cost_structure(object()) is None


def test_the_one_row_cost_is_cost_evaluate_bit_for_bit():
    from cbo_with_oop_amd import graphs
    rng = np.random.default_rng(5)
    for graph in (graphs.CompleteGraph, graphs.CoralGraph):
        for type_cost in (1, 2, 3, 4):
            table = graph.get_cost_structure(type_cost)
            for es in graph.get_exploration_set("MIS"):
                cost = Cost(table, es)
                fix, variable = cost_structure(cost)
                for _ in range(20):
                    x = rng.uniform(-7, 7, (1, len(es))) * rng.choice([1.0, 1e-3, 1e3])
                    want = cost.evaluate(x)
                    got = one_row_cost(fix, variable, x[0])
                    assert float(want) == got and np.float64(want).tobytes() == np.float64(got).tobytes()
