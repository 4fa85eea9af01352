"""log Expected Improvement, what needs no GPU: the host restatement of the device formula against mpmath at
60 digits, the quotient with a cost, the argument checks of the Python layers and of the library, and the pins of the ABI."""
import ctypes
import functools
import inspect
import os
import re

import mpmath as mp
import numpy as np
import pytest

from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import Cost, ProbabilityOfFeasibility, find_next_y_point, find_next_y_points
from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement, LogAcquisitionQuotient
from cbo_with_oop_amd.utils_functions.utils import sets_acquisition, sets_acquisition_or_default

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the ladder of the standardised improvement: both ends, the three ranges and the split at -1
LADDER = np.concatenate([np.linspace(-1.5, 40, 800), -np.logspace(0, 7.5, 1500), np.linspace(-40, -1, 2000),
                         np.linspace(-1.01, -0.99, 200)])
BOUND = 4e-15            # |got - ref| <= BOUND * max(1, |ref|)


@pytest.fixture(scope="module")
def reference():
    """(log h, A, B) of every u of the ladder with mpmath at 60 digits: log(npdf(u) + u ncdf(u)), ncdf / h, npdf / h."""
    with mp.workdps(60):
        out = []
        for u in LADDER:
            x = mp.mpf(float(u))
            pdf, cdf = mp.npdf(x), mp.ncdf(x)
            h = pdf + x * cdf
            out.append((mp.log(h), cdf / h, pdf / h))
    return out


def scaled_errors(got, ref):
    with mp.workdps(60):
        return np.array([float(abs(mp.mpf(float(g)) - r) / max(mp.mpf(1), abs(r))) for g, r in zip(got, ref)])


def test_log_ei_against_mpmath_over_the_ladder(reference):
    # sd = 1, y_best = 0, task 'min': u = -mean exactly, log sd = 0 -- the value is log h(u)
    got = CausalLogExpectedImprovement.log_ei(-LADDER, np.ones_like(LADDER), 0.0, "min", 0.0)
    assert np.all(np.isfinite(got))
    err = scaled_errors(got, [r[0] for r in reference])
    worst = int(np.argmax(err))
    print(f"log_ei: worst scaled error {err[worst]:.3e} at u = {LADDER[worst]!r}")
    assert err[worst] <= BOUND, (err[worst], LADDER[worst])
    # the mirror: task 'max' with the mean mirrored about the incumbent gives the same u, hence the same bits
    mirrored = CausalLogExpectedImprovement.log_ei(LADDER, np.ones_like(LADDER), 0.0, "max", 0.0)
    assert mirrored.tobytes() == got.tobytes()
    # log sd is added, the jitter moves the mean (dyadic numbers: every step exact)
    shifted = CausalLogExpectedImprovement.log_ei(-2.0 * LADDER - 0.25, np.full_like(LADDER, 2.0), 0.0, "min", 0.25)
    assert np.allclose(shifted, got + np.log(2.0), rtol=0, atol=4e-15 * np.maximum(1.0, np.abs(got)))


def test_gradient_coefficients_against_mpmath_over_the_ladder(reference):
    a, b = CausalLogExpectedImprovement.gradient_coefficients(LADDER)
    for name, got, k in (("A", a, 1), ("B", b, 2)):
        assert np.all(np.isfinite(got)), name
        err = scaled_errors(got, [r[k] for r in reference])
        worst = int(np.argmax(err))
        print(f"{name}: worst scaled error {err[worst]:.3e} at u = {LADDER[worst]!r}")
        assert err[worst] <= BOUND, (name, err[worst], LADDER[worst])


def test_nan_in_nan_out_and_the_far_end():
    f = CausalLogExpectedImprovement.log_ei
    assert np.isnan(f(np.array([np.nan]), np.array([1.0]), 0.0))[0] and np.isnan(f(np.array([0.0]), np.array([np.nan]), 0.0))[0]
    far = f(np.array([3e7]), np.array([1.0]), 0.0)[0]               # u = -3e7
    with mp.workdps(60):
        u = mp.mpf(-3e7)
        ref = mp.log(mp.npdf(u) + u * mp.ncdf(u))
        assert np.isfinite(far) and abs(mp.mpf(float(far)) - ref) <= BOUND * abs(ref)


class _Numerator:
    """An acquisition whose value and gradient are known: what the quotient must leave alone."""
    model = None

    def evaluate_with_gradients(self, x):
        return np.full((x.shape[0], 1), -1234.5), np.tile(np.array([[3.0, -7.0]]), (x.shape[0], 1))


def test_the_quotient_subtracts_log_cost_and_leaves_the_gradient_alone():
    graphs = __import__("cbo_with_oop_amd").graphs
    cost = Cost({"X": functools.partial(graphs.cost, 2, True), "Z": functools.partial(graphs.cost, 3, False)}, ["X", "Z"])
    x = np.array([[1.5, -4.0]])
    c = float(cost.evaluate(x))
    assert c == 2 + 1.5 + 3
    q = LogAcquisitionQuotient(_Numerator(), cost)
    f, df = q.evaluate_with_gradients(x)
    assert f.shape == (1, 1) and f[0, 0] == -1234.5 - np.log(c)
    assert df.tolist() == [[3.0, -7.0]]
    # ... and `/` on the class builds it, not AcquisitionQuotient's f / c
    built = CausalLogExpectedImprovement(0.0, "min", None) / cost
    assert type(built) is LogAcquisitionQuotient and built.has_gradients
    # the lockstep searches price a row at its own cost the same way
    from cbo_with_oop_amd.utils_functions.causal_optimizer import _values_and_gradients
    X = np.array([[1.5, -4.0], [0.5, 2.0]])
    vals, grads = _values_and_gradients(q, X)
    assert vals.tolist() == [-1234.5 - np.log(6.5), -1234.5 - np.log(5.5)] and grads.tolist() == [[3.0, -7.0]] * 2


def test_the_name_is_accepted_with_its_jitter_and_the_old_messages_stand():
    assert sets_acquisition("LOGEI") == ("LOGEI", 0.0) and sets_acquisition_or_default("LOGEI", 0.25) == ("LOGEI", 0.25)
    assert sets_acquisition(("LOGEI", 0.5)) == ("LOGEI", 0.5)
    for bad in (np.inf, np.nan, "x", None.__class__):
        with pytest.raises(ValueError, match="jitter"):
            sets_acquisition("LOGEI", bad)
    with pytest.raises(ValueError, match="'EI', 'MES', 'LCB', 'PI', 'MPEI' or 'VAR' in a multi-set sweep"):
        sets_acquisition("LOG_EI")
    with pytest.raises(ValueError, match="'EI', 'LCB', 'PI', 'MPEI' or 'VAR' -- or 'MES' with acquisition_param"):
        sets_acquisition("MES")
    with pytest.raises(ValueError, match="jitter"):
        CausalLogExpectedImprovement(0.0, "min", None, jitter=np.inf)
    with pytest.raises(ValueError, match="task"):
        CausalLogExpectedImprovement(0.0, "most", None)
    assert CausalLogExpectedImprovement.kind == "LOGEI"


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
    sweep = lambda **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition="LOGEI", **kw)  # noqa: E731
    with pytest.raises(ValueError, match="constraints"):
        sweep(constraints=[[ProbabilityOfFeasibility(obj)], []])
    with pytest.raises(ValueError, match="hyper"):
        sweep(hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
    with pytest.raises(ValueError, match="batch"):
        sweep(batch_size=2)
    with pytest.raises(ValueError, match="device_prior"):
        sweep(refine=True, spaces=boxes, device_prior=True)
    with pytest.raises(ValueError, match="raw"):
        sweep(raw=True)
    with pytest.raises(ValueError, match="jitter"):
        sweep(acquisition_param=np.nan)
    with pytest.raises(ValueError, match="task"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "most", [obj, obj], acquisition="LOGEI")
    # max-value entropy search is a name of its own with a parameter of its own: the log EI's jitter is not one
    with pytest.raises(ValueError, match="acquisition_param"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition="MES", acquisition_param=0.25)
    # the single-set function
    single = lambda **kw: find_next_y_point(obj, obj, 0.0, ["X"], obj, acquisition="LOGEI", **kw)      # noqa: E731
    with pytest.raises(ValueError, match="constraints"):
        single(constraints=[ProbabilityOfFeasibility(obj)])
    with pytest.raises(ValueError, match="hyper"):
        single(hyper_samples=4)
    with pytest.raises(ValueError, match="batch"):
        single(batch_size=2)
    # the path and the agent
    path = lambda **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes,  # noqa: E731
                                                      comm=None, acquisition="LOGEI", **kw)
    col = np.zeros((3, 1))
    with pytest.raises(ValueError, match="constraints"):
        path(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    with pytest.raises(ValueError, match="hyper"):
        path(hyper_samples=4)
    with pytest.raises(ValueError, match="batch"):
        path(batch_size=3)
    with pytest.raises(ValueError, match="device_prior"):
        path(refine=True, device_prior=True)
    with pytest.raises(ValueError, match="jitter"):
        path(acquisition_param=np.inf)
    assert path()._kind == ("LOGEI", 0.0) and path(acquisition_param=0.5, refine=True)._kind == ("LOGEI", 0.5)

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes, comm=Two(),
                                          acquisition="LOGEI")
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data,      # noqa: E731
                                       acquisition="LOGEI", **kw)
    with pytest.raises(ValueError, match="batch"):
        make(batch_size=3)
    with pytest.raises(ValueError, match="hyper"):
        make(hyper_samples=5)
    with pytest.raises(ValueError, match="constraints"):
        make(constraints={"C": ("<=", 1.0)})
    with pytest.raises(ValueError, match="device_prior"):
        make(refine=True, device_prior=True)
    # refine_sets
    cost = Cost({"X": functools.partial(__import__("cbo_with_oop_amd").graphs.cost, 1, False)}, ["X"])
    with pytest.raises(ValueError, match="device_prior"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [cost], kind=("LOGEI", 0.0), device_prior=True)
    with pytest.raises(ValueError, match="jitter"):
        refine_sets(models[:1], [np.zeros((1, 1))], boxes[:1], 0.0, "min", [cost], kind=("LOGEI", np.nan))
    # every default is today's
    for fn in (find_next_y_point, find_next_y_points):
        assert inspect.signature(fn).parameters["acquisition"].default == "EI"
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        assert inspect.signature(cls.__init__).parameters["acquisition"].default == "EI"


def test_the_kind_tables_and_the_abi_version_are_what_they_were():
    assert _lib.ACQ_KIND_CODE == {"LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.REFINE_KIND_CODE == {"EI": 0, "LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.LOGEI == "LOGEI" and _lib.LOGEI not in _lib.ACQ_KIND_CODE and _lib.LOGEI not in _lib.REFINE_KIND_CODE
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)


@pytest.mark.parametrize("name, sibling, dropped", [("cbo_acq_sweep_logei", "cbo_acq_sweep_kind", 1),
                                                     ("cbo_acq_sweep_sets_logei", "cbo_acq_sweep_sets_kind", 1),
                                                     ("cbo_acq_refine_sets_logei", "cbo_acq_refine_sets", 1)])
def test_the_entry_points_are_declared_exported_and_prototyped(name, sibling, dropped):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cbo_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, f"{name} not declared in include/cbo_hip.h"
    assert not re.search(r"\bint\s+kind\b", decl.group(1))
    restype, argtypes = _lib.SIGNATURES[name]
    _, sibling_types = _lib.SIGNATURES[sibling]
    assert restype is ctypes.c_int and len(argtypes) == len(decl.group(1).split(",")) == len(sibling_types) - dropped
    # the sibling's argument list without `kind` (its one plain int in front of y_best)
    without_kind = list(sibling_types)
    without_kind.pop(2 if sibling == "cbo_acq_sweep_kind" else 3)
    assert argtypes == without_kind
    assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"


def test_the_library_refuses_null_handles_and_bad_scalars():
    lib = _lib.load()
    out, ints = np.zeros(4), np.zeros(4, dtype=np.int32)
    idx = np.zeros(4, dtype=np.int64)
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)      # noqa: E731
    refused = lambda rc, word: rc == _lib.CBO_ERR_INVALID and word in lib.cbo_last_error()      # noqa: E731

    def single(y_best=0.5, task=0, jitter=0.0, cost=1.0):
        return lib.cbo_acq_sweep_logei(None, None, y_best, task, jitter, cost, None, None, None, None, None)

    def sets(n_sets=1, y_best=0.5, task=0, jitter=0.0, cost=1.0, y=True, costs=True):
        return lib.cbo_acq_sweep_sets_logei(n_sets, None, None, _lib.dptr(np.array([y_best])) if y else None, task, jitter,
                                            _lib.dptr(np.array([cost])) if costs else None, _lib.dptr(out),
                                            idx.ctypes.data_as(_lib.c_int64_p))

    def refine(n_sets=1, y_best=0.5, task=0, jitter=0.0, y=True):
        return lib.cbo_acq_refine_sets_logei(n_sets, None, None, _lib.dptr(np.array([y_best])) if y else None, task, jitter,
                                             10, _lib.dptr(out), _lib.dptr(out), _lib.dptr(out), ip(ints), ip(ints))

    assert refused(single(), b"NULL")
    assert refused(sets(), b"argument") and refused(refine(), b"NULL")
    for call in (single, sets, refine):
        assert refused(call(y_best=np.nan), b"y_best") and refused(call(y_best=np.inf), b"y_best"), call.__name__
        assert refused(call(jitter=np.inf), b"jitter") and refused(call(jitter=np.nan), b"jitter"), call.__name__
        assert refused(call(task=2), b"task") and refused(call(task=-1), b"task"), call.__name__
    for call in (single, sets):
        for cost in (0.0, -1.0, np.nan):
            assert refused(call(cost=cost), b"cost"), (call.__name__, cost)
    assert refused(sets(n_sets=0), b"argument") and refused(sets(y=False), b"argument") and refused(sets(costs=False), b"argument")
    assert refused(refine(n_sets=0), b"n_sets") and refused(refine(y=False), b"NULL")
    # the siblings keep refusing the internal kind code
    assert lib.cbo_acq_sweep_kind(None, None, 7, 0.5, 0, 0.0, 1.0, None, None, None, None, None) == _lib.CBO_ERR_INVALID
    assert b"kind" in lib.cbo_last_error()
    one = _lib.dptr(np.array([0.5]))
    assert lib.cbo_acq_sweep_sets_kind(1, None, None, 7, one, 0, 0.0, one, _lib.dptr(out),
                                       idx.ctypes.data_as(_lib.c_int64_p)) == _lib.CBO_ERR_INVALID
    assert b"kind" in lib.cbo_last_error()
    gps = (ctypes.c_void_p * 1)(None)
    sets_arr = (_lib.CboRefineSet * 1)()
    assert lib.cbo_acq_refine_sets(1, gps, sets_arr, 7, one, 0, 0.0, 10, _lib.dptr(out), _lib.dptr(out), _lib.dptr(out),
                                   ip(ints), ip(ints)) == _lib.CBO_ERR_INVALID
    assert b"kind" in lib.cbo_last_error()
