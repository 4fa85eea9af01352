"""Gradient refinement under constraints, what needs no GPU: the entry point's declaration, export and
prototype, the library's argument checks, the refusals of the Python layers before the library is loaded, the defaults and
parameter positions, the host route's acquisitions, and the hazard ratio's host restatement against mpmath at 60 digits."""
import ctypes
import functools
import inspect
import os
import re

import mpmath as mp
import numpy as np
import pytest

from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib, graphs
from cbo_with_oop_amd.utils_functions import Cost, ProbabilityOfFeasibility, find_next_y_point, find_next_y_points
from cbo_with_oop_amd.utils_functions import causal_optimizer
from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
from cbo_with_oop_amd.utils_functions.constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cbo_acq_refine_sets_constrained"

# §4x's ladder of the standardised argument: both ends, the ranges and the split at -1
LADDER = np.concatenate([-np.logspace(0, 7.5, 1500), np.linspace(-40, -1, 2000), np.linspace(-1.5, 40, 800),
                         np.linspace(-1.01, -0.99, 200)])
BOUND = 4e-15            # |got - ref| <= BOUND * max(1, |ref|): §4x's host bound


def test_the_entry_point_is_declared_exported_and_prototyped():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cbo_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, f"{NAME} not declared in include/cbo_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert [re.sub(r".*[\s\*]", "", p) for p in params] == [
        "n_sets", "gps", "sets", "log_form", "y_best", "task", "ei_jitter", "n_con", "con_gps", "con_value", "con_jitter",
        "con_sense", "max_rounds", "x_out", "val_out", "grad_out", "rounds_out", "status_out"]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 18
    _, sibling = _lib.SIGNATURES["cbo_acq_refine_sets_pointcost"]
    # the sibling's list with the five constraint arguments between the jitter and max_rounds
    assert argtypes == sibling[:7] + [_lib.c_int_p, _lib.c_void_pp, _lib.c_double_p, _lib.c_double_p, _lib.c_int_p] + sibling[7:]
    assert hasattr(_lib.load(), NAME), f"{NAME} not exported by libcbo_hip.so"
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_abi_version_and_the_kind_tables_are_what_they_were():
    assert _lib.ACQ_KIND_CODE == {"LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.REFINE_KIND_CODE == {"EI": 0, "LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_the_library_refuses_null_and_bad_scalars_before_any_launch():
    lib = _lib.load()
    out, ints = np.zeros(4), np.zeros(4, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)      # noqa: E731
    gps = (ctypes.c_void_p * 1)(None)
    sets = (_lib.CboRefineSet * 1)()

    def call(n_sets=1, log_form=0, y_best=0.5, task=0, jitter=0.0, n_con=0, max_rounds=10, y=True, counts=True, handles=True,
             values=None, jitters=None, senses=None, con_gps=None):
        return lib.cbo_acq_refine_sets_constrained(
            n_sets, gps if handles else None, sets, log_form, _lib.dptr(np.array([y_best])) if y else None, task, jitter,
            ip(np.array([n_con], dtype=np.int32)) if counts else None, con_gps,
            None if values is None else _lib.dptr(np.asarray(values, dtype=np.float64)),
            None if jitters is None else _lib.dptr(np.asarray(jitters, dtype=np.float64)),
            None if senses is None else ip(np.asarray(senses, dtype=np.int32)), max_rounds, _lib.dptr(out), _lib.dptr(out),
            _lib.dptr(out), ip(ints), ip(ints))

    refused = lambda rc, word: rc == _lib.CBO_ERR_INVALID and word in lib.cbo_last_error()      # noqa: E731
    assert refused(call(n_sets=0), b"n_sets")
    assert refused(call(log_form=2), b"log_form") and refused(call(log_form=-1), b"log_form")
    assert refused(call(handles=False), b"NULL") and refused(call(y=False), b"NULL") and refused(call(counts=False), b"NULL")
    assert refused(call(max_rounds=-1), b"max_rounds") and refused(call(max_rounds=10 ** 6), b"max_rounds")
    assert refused(call(task=2), b"task") and refused(call(task=-1), b"task")
    assert refused(call(jitter=np.inf), b"jitter") and refused(call(jitter=np.nan), b"jitter")
    assert refused(call(y_best=np.nan), b"y_best") and refused(call(y_best=np.inf), b"y_best")
    assert refused(call(n_con=-1), b"n_con") and refused(call(n_con=9), b"n_con")
    one = (ctypes.c_void_p * 1)(None)
    full = dict(con_gps=one, values=[0.0], jitters=[0.0], senses=[0])
    for missing, word in (("con_gps", b"con_gps"), ("values", b"con_value"), ("jitters", b"con_jitter"), ("senses", b"con_sense")):
        assert refused(call(n_con=1, **{k: v for k, v in full.items() if k != missing}), word), missing
    assert refused(call(n_con=1, **dict(full, values=[np.nan])), b"con_value")
    assert refused(call(n_con=1, **dict(full, jitters=[np.inf])), b"con_jitter")
    assert refused(call(n_con=1, **dict(full, senses=[2])), b"con_sense")
    # the scalars pass: the first handle is looked at (cbo_acq_refine_sets' checks), then the constraint's
    assert refused(call(n_con=1, **full), b"NULL gp")
    assert refused(call(), b"NULL gp")


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


class Model:
    def __init__(self, handle, dim=1):
        self._handle = ctypes.c_void_p(handle)
        self.small, self.stale, self.causal, self.input_dim = True, True, False, dim


def no_device(*a, **k):
    raise AssertionError("the device library was reached")


def test_refused_combinations_raise_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(_lib, "load", no_device)
    obj = Untouchable()
    models = [Model(11), Model(12)]
    boxes = [[(-1.0, 1.0)], [(-2.0, 2.0)]]
    cons = [[ProbabilityOfFeasibility(obj)], []]

    def sweep(acquisition="EI", **kw):
        kw.setdefault("constraints", cons)
        kw.setdefault("spaces", boxes)
        return find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition=acquisition,
                                  refine_constrained=True, **kw)
    for name in ("LOGEI", "LCB", "PI", "MPEI", "VAR"):
        with pytest.raises(ValueError, match="refine_constrained"):
            sweep(name)
    for empty in (None, [[], []]):
        with pytest.raises(ValueError, match="constraints"):
            sweep(constraints=empty)
        with pytest.raises(ValueError, match="constraints"):
            sweep("LOGCEI", constraints=empty)
    for name in ("EI", "LOGCEI"):
        with pytest.raises(ValueError, match="spaces"):
            sweep(name, spaces=None)
        with pytest.raises(ValueError, match="spaces"):
            sweep(name, spaces=boxes[:1])
        with pytest.raises(ValueError, match="raw"):
            sweep(name, raw=True)
        with pytest.raises(ValueError, match="hyper"):
            sweep(name, hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
        with pytest.raises(ValueError, match="batch"):
            sweep(name, batch_size=2)
        with pytest.raises(ValueError, match="device_prior"):
            sweep(name, device_prior=True)
        with pytest.raises(ValueError, match="cost_mode"):
            sweep(name, cost_mode="pointwise")
    # the pinned refusals: refine=True with constraints, everywhere
    with pytest.raises(ValueError, match="constraints"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], refine=True, spaces=boxes, constraints=cons)
    with pytest.raises(ValueError, match="refine"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition="LOGCEI", refine=True,
                           spaces=boxes, constraints=cons)
    col = np.zeros((3, 1))
    path = lambda **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes,  # noqa: E731
                                                      comm=None, **kw)
    con_kw = dict(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    with pytest.raises(ValueError, match="constraints"):
        path(refine=True, **con_kw)
    with pytest.raises(ValueError, match="refine"):
        path(acquisition="LOGCEI", refine=True, **con_kw)
    with pytest.raises(ValueError, match="constraints"):
        path(refine_constrained=True)
    with pytest.raises(ValueError, match="refine_constrained"):
        path(acquisition="LOGEI", refine_constrained=True)
    with pytest.raises(ValueError, match="cost_mode"):
        path(refine_constrained=True, cost_mode="pointwise", **con_kw)
    for name in ("EI", "LOGCEI"):
        built = path(acquisition=name, refine_constrained=True, **con_kw)
        assert built.refine_constrained is True and built.refine is False
    assert path(**con_kw).refine_constrained is False

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes, comm=Two(),
                                          refine_constrained=True, **con_kw)
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="constraints"):
        make(refine=True, constraints={"C": ("<=", 1.0)})
    with pytest.raises(ValueError, match="constraints"):
        make(refine_constrained=True)
    with pytest.raises(ValueError, match="acquisition"):
        make(refine_constrained=True, acquisition="PI", constraints={"C": ("<=", 1.0)})
    with pytest.raises(ValueError, match="batch"):
        make(refine_constrained=True, batch_size=2, constraints={"C": ("<=", 1.0)})
    # refine_sets
    cost = Cost({"X": functools.partial(graphs.cost, 1, False)}, ["X"])
    one = dict(models=models[:1], starts=[np.zeros((1, 1))], bounds=boxes[:1], current_global_best=0.0, task="min", costs=[cost])
    pof = ProbabilityOfFeasibility(obj)
    for kind in (("LOGEI", 0.0), ("LCB", 1.0), ("PI", 0.0), ("MPEI", 0.0), ("VAR", 0.0)):
        with pytest.raises(ValueError, match="constraints"):
            refine_sets(**one, kind=kind, constraints=[[pof]])
    with pytest.raises(ValueError, match="constraints"):
        refine_sets(**one, kind=("LOGCEI", 0.0))
    with pytest.raises(ValueError, match="device_prior"):
        refine_sets(**one, constraints=[[pof]], device_prior=True)
    with pytest.raises(ValueError, match="cost_mode"):
        refine_sets(**one, constraints=[[pof]], cost_mode="pointwise")
    with pytest.raises(ValueError, match="one list per exploration set"):
        refine_sets(**one, constraints=[[pof], [pof]])
    with pytest.raises(ValueError, match="at most 8"):
        refine_sets(**one, constraints=[[pof] * 9])
    with pytest.raises(ValueError, match="ProbabilityOfFeasibility"):
        refine_sets(**one, constraints=[[object()]])
    with pytest.raises(ValueError, match="jitter"):
        refine_sets(**one, kind=("LOGCEI", np.nan), constraints=[[pof]])


def test_defaults_and_parameter_positions():
    for fn in (find_next_y_point, find_next_y_points):
        assert list(inspect.signature(fn).parameters)[-1] == "constraints"
    params = list(inspect.signature(find_next_y_points).parameters)
    assert params[-2] == "refine_constrained"
    assert inspect.signature(find_next_y_points).parameters["refine_constrained"].default is False
    assert "refine_constrained" not in inspect.signature(find_next_y_point).parameters
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["refine_constrained"].default is False and sig["refine"].default is False
    sig = inspect.signature(refine_sets).parameters
    assert list(sig)[-1] == "constraints" and sig["constraints"].default is None
    assert list(sig)[:11] == ["models", "starts", "bounds", "current_global_best", "task", "costs", "kind", "max_rounds",
                              "host_fallback", "device_prior", "cost_mode"]


def test_the_fallback_route_climbs_the_host_classes(monkeypatch):
    """A set the launch cannot take (a causal objective; a large constraint model) goes through ``refine_batched`` with
    ``AcquisitionProduct([...]) / cost`` or ``ConstrainedLogExpectedImprovement(...) / cost``: a stub optimiser records the
    acquisition it is handed and whose ``evaluate_with_gradients`` it would call."""
    monkeypatch.setattr(_lib, "load", no_device)
    seen = []

    class Stub:
        def __init__(self, space):
            self.space = space

        def refine_batched(self, acquisition, x0, max_rounds=200, history=8):
            seen.append((acquisition, max_rounds))
            return np.asarray(x0) + 0.25, np.full(len(x0), 3.5)
    monkeypatch.setattr(causal_optimizer, "CausalGradientAcquisitionOptimizer", Stub)
    causal, large_con = Model(1), Model(2)
    causal.causal = True
    big = Model(3)
    big.small = False
    cost = Cost({"X": functools.partial(graphs.cost, 1, True)}, ["X"])
    cons = [[ProbabilityOfFeasibility(Model(4), max_value=0.5)], [ProbabilityOfFeasibility(big, sense=">=")]]
    starts = [np.zeros((2, 1)), np.ones((1, 1))]
    for kind, cls in ((("EI", None), AcquisitionProduct), (("LOGCEI", 0.25), ConstrainedLogExpectedImprovement)):
        del seen[:]
        out = refine_sets([causal, large_con], starts, [[(-1.0, 1.0)]] * 2, 0.5, "min", [cost, cost], kind=kind, max_rounds=7,
                          constraints=cons)
        assert len(seen) == 2 and all(r == 7 for _, r in seen)
        for (acq, _), con, start, (x, f, status) in zip(seen, cons, starts, out):
            num = acq.numerator
            assert type(num) is cls and acq.denominator is cost and num.constraints == con
            assert type(num).evaluate_with_gradients is cls.evaluate_with_gradients
            assert bool(getattr(acq, "is_log", False)) == (cls is ConstrainedLogExpectedImprovement)
            assert num.objective.jitter == (0.25 if kind[0] == "LOGCEI" else 0.0)
            assert np.array_equal(x, start + 0.25) and np.all(f == 3.5) and np.all(status == _lib.REFINE_DECLINED)
    # host_fallback=False behaves as today: the starts, NaN, DECLINED
    del seen[:]
    (x, f, status), = refine_sets([causal], starts[:1], [[(-1.0, 1.0)]], 0.5, "min", [cost], constraints=cons[:1],
                                  host_fallback=False)
    assert not seen and np.array_equal(x, starts[0]) and np.all(np.isnan(f)) and np.all(status == _lib.REFINE_DECLINED)


def test_optimize_recognises_the_constrained_numerators(monkeypatch):
    """``_device_refinable`` names the form by the numerator's class and refuses what the launch cannot take."""
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement
    from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement
    monkeypatch.setattr(_lib, "load", no_device)
    cost = Cost({"X": functools.partial(graphs.cost, 1, True)}, ["X"])
    model, con = Model(1), Model(2)
    pof = ProbabilityOfFeasibility(con, max_value=0.5)
    product = AcquisitionProduct([CausalExpectedImprovement(0.5, "min", model), pof]) / cost
    assert causal_optimizer._device_refinable(product) == (("EI", None), model, 0.5, "min", cost)
    assert causal_optimizer._product_constraints(product.numerator) == [pof]
    log = ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(0.5, "max", model, 0.125), [pof]) / cost
    assert causal_optimizer._device_refinable(log) == (("LOGCEI", 0.125), model, 0.5, "max", cost)
    assert causal_optimizer._product_constraints(CausalExpectedImprovement(0.5, "min", model)) is None
    assert causal_optimizer._product_constraints(AcquisitionProduct([pof])) is None
    con.small = False
    with pytest.raises(ValueError, match="constraint model"):
        causal_optimizer._device_refinable(product)
    con.small, con.input_dim = True, 2
    with pytest.raises(ValueError, match="dimension"):
        causal_optimizer._device_refinable(log)
    con.input_dim = 1
    with pytest.raises(ValueError, match="device_prior"):
        causal_optimizer._device_refinable(product, True)


@pytest.fixture(scope="module")
def reference():
    """pdf(u) / cdf(u) of every u of the ladder with mpmath at 60 digits."""
    with mp.workdps(60):
        return [mp.npdf(mp.mpf(float(u))) / mp.ncdf(mp.mpf(float(u))) for u in LADDER]


def test_the_hazard_ratio_against_mpmath_over_the_ladder(reference):
    got = ConstrainedLogExpectedImprovement.hazard_ratio(LADDER)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    with mp.workdps(60):
        err = np.array([float(abs(mp.mpf(float(g)) - r) / max(mp.mpf(1), abs(r))) for g, r in zip(got, reference)])
    worst = int(np.argmax(err))
    print(f"hazard ratio: worst scaled error {err[worst]:.3e} at u = {LADDER[worst]!r}")
    assert err[worst] <= BOUND, (err[worst], LADDER[worst])
    # what the plain ratio of an underflowed density over an underflowed distribution gives where this does not
    assert np.isfinite(ConstrainedLogExpectedImprovement.hazard_ratio(np.array([-1e300])))[0]
    assert np.isnan(ConstrainedLogExpectedImprovement.hazard_ratio(np.array([np.nan])))[0]
    # the host class's own ratio (two logarithms) agrees where it is well conditioned
    import scipy.special
    u = np.linspace(-30, 5, 300)
    host = np.exp((-(u * u) / 2.0 - 0.918938533204672741780) - scipy.special.log_ndtr(u))
    assert np.allclose(ConstrainedLogExpectedImprovement.hazard_ratio(u), host, rtol=1e-12, atol=0.0)
