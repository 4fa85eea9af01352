"""The constrained acquisition in log space, what needs no GPU: the two entry points' declarations, exports
and prototypes, the library's refusals, the refusals of the Python layers, the pins that keep holding, the host restatement
against mpmath at 60 digits and the host gradient against central differences of that reference."""
import ctypes
import inspect
import os
import re

import mpmath as mp
import numpy as np
import pytest
import scipy.special

from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import (AcquisitionProduct, ConstrainedLogExpectedImprovement, Cost,
                                              ProbabilityOfFeasibility, find_next_y_point, find_next_y_points)
from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement, LogAcquisitionQuotient
from cbo_with_oop_amd.utils_functions.utils import sets_acquisition, sets_acquisition_or_default

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# §4x's ladder of u, for every constraint term
LADDER = np.concatenate([-np.logspace(0, 7.5, 1500), np.linspace(-40, -1, 2000), np.linspace(-1.5, 40, 800),
                         np.linspace(-1.01, -0.99, 200)])
BOUND = 4e-15            # §4x's host bound: |got - ref| <= BOUND * max(1, |ref|)


# ------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name, sibling, renamed", [
    ("cbo_acq_sweep_constrained_log", "cbo_acq_sweep_constrained", {"ei_out": "logei_out", "pof_out": "logpof_out"}),
    ("cbo_acq_sweep_sets_constrained_log", "cbo_acq_sweep_sets_constrained", {})])
def test_the_entry_points_are_declared_exported_and_prototyped(name, sibling, renamed):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cbo_hip.h")).read(), flags=re.S)

    def arguments(symbol):
        decl = re.search(r"\bint\s+" + symbol + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, f"{symbol} not declared in include/cbo_hip.h"
        return [" ".join(a.split()) for a in decl.group(1).split(",")]
    mine, theirs = arguments(name), arguments(sibling)
    for old, new in renamed.items():
        assert any(a.endswith("*" + old) for a in theirs) and any(a.endswith("*" + new) for a in mine)
        theirs = [a[:-len(old)] + new if a.endswith("*" + old) else a for a in theirs]
    assert mine == theirs
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == _lib.SIGNATURES[sibling][1] and len(argtypes) == len(mine)
    assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"


def test_the_kind_tables_and_the_abi_version_are_what_they_were():
    assert _lib.ACQ_KIND_CODE == {"LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.REFINE_KIND_CODE == {"EI": 0, "LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)


def test_the_library_refuses_null_handles_and_bad_scalars():
    lib = _lib.load()
    out, idx = np.zeros(4), np.zeros(4, dtype=np.int64)
    refused = lambda rc, word: rc == _lib.CBO_ERR_INVALID and word in lib.cbo_last_error()      # noqa: E731
    none = (ctypes.c_void_p * 8)()                                    # NULL handles: what is refused first needs none
    ip = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(_lib.c_int_p)      # noqa: E731

    def single(n_con=1, value=0.0, jitter=0.0, sense=0, cost=1.0, y_best=0.5, ei_jitter=0.0):
        return lib.cbo_acq_sweep_constrained_log(None, None, y_best, 0, ei_jitter, cost, n_con, none, none,
                                                 _lib.dptr(np.full(8, value)), _lib.dptr(np.full(8, jitter)), ip([sense] * 8),
                                                 None, None, None, None, None)

    def sets(n_con=1, value=0.0, jitter=0.0, sense=0, cost=1.0, y_best=0.5, ei_jitter=0.0, task=0, n_sets=1):
        return lib.cbo_acq_sweep_sets_constrained_log(n_sets, none, none, _lib.dptr(np.array([y_best])), task, ei_jitter,
                                                      _lib.dptr(np.array([cost])), ip([n_con]), none, none,
                                                      _lib.dptr(np.full(8, value)), _lib.dptr(np.full(8, jitter)),
                                                      ip([sense] * 8), _lib.dptr(out), idx.ctypes.data_as(_lib.c_int64_p))

    assert refused(single(), b"NULL") and refused(sets(), b"NULL")    # every scalar is good: the NULL handles are met
    for call in (single, sets):
        for n_con in (-1, 9):
            assert refused(call(n_con=n_con), b"0..8"), (call.__name__, n_con)
        for bad in (np.nan, np.inf, -np.inf):
            assert refused(call(value=bad), b"finite") and refused(call(jitter=bad), b"finite"), (call.__name__, bad)
        for sense in (2, -1):
            assert refused(call(sense=sense), b"sense"), (call.__name__, sense)
        for cost in (0.0, -1.0, np.nan):
            assert refused(call(cost=cost), b"cost"), (call.__name__, cost)
    # the log EI's own scalars, as cbo_acq_sweep_sets_logei refuses them
    for bad in (np.nan, np.inf):
        assert refused(sets(ei_jitter=bad), b"jitter") and refused(sets(y_best=bad), b"y_best")
    assert refused(sets(task=2), b"task") and refused(sets(n_sets=0), b"n_sets")
    assert refused(lib.cbo_acq_sweep_constrained_log(None, None, 0.5, 0, 0.0, 1.0, 0, None, None, None, None, None, None,
                                                     None, None, None, None), b"no objective")


# ------------------------------------------------------------------------------------------------------------ the Python layers
def test_the_name_is_accepted_with_its_jitter():
    assert sets_acquisition("LOGCEI") == ("LOGCEI", 0.0) and sets_acquisition_or_default("LOGCEI", 0.25) == ("LOGCEI", 0.25)
    assert sets_acquisition(("LOGCEI", 0.5)) == ("LOGCEI", 0.5)
    for bad in (np.inf, np.nan, "x"):
        with pytest.raises(ValueError, match="jitter"):
            sets_acquisition("LOGCEI", bad)
    assert "LOGCEI" not in _lib.ACQ_KIND_CODE and "LOGCEI" not in _lib.REFINE_KIND_CODE


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


class Handle:
    def __init__(self, handle):
        self._handle = ctypes.c_void_p(handle)
        self.small, self.stale, self.causal, self.input_dim = True, True, False, 1


def test_refused_combinations_raise_before_the_library_is_loaded(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    obj = Untouchable()
    models = [Handle(11), Handle(12)]
    boxes = [[(-1.0, 1.0)], [(-2.0, 2.0)]]
    cons = [[ProbabilityOfFeasibility(obj)], []]
    sweep = lambda **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition="LOGCEI", **kw)  # noqa: E731
    with pytest.raises(ValueError, match="'LOGEI'"):
        sweep()
    with pytest.raises(ValueError, match="hyper_samples"):
        sweep(constraints=cons, hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
    with pytest.raises(ValueError, match="batch_size"):
        sweep(constraints=cons, batch_size=2)
    with pytest.raises(ValueError, match="refine"):
        sweep(constraints=cons, refine=True, spaces=boxes)
    with pytest.raises(ValueError, match="device_prior"):
        sweep(constraints=cons, device_prior=True)
    with pytest.raises(ValueError, match="cost_mode"):
        sweep(constraints=cons, cost_mode="pointwise")
    with pytest.raises(ValueError, match="raw"):
        sweep(constraints=cons, raw=True)
    with pytest.raises(ValueError, match="jitter"):
        sweep(constraints=cons, acquisition_param=np.nan)
    with pytest.raises(ValueError, match="at most 8"):
        sweep(constraints=[[ProbabilityOfFeasibility(obj)] * 9, []])
    # the single-set function
    one = [ProbabilityOfFeasibility(obj)]
    single = lambda **kw: find_next_y_point(obj, obj, 0.0, ["X"], obj, acquisition="LOGCEI", **kw)      # noqa: E731
    with pytest.raises(ValueError, match="'LOGEI'"):
        single()
    with pytest.raises(ValueError, match="hyper_samples"):
        single(constraints=one, hyper_samples=4)
    with pytest.raises(ValueError, match="batch_size"):
        single(constraints=one, batch_size=2)
    with pytest.raises(ValueError, match="cost_mode"):
        single(constraints=one, cost_mode="pointwise")
    with pytest.raises(ValueError, match="anchors"):
        single(constraints=one, anchors="uniform")
    # the path and the agent
    col = np.zeros((3, 1))
    given = dict(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    path = lambda **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes,  # noqa: E731
                                                      comm=None, acquisition="LOGCEI", **kw)
    with pytest.raises(ValueError, match="'LOGEI'"):
        path()
    with pytest.raises(ValueError, match="hyper_samples"):
        path(hyper_samples=4, **given)
    with pytest.raises(ValueError, match="batch_size"):
        path(batch_size=3, **given)
    with pytest.raises(ValueError, match="refine"):
        path(refine=True, **given)
    with pytest.raises(ValueError, match="cost_mode"):
        path(cost_mode="pointwise", **given)
    with pytest.raises(ValueError, match="jitter"):
        path(acquisition_param=np.inf, **given)
    assert path(**given)._kind == ("LOGCEI", 0.0) and path(acquisition_param=0.5, **given)._kind == ("LOGCEI", 0.5)

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes, comm=Two(),
                                          acquisition="LOGCEI", **given)
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = [["B"], ["D"]]
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data,      # noqa: E731
                                       exploration_set=es, acquisition="LOGCEI", **kw)
    bound = {"C": ("<=", 1.0)}
    with pytest.raises(ValueError, match="'LOGEI'"):
        make()
    with pytest.raises(ValueError, match="batch_size"):
        make(constraints=bound, batch_size=3)
    with pytest.raises(ValueError, match="hyper_samples"):
        make(constraints=bound, hyper_samples=5)
    with pytest.raises(ValueError, match="refine"):
        make(constraints=bound, refine=True)
    with pytest.raises(ValueError, match="cost_mode"):
        make(constraints=bound, cost_mode="pointwise")


def test_the_old_refusals_stand(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    obj = Untouchable()
    models = [Handle(11), Handle(12)]
    boxes = [[(-1.0, 1.0)], [(-2.0, 2.0)]]
    cons = [[ProbabilityOfFeasibility(obj)], []]
    col = np.zeros((3, 1))
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = [["B"], ["D"]]
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    for name, message in (("LOGEI", "constraints"), ("LCB", "acquisition must be 'EI'"), ("PI", "acquisition must be 'EI'"),
                          ("MES", "acquisition must be 'EI'")):
        with pytest.raises(ValueError, match=message):
            find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition=name, constraints=cons,
                               spaces=boxes)
        with pytest.raises(ValueError, match=message):
            find_next_y_point(obj, obj, 0.0, ["X"], obj, acquisition=name, constraints=cons[0])
        with pytest.raises(ValueError, match=message):
            cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes, comm=None,
                                          acquisition=name, constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
        with pytest.raises(ValueError, match=message):
            cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data, exploration_set=es,
                           acquisition=name, constraints={"C": ("<=", 1.0)})
    with pytest.raises(ValueError, match="pointwise"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], constraints=cons, cost_mode="pointwise")
    with pytest.raises(ValueError, match="pointwise"):
        find_next_y_point(obj, obj, 0.0, ["X"], obj, constraints=cons[0], cost_mode="pointwise")
    assert list(inspect.signature(find_next_y_point).parameters)[-1] == "constraints"
    log_ei = CausalLogExpectedImprovement(0.0, "min", None)
    with pytest.raises(ValueError, match="CausalExpectedImprovement and ProbabilityOfFeasibility"):
        AcquisitionProduct([log_ei, ProbabilityOfFeasibility(None)])
    for fn in (find_next_y_point, find_next_y_points):
        assert inspect.signature(fn).parameters["acquisition"].default == "EI"


def test_the_class_checks_its_arguments_and_divides_into_a_log_quotient():
    from cbo_with_oop_amd import CausalExpectedImprovement, graphs
    import functools
    log_ei = CausalLogExpectedImprovement(0.0, "min", None)
    pof = ProbabilityOfFeasibility(None, 0.0, 1.0)
    with pytest.raises(ValueError, match="CausalLogExpectedImprovement"):
        ConstrainedLogExpectedImprovement(CausalExpectedImprovement(0.0, "min", None), [pof])
    with pytest.raises(ValueError, match="ProbabilityOfFeasibility"):
        ConstrainedLogExpectedImprovement(log_ei, [log_ei])
    with pytest.raises(ValueError, match="at most 8"):
        ConstrainedLogExpectedImprovement(log_ei, [pof] * 9)
    acq = ConstrainedLogExpectedImprovement(log_ei, [pof] * 8)
    assert acq.objective is log_ei and acq.constraints == [pof] * 8 and acq.factors == [log_ei] + [pof] * 8
    assert isinstance(acq, AcquisitionProduct)                          # (the candidate-grid handling is the product's)
    cost = Cost({"X": functools.partial(graphs.cost, 2, False)}, ["X"])
    quotient = acq / cost
    assert type(quotient) is LogAcquisitionQuotient and quotient.is_log and quotient.numerator is acq


# ------------------------------------------------------------------------------------------------------------ the host restatement
def test_a_constraint_term_against_mpmath_over_the_ladder():
    """sd = 1, max_value = 0, jitter 0: u = -mean exactly, the term is log_ndtr(u) ('<=') and log_ndtr(-u) ('>=')."""
    with mp.workdps(60):
        ref = [mp.log(mp.ncdf(mp.mpf(float(u)))) for u in LADDER]
        for sense, mean in (("<=", -LADDER), (">=", LADDER)):
            got = ConstrainedLogExpectedImprovement.log_feasibility(mean, np.ones_like(LADDER), 0.0, 0.0, sense)
            assert np.all(np.isfinite(got))
            err = np.array([float(abs(mp.mpf(float(g)) - r) / max(mp.mpf(1), abs(r))) for g, r in zip(got, ref)])
            worst = int(np.argmax(err))
            print(f"log_feasibility {sense}: worst scaled error {err[worst]:.3e} at u = {LADDER[worst]!r}")
            assert err[worst] <= BOUND, (err[worst], LADDER[worst])
    # the jitter moves the mean, sd divides: the same u up to one rounding of the shifted mean, |du| <= 2^-53 |u|, which moves
    # log_ndtr by |u| |du| <= 2^-52 |log_ndtr| in the tail
    shifted = ConstrainedLogExpectedImprovement.log_feasibility(-2.0 * LADDER - 0.25, np.full_like(LADDER, 2.0), 0.5, 0.75)
    want = scipy.special.log_ndtr(LADDER)
    assert np.allclose(shifted, want, rtol=0, atol=4e-15 * np.maximum(1.0, np.abs(want)))


def test_the_sum_against_mpmath_over_the_ladder():
    """log EI (CausalLogExpectedImprovement.log_ei) plus two constraint terms, every u of the ladder in every term: the sum's
    error is bounded by the terms' own, BOUND each relative to max(1, |term|), plus one rounding per addition."""
    with mp.workdps(60):
        got = CausalLogExpectedImprovement.log_ei(-LADDER, np.ones_like(LADDER), 0.0, "min", 0.0)
        terms = [got]
        for shift in (700, 1900):                                      # (the constraints walk the ladder out of step)
            u = np.roll(LADDER, shift)
            terms.append(ConstrainedLogExpectedImprovement.log_feasibility(-u, np.ones_like(u), 0.0))
        total = (terms[0] + terms[1]) + terms[2]
        worst = 0.0
        for i in range(len(LADDER)):
            x = mp.mpf(float(LADDER[i]))
            refs = [mp.log(mp.npdf(x) + x * mp.ncdf(x))] + [mp.log(mp.ncdf(mp.mpf(float(np.roll(LADDER, s)[i]))))
                                                           for s in (700, 1900)]
            scale = max(mp.mpf(1), sum(abs(r) for r in refs))
            worst = max(worst, float(abs(mp.mpf(float(total[i])) - sum(refs)) / scale))
        print(f"log EI + 2 log PoF: worst scaled error {worst:.3e}")
        assert worst <= BOUND + 2 * 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------ the gradient
class Analytic:
    """A 'model' whose posterior is a closed form of x (d = 2): mean = a sin(b x0) + c + 0.1 x1, variance = v0 + v1 x0^2 +
    0.01 x1^2 -- with the gradients, and the same in mpmath."""

    def __init__(self, a, b, c, v0, v1):
        self.p = (a, b, c, v0, v1)

    def predict(self, x):
        a, b, c, v0, v1 = self.p
        return (a * np.sin(b * x[:, :1]) + c + 0.1 * x[:, 1:2]), (v0 + v1 * x[:, :1] ** 2 + 0.01 * x[:, 1:2] ** 2)

    def get_prediction_gradients(self, x):
        a, b, c, v0, v1 = self.p
        dmean = np.hstack([a * b * np.cos(b * x[:, :1]), np.full((x.shape[0], 1), 0.1)])
        return dmean, np.hstack([2 * v1 * x[:, :1], 0.02 * x[:, 1:2]])

    def mp_predict(self, x0, x1):
        a, b, c, v0, v1 = (mp.mpf(v) for v in self.p)
        return a * mp.sin(b * x0) + c + mp.mpf("0.1") * x1, v0 + v1 * x0 ** 2 + mp.mpf("0.01") * x1 ** 2


GRAD_STEP = 2.0 ** -16
GRAD_ROUNDING = 1e-10


@pytest.mark.parametrize("task", ["min", "max"])
def test_evaluate_with_gradients_against_central_differences_of_the_reference(task):
    """Three points, the second constraint's u below -30 at the first (sd 0.042 there, the bound 1.5 away on the wrong side).
    The reference is mpmath at 60 digits from the closed-form posterior, so its differences carry no rounding; the step is
    h = 2^-16 in every coordinate.  The bound has two parts, as test_logei_gpu.py's.
    Truncation: D_h - f' = h^2 f3 / 6 + O(h^4) and D_2h - D_h = 3 (h^2 f3 / 6) + O(h^4): |D_2h - D_h| / 3 estimates it from the
    same reference; twice that is allowed, for the O(h^4) terms.
    Rounding, of the host class in double: mean and sd come from numpy to 2 ulps of numbers of order 1, so a = value - mean
    is good to 4 x 1.1e-16 and u = a / sd to 4.4e-16 / sd + 4.4e-16 |u| -- with sd >= 0.04 and |u| <= 40 that is 2.9e-14.  A
    constraint's coefficient is exp(-(u^2 / 2) - log sqrt(2 pi) - log_ndtr(u)); its exponent errs by |u| du (1.2e-12), by
    the roundings of numbers of size u^2 / 2 = 800 (3 x 800 x 1.1e-16 = 2.7e-13) and by log_ndtr's own 4e-15 x 800 =
    3.2e-12: 4.7e-12 in all, which is the coefficient's relative error; du/dx adds a few ulps and the log EI's A and B
    (4e-15, test_logei_host.py) less.  Allowed: GRAD_ROUNDING = 1e-10 relative to the largest of 1 and the gradient
    component's size -- twenty times the 4.7e-12, since the terms of the sum may cancel against each other by that much."""
    objective = Analytic(0.4, 1.1, 0.2, 0.09, 0.02)
    con_a, con_b = Analytic(0.3, 0.7, 0.1, 0.25, 0.05), Analytic(0.1, 0.9, 0.5, 0.0016, 0.6)
    y_best, jitter = (-0.5, 0.0078125) if task == "min" else (1.0, 0.0078125)
    spec = [(con_a, "<=", 0.4, 0.01), (con_b, ">=", 2.0, 0.0)]
    acq = ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(y_best, task, objective, jitter),
                                            [ProbabilityOfFeasibility(m, j, v, sense=s) for m, s, v, j in spec])
    pts = np.array([[0.0, 0.125], [0.75, -1.0], [-1.25, 0.25]])

    def reference(x0, x1):
        mean, var = objective.mp_predict(x0, x1)
        s = mp.sqrt(var)
        u = (mp.mpf(y_best) - (mean + mp.mpf(jitter))) / s if task == "min" else ((mean - mp.mpf(jitter)) - mp.mpf(y_best)) / s
        total, us = mp.log(mp.npdf(u) + u * mp.ncdf(u)) + mp.log(s), []
        for m, sense, value, jit in spec:
            mean, var = m.mp_predict(x0, x1)
            uc = (mp.mpf(value) - (mean + mp.mpf(jit))) / mp.sqrt(var)
            uc = uc if sense == "<=" else -uc
            us.append(uc)
            total += mp.log(mp.ncdf(uc))
        return total, us

    f, df = acq.evaluate_with_gradients(pts)
    assert f.shape == (3, 1) and df.shape == (3, 2) and np.all(np.isfinite(f)) and np.all(np.isfinite(df))
    with mp.workdps(60):
        h = mp.mpf(GRAD_STEP)
        below = []
        for i, (x0, x1) in enumerate(pts):
            x0, x1 = mp.mpf(float(x0)), mp.mpf(float(x1))
            ref, us = reference(x0, x1)
            below.append(float(us[1]))
            assert abs(mp.mpf(float(f[i, 0])) - ref) <= 3 * BOUND * max(1, abs(ref)), (i, f[i, 0], ref)
            for j, (e0, e1) in enumerate(((1, 0), (0, 1))):
                d_h = (reference(x0 + h * e0, x1 + h * e1)[0] - reference(x0 - h * e0, x1 - h * e1)[0]) / (2 * h)
                d_2h = (reference(x0 + 2 * h * e0, x1 + 2 * h * e1)[0] - reference(x0 - 2 * h * e0, x1 - 2 * h * e1)[0]) / (4 * h)
                bound = 2 * abs(d_2h - d_h) / 3 + GRAD_ROUNDING * max(1, abs(d_h))
                err = abs(mp.mpf(float(df[i, j])) - d_h)
                print(f"{task} point {i} coordinate {j}: gradient {df[i, j]!r}, |grad - D_h| {float(err):.3e}, bound "
                      f"{float(bound):.3e}, u of the constraints {[float(u) for u in us]}")
                assert err <= bound, (i, j, float(err), float(bound))
        assert below[0] < -30.0 and min(below[1:]) > -30.0               # the precondition: one point in the far range
    # under a cost: the value less log cost, the gradient as it is
    import functools
    from cbo_with_oop_amd import graphs
    cost = Cost({"X": functools.partial(graphs.cost, 2, False), "Z": functools.partial(graphs.cost, 3, False)}, ["X", "Z"])
    fq, dfq = (acq / cost).evaluate_with_gradients(pts[:1])
    assert fq[0, 0] == f[0, 0] - np.log(5.0) and np.array_equal(dfq, df[:1])
