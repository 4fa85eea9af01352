"""CPU tests of the hyper-marginalised EI in log space: cbo_acq_sweep_hyper_log, cbo_acq_sweep_sets_hyper_log
and cbo_lse_rows are declared, exported and prototyped and refuse bad scalars without a device; acquisition="LOGMEI" needs
hyper_samples and refuses what it does not combine with before a device is touched, at every level; rows take the log entry
point with the rows and the jitter they were given; the class accepts the log generator and refuses the others; and the
streaming log-sum-exp of csrc/lse_stream.h, restated in numpy, meets its error bound against mpmath.  The values are checked
on the GPU (tests/test_hyper_log_gpu.py)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility, find_next_y_point, find_next_y_points
from cbo_with_oop_amd.utils_functions.causal_acquisition_functions import CandidateGrid, CausalExpectedImprovement
from cbo_with_oop_amd.utils_functions.cost_functions import Cost
from cbo_with_oop_amd.utils_functions.integrated_hyper import IntegratedHyperParameterAcquisition
from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import (CausalLogExpectedImprovement,
                                                                     CausalProbabilityOfImprovement)


class Untouchable:
    """Argument checks must not touch grids or cost tables."""

    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


class _Model:
    """What the row check reads of a model: its lengthscales and whether its noise is fixed."""

    def __init__(self, n_ls=1, fix_noise=False, noise_var=1e-2, handle=11):
        self.lengthscale = np.ones(n_ls)
        self.fix_noise, self.noise_var = fix_noise, noise_var
        self._handle = ctypes.c_void_p(handle)
        self.small, self.stale = True, True

    def generate_hyperparameters_samples(self, *a, **k):
        raise AssertionError("the sampler was reached")


class _Grid:
    def __init__(self, value):
        self._handle = ctypes.c_void_p(value)
        self.index_offset = 0
        self.points = np.zeros((3, 1))


def no_device(*a, **k):
    raise AssertionError("the device library was reached")


def test_the_entry_points_are_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, twin, n_args in (("cbo_acq_sweep_hyper_log", "cbo_acq_sweep_hyper", 11),
                               ("cbo_acq_sweep_sets_hyper_log", "cbo_acq_sweep_sets_hyper", 11), ("cbo_lse_rows", None, 6)):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} not declared in include/cbo_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name), f"{name} not exported by libcbo_hip.so"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args
        if twin:                                    # the EI form's argument list
            assert argtypes == _lib.SIGNATURES[twin][1]
    assert _lib.ABI_VERSION == 5 and lib.cbo_abi_version() == 5 and _lib.LOGMEI == "LOGMEI"


def test_the_library_refuses_bad_scalars_without_a_device():
    lib = _lib.load()
    vals, idxs = np.full(2, -7.0), np.full(2, -7, dtype=np.int64)
    good = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 0.0]])

    def sets(n_sets=2, counts=(2, 1), rows=(good, good), y_best=(0.1, 0.2), task=0, jitter=0.0, costs=(1.0, 2.0)):
        arr = lambda a: None if a is None else _lib.dptr(np.array(a, dtype=np.float64))                          # noqa: E731
        cnt = None if counts is None else (ctypes.c_int * len(counts))(*counts)
        ptrs = None if rows is None else (ctypes.c_void_p * len(rows))(*[None if r is None else r.ctypes.data for r in rows])
        return lib.cbo_acq_sweep_sets_hyper_log(n_sets, None, None, cnt, ptrs, arr(y_best), task, jitter, arr(costs),
                                                _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p))

    # cbo_acq_sweep_sets_hyper's refusals, and the log EI's scalar ones
    bad = ((dict(n_sets=0), b"n_sets"), (dict(counts=None), b"n_samples"), (dict(rows=None), b"hyper"),
           (dict(task=2), b"task"), (dict(counts=(0, 1)), b"samples"), (dict(counts=(2, 257)), b"samples"),
           (dict(rows=(good, None)), b"hyper"), (dict(costs=(1.0, 0.0)), b"cost"), (dict(costs=(1.0, np.nan)), b"cost"),
           (dict(jitter=np.nan), b"jitter"), (dict(jitter=np.inf), b"jitter"), (dict(y_best=(0.1, np.nan)), b"y_best"),
           (dict(y_best=(-np.inf, 0.2)), b"y_best"))
    for kw, word in bad:
        assert sets(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    assert sets() == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert np.all(vals == -7.0) and np.all(idxs == -7)

    # the single-set call: the log EI's scalars are refused first, then the NULL handles
    def one(y_best=0.1, jitter=0.0):
        return lib.cbo_acq_sweep_hyper_log(None, None, 2, _lib.dptr(good), y_best, 0, jitter, 1.0, None,
                                           ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int64()))
    assert one(jitter=np.nan) == _lib.CBO_ERR_INVALID and b"jitter" in lib.cbo_last_error()
    assert one(y_best=np.inf) == _lib.CBO_ERR_INVALID and b"y_best" in lib.cbo_last_error()
    assert one() == _lib.CBO_ERR_INVALID and b"NULL" in lib.cbo_last_error()

    terms, out = np.zeros((2, 3)), np.full(3, -7.0)
    assert lib.cbo_lse_rows(None, 2, 3, _lib.dptr(terms), 1.0, _lib.dptr(out)) == _lib.CBO_ERR_INVALID
    assert b"NULL" in lib.cbo_last_error() and np.all(out == -7.0)


ROWS = [np.array([[1.0, 1.0, 1e-2]]), np.array([[1.0, 1.0, 2.0, 3.0, 1e-2], [2.0, 1.0, 2.0, 3.0, 0.0]])]
# what "LOGMEI" does not combine with, by the keyword that says so
EXCLUDED_SETS = (dict(constraints=[[ProbabilityOfFeasibility(Untouchable())], []]), dict(batch_size=2), dict(refine=True),
                 dict(refine_constrained=True), dict(refine=True, device_prior=True), dict(cost_mode="pointwise"),
                 dict(raw=True))


def test_logmei_needs_samples_and_refuses_what_it_does_not_combine_with_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", no_device)
    obj = Untouchable()
    models = [_Model(1), _Model(3)]
    sweep = lambda hyper=ROWS, **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj],     # noqa: E731
                                                        acquisition="LOGMEI", hyper_samples=hyper, spaces=[obj, obj], **kw)
    with pytest.raises(ValueError, match="hyper_samples must be given"):
        sweep(None)
    for kw in EXCLUDED_SETS:
        with pytest.raises(ValueError, match="LOGMEI"):
            sweep(**kw)
    for bad in (np.nan, np.inf, "much"):
        with pytest.raises(ValueError, match="jitter"):
            sweep(acquisition_param=bad)
    with pytest.raises(ValueError, match="one entry per exploration set"):
        sweep(ROWS[:1])
    # the other kinds keep their message; LOGEI and LOGCEI keep raising with samples
    for other in ("LCB", "LOGEI"):
        with pytest.raises(ValueError, match="acquisition must be 'EI'"):
            find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition=other, hyper_samples=ROWS)
    with pytest.raises(ValueError):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition="LOGCEI", hyper_samples=ROWS,
                           constraints=[[], []])

    # the single-set function (no acquisition_param: the jitter is 0)
    point = lambda hyper=ROWS[0], **kw: find_next_y_point(obj, models[0], 0.0, ["X"], obj, acquisition="LOGMEI",   # noqa: E731
                                                          hyper_samples=hyper, **kw)
    with pytest.raises(ValueError, match="hyper_samples must be given"):
        point(None)
    for kw in (dict(constraints=[ProbabilityOfFeasibility(obj)]), dict(batch_size=2), dict(cost_mode="pointwise"),
               dict(anchors="uniform")):
        with pytest.raises(ValueError, match="LOGMEI"):
            point(**kw)
    for bad in (0, True):
        with pytest.raises(ValueError, match="positive int"):
            point(bad)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        find_next_y_point(obj, models[0], 0.0, ["X"], obj, acquisition="PI", hyper_samples=ROWS[0])

    # the path: an int or a callable, either sampler
    path = lambda hyper=3, **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj],        # noqa: E731
                                                               [obj, obj], [obj, obj], comm=None, acquisition="LOGMEI",
                                                               hyper_samples=hyper, **kw)
    with pytest.raises(ValueError, match="hyper_samples must be given"):
        path(None)
    col = np.zeros((3, 1))
    for kw in (dict(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]]), dict(batch_size=2), dict(refine=True),
               dict(refine=True, device_prior=True), dict(cost_mode="pointwise"),
               dict(refine_constrained=True, constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])):
        with pytest.raises(ValueError, match="LOGMEI"):
            path(**kw)
    for bad in (0, True, 257, "ten"):
        with pytest.raises(ValueError, match="hyper_samples"):
            path(bad)
    sampler = lambda model, s: ROWS[s]                                                                         # noqa: E731
    kept = path(sampler, acquisition_param=0.25)
    assert kept.hyper_samples is sampler and kept._kind == ("LOGMEI", 0.25)
    assert path(4, hyper_sampler="device").hyper_sampler == "device" and path(4)._kind == ("LOGMEI", 0.0)
    with pytest.raises(ValueError, match="callable"):
        path(sampler, hyper_sampler="device")


def test_the_agent_refuses_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", no_device)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data,   # noqa: E731
                                       acquisition="LOGMEI", **kw)
    with pytest.raises(ValueError, match="hyper_samples must be given"):
        make()
    for kw in (dict(constraints={"C": ("<=", 1.0)}), dict(batch_size=2), dict(refine=True), dict(cost_mode="pointwise"),
               dict(refine=True, device_prior=True), dict(refine_constrained=True, constraints={"C": ("<=", 1.0)})):
        with pytest.raises(ValueError, match="LOGMEI"):
            make(hyper_samples=3, **kw)
    with pytest.raises(ValueError, match="jitter"):
        make(hyper_samples=3, acquisition_param=np.nan)
    agent = make(hyper_samples=3, acquisition_param=0.5, hyper_sampler="device")
    assert agent.hyper_samples == 3 and agent._kind == ("LOGMEI", 0.5) and agent.hyper_rows == [None] * len(es)


class _StubLibrary:
    """Records the calls; every multi-set call reports set i's winner as (10 + i, i)."""

    def __init__(self):
        self.calls = []

    def _answer(self, s, vals, idxs):
        np.ctypeslib.as_array(vals, shape=(s,))[:] = 10.0 + np.arange(s)
        np.ctypeslib.as_array(idxs, shape=(s,))[:] = np.arange(s)
        return 0

    def _rows(self, s, gps, counts, ptrs):
        rows = []
        for i in range(s):
            width = {11: 3, 12: 5}[gps[i]]
            flat = np.ctypeslib.as_array(ctypes.cast(ptrs[i], _lib.c_double_p), shape=(counts[i] * width,))
            rows.append(flat.reshape(counts[i], width).copy())
        return rows

    def cbo_acq_sweep_sets(self, s, gps, cds, y_best, task, jitter, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets",))
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_hyper(self, s, gps, cds, counts, ptrs, y_best, task, jitter, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets_hyper", task, jitter, self._rows(s, gps, counts, ptrs)))
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_hyper_log(self, s, gps, cds, counts, ptrs, y_best, task, jitter, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets_hyper_log", task, jitter, self._rows(s, gps, counts, ptrs)))
        return self._answer(s, vals, idxs)

    def _single(self, name, gp, cands, n, hyper, y_best, task, jitter, cost, acq, best_val, best_idx):
        rows = np.ctypeslib.as_array(hyper, shape=(n * 3,)).reshape(n, 3).copy()
        self.calls.append((name, y_best, task, jitter, cost, rows))
        if acq:
            np.ctypeslib.as_array(acq, shape=(3,))[:] = (-3.0, -1.0, -2.0)
        best_val._obj.value, best_idx._obj.value = -1.0, 1
        return 0

    def cbo_acq_sweep_hyper(self, *a):
        return self._single("cbo_acq_sweep_hyper", *a)

    def cbo_acq_sweep_hyper_log(self, *a):
        return self._single("cbo_acq_sweep_hyper_log", *a)


def test_rows_take_the_log_entry_point_and_a_change_of_kind_drops_the_trial_arguments(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    models, grids = [_Model(1, fix_noise=True, noise_var=0.25, handle=11), _Model(3, handle=12)], [_Grid(21), _Grid(22)]
    models[1].small = False
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    cache = {}
    given = [np.array([[1.5, 0.7], [0.5, 2.0]]), np.array([[1.0, 1.0, 2.0, 3.0, 1e-2]])]
    call = lambda **kw: find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "max", grids, cache=cache,         # noqa: E731
                                           hyper_samples=given, **kw)
    # the EI form first: today's call, jitter 0
    call()
    assert stub.calls[-1][:3] == ("cbo_acq_sweep_sets_hyper", 1, 0.0)
    entry = cache["sweep_sets"]
    entry["trial_args"] = "made by a trial step"
    xs, ys = call(acquisition="LOGMEI", acquisition_param=0.125)
    name, task, jitter, rows = stub.calls[-1]
    assert (name, task, jitter) == ("cbo_acq_sweep_sets_hyper_log", 1, 0.125)
    assert np.array_equal(rows[0], [[1.5, 0.7, 0.25], [0.5, 2.0, 0.25]]) and np.array_equal(rows[1], given[1])
    assert [y.tolist() for y in ys] == [[[10.0]], [[11.0]]] and [x.shape for x in xs] == [(1, 1), (1, 1)]
    assert cache["sweep_sets"] is entry and "trial_args" not in entry and entry["kind"] == ("LOGMEI", 0.125)
    assert models[1].stale                                          # (the marginalised general path restores: not marked fitted)
    # the default jitter is 0; back to the EI form the entry drops the arguments again
    call(acquisition="LOGMEI")
    assert stub.calls[-1][:3] == ("cbo_acq_sweep_sets_hyper_log", 1, 0.0)
    entry["trial_args"] = "made by a trial step"
    call()
    assert stub.calls[-1][:3] == ("cbo_acq_sweep_sets_hyper", 1, 0.0) and "trial_args" not in entry
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache)
    assert stub.calls[-1] == ("cbo_acq_sweep_sets",) and len(stub.calls) == 5


def test_the_class_accepts_the_log_generator_and_refuses_the_others(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    model = _Model(1)
    samples = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 0.0]])
    cost = Cost({"X": lambda col: 4.0}, ["X"])
    grid = object.__new__(CandidateGrid)
    grid.points, grid._handle, grid.index_offset = np.zeros((3, 1)), ctypes.c_void_p(21), 0
    bare = IntegratedHyperParameterAcquisition(model, lambda m: CausalLogExpectedImprovement(0.5, "max", m, 0.25),
                                               samples=samples)
    over = IntegratedHyperParameterAcquisition(model, lambda m: CausalLogExpectedImprovement(0.5, "max", m, 0.25) / cost,
                                               samples=samples)
    plain = IntegratedHyperParameterAcquisition(model, lambda m: CausalExpectedImprovement(0.5, "max", m), samples=samples)
    assert bare.is_log and over.is_log and not plain.is_log and not bare.has_gradients
    res = bare.sweep(grid, want_acq=True)
    name, y_best, task, jitter, c, rows = stub.calls[-1]
    assert (name, y_best, task, jitter, c) == ("cbo_acq_sweep_hyper_log", 0.5, 1, 0.25, 1.0) and np.array_equal(rows, samples)
    assert (res["best_val"], res["best_idx"]) == (-1.0, 1) and res["acq"].tolist() == [[-3.0], [-1.0], [-2.0]]
    over.sweep(grid)
    assert stub.calls[-1][0] == "cbo_acq_sweep_hyper_log" and stub.calls[-1][4] == 4.0       # (the generator's Cost)
    plain.sweep(grid)
    assert stub.calls[-1][0] == "cbo_acq_sweep_hyper" and stub.calls[-1][3] == 0.0
    from cbo_with_oop_amd.utils_functions.constrained import ConstrainedLogExpectedImprovement
    others = (lambda m: CausalProbabilityOfImprovement(0.5, "min", m),
              lambda m: CausalProbabilityOfImprovement(0.5, "min", m) / cost,
              lambda m: ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(0.5, "min", m), []) / cost)
    for generator in others:
        with pytest.raises(TypeError, match="CausalExpectedImprovement"):
            IntegratedHyperParameterAcquisition(model, generator, samples=samples)


# ---- the reduction of csrc/lse_stream.h, restated: start, push in sample order, close ------------------------------------
def lse_stream(terms, cost):
    """numpy's restatement of lse_start / lse_push / lse_close over the rows of ``terms`` (H, m): one rounding per
    operation, numpy's exp and log in the place of the device library's."""
    terms = np.asarray(terms, dtype=np.float64)
    out = np.empty(terms.shape[1])
    with np.errstate(all="ignore"):
        for i in range(terms.shape[1]):
            M, S = terms[0, i], np.float64(1.0)
            for l in terms[1:, i]:
                if l > M:
                    S = S * np.exp(M - l) + np.float64(1.0)
                    M = l
                elif l == M:
                    S = S + np.float64(1.0)
                else:
                    S = S + np.exp(l - M)
            out[i] = ((M + np.log(S)) - np.log(np.float64(terms.shape[0]))) - np.log(np.float64(cost))
    return out


def lse_reference(terms, cost):
    """log((1 / H) sum_h exp(l_h)) - log cost of the same doubles in 60 digits."""
    import mpmath
    terms = np.asarray(terms, dtype=np.float64)
    out = []
    with mpmath.workdps(60):
        for i in range(terms.shape[1]):
            col = [mpmath.mpf(float(v)) for v in terms[:, i]]
            top = max(col)
            total = mpmath.fsum(mpmath.exp(v - top) for v in col)
            out.append(top + mpmath.log(total) - mpmath.log(terms.shape[0]) - mpmath.log(mpmath.mpf(float(cost))))
    return out


def lse_error_in_bar_units(got, ref, n_terms):
    """|got - ref| / (2^-53 (H + |ref|)): the bar of DESIGN.md §4ac is 4 in these units."""
    import mpmath
    with mpmath.workdps(60):
        return max(float(abs(mpmath.mpf(float(g)) - r) / (mpmath.mpf(2) ** -53 * (n_terms + abs(r)))) for g, r in zip(got, ref))


@pytest.mark.parametrize("n_terms", (1, 2, 3, 10, 50))
def test_the_restated_reduction_meets_its_bound_against_mpmath(n_terms):
    rng = np.random.default_rng(100 + n_terms)
    m = 300
    close = rng.normal(-20.0, 3.0, (n_terms, m))                    # terms of similar size: every exp counts
    spread = rng.uniform(-700.0, 5.0, (n_terms, m))                 # a few nats to hundreds apart
    far = rng.normal(0.0, 1.0, (n_terms, m)) + 1e8 * rng.integers(-4, 1, (n_terms, m))   # 1e8 apart: exp underflows to 0
    for terms in (close, spread, far):
        for cost in (1.0, 3.7):
            got = lse_stream(terms, cost)
            worst = lse_error_in_bar_units(got, lse_reference(terms, cost), n_terms)
            assert worst <= 4.0, (n_terms, cost, worst)
    if n_terms > 1:
        assert np.all(np.exp(far.min(axis=0) - far.max(axis=0))[np.ptp(far, axis=0) > 1e7] == 0.0)


def test_the_restated_reduction_keeps_its_contracts():
    inf, nan = np.inf, np.nan
    # one term: the term itself minus the log cost, to the bit
    one = np.array([[-4.9e8, -1.25, 0.0, 700.0, -inf]])
    assert np.array_equal(lse_stream(one, 1.0), one[0])
    assert np.array_equal(lse_stream(one, 3.0)[:4], one[0, :4] - np.log(3.0))
    # -inf is an ordinary value: all samples at -inf give -inf, one finite sample gives it minus log H
    terms = np.array([[-inf, -inf, -2.0, -inf], [-inf, -2.0, -inf, -inf], [-inf, -inf, -inf, -5.0]])
    got = lse_stream(terms, 1.0)
    assert got[0] == -inf and np.array_equal(got[1:], np.array([-2.0, -2.0, -5.0]) - np.log(3.0))
    # NaN propagates from any position
    for pos in range(3):
        terms = np.array([[-1.0], [-2.0], [-3.0]])
        terms[pos, 0] = nan
        assert np.isnan(lse_stream(terms, 1.0)[0])
    # equal terms count exactly (S = 8, no exp): H equal terms give the term back within the close's two roundings
    assert abs(lse_stream(np.full((8, 1), -123.456), 1.0)[0] + 123.456) <= 2.0 ** -52 * 126.0
    # the three branches in one column: the maximum rises, is met again, and is undercut
    assert math.isclose(lse_stream(np.array([[-3.0], [-1.0], [-1.0], [-2.0]]), 1.0)[0],
                        math.log((math.exp(-3) + 2 * math.exp(-1) + math.exp(-2)) / 4), rel_tol=1e-15)
