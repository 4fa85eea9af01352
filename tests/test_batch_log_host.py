"""CPU tests of greedy batch selection in log space: cbo_acq_sweep_batch_logei and
cbo_acq_sweep_sets_batch_logei are declared, exported and prototyped as their siblings and refuse bad scalars without a device;
``acquisition="LOGBEI"`` is routed by name to the one new multi-set call, requires a ``batch_size`` and refuses what it does
not combine with before the device library is loaded; and the numpy restatement of the believer with the host log EI in the
place of the EI -- ``log_believer`` below, the loop of ``sets_batch_support.believer``, which the GPU tests compare the device
with -- reproduces the dead-region table of §4ad and, where the EI is representable, the EI believer's picks.  The device's
values are checked on the GPU (tests/test_batch_log_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_fixture
from oracle import gp_oracle as O
from sets_batch_support import believer, model_args
from test_sets_batch_host import Untouchable, _Grid, _Model

from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility, find_next_y_point, find_next_y_points
from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def log_believer(f, batch_size, y_best=None, task=None, cost=None, update_incumbent=False, jitter=0.0):
    """``sets_batch_support.believer``'s loop scored by the host log EI (``CausalLogExpectedImprovement.log_ei``) minus
    log cost.  Returns idx (B,), val (B,), gap (B,) -- the relative distance between the best and the runner-up, as the EI
    believer reports it -- log_gap (B,) -- their absolute distance in log value -- the data every pick was fitted on, the
    incumbent every pick saw and acq / mean / var at the last pick."""
    X, y, mX, vX = f["X"], f["y"], f["mX"], f["vX"]
    Xs, mXs, vXs = f["Xs"], f["mXs"], f["vXs"]
    y_best = float(f["y_best"]) if y_best is None else float(y_best)
    task = f["task"] if task is None else task
    cost = float(f["cost"]) if cost is None else float(cost)
    out = dict(idx=[], val=[], gap=[], log_gap=[], data=[], y_best=[])
    for _ in range(batch_size):
        post = O.fit(X, y, mX, vX, **model_args(f))
        _, _, _, mean, var = O.acquisition_sweep(post, Xs, y_best, mXs, vXs, task, cost, 0.0)
        a = CausalLogExpectedImprovement.log_ei(mean[:, 0], np.sqrt(var[:, 0]), y_best, task, jitter) - np.log(cost)
        idx = int(np.argmax(a))
        val = float(a[idx])
        runner_up = np.max(np.delete(a, idx)) if a.size > 1 else -np.inf
        out["gap"].append(abs(val - runner_up) / max(abs(val), 1e-300))
        out["log_gap"].append(val - runner_up)
        out["idx"].append(idx); out["val"].append(val); out["data"].append((X, y, mX, vX)); out["y_best"].append(y_best)
        out.update(acq=a, mean=mean, var=var)
        y_new = float(mean[idx, 0])
        X = np.vstack([X, Xs[idx:idx + 1]])
        y = np.vstack([y, [[y_new]]])
        if mX is not None:
            mX = np.vstack([mX, mXs[idx:idx + 1]])
            vX = np.vstack([vX, vXs[idx:idx + 1]])
        if update_incumbent:
            y_best = min(y_best, y_new) if task == "min" else max(y_best, y_new)
    for k in ("val", "gap", "log_gap"):
        out[k] = np.array(out[k])
    out["idx"] = np.array(out["idx"], dtype=np.int64)
    return out


def dead_region_problem():
    """The recipe of DESIGN.md §4x / §4ad as a fixture dictionary: 50 noise-free observations of cos x - exp(-x / 20) on
    [-5, 20], hyper-parameters (1, 1, 1e-10), a grid of 200, task 'min', cost 1."""
    X = np.random.default_rng(7).uniform(-5.0, 20.0, (50, 1))
    Y = np.cos(X) - np.exp(-X / 20.0)
    return dict(X=X, y=Y, mX=None, vX=None, Xs=np.linspace(-5.0, 20.0, 200)[:, None], mXs=None, vXs=None, variance=1.0,
                lengthscale_arg=1.0, noise_var=1e-10, task="min", cost=1.0, y_best=float(Y.min()))


# incumbent below Y.min() -> (EI picks, EI values, log picks, log values, relative gaps): the table of the issue and of §4ad
DEAD_REGION = {0.5: ([69, 15, 0, 0, 0], [9.7e-148, 5.3e-265, 0.0, 0.0, 0.0], [69, 15, 191, 80, 23],
                     [-338.5, -608.5, -1735.0, -1900.0, -11436.0], [0.098, 0.075, 0.066, 0.0086, 0.067]),
               3.0: ([0, 0, 0, 0, 0], [0.0] * 5, [79, 191, 23, 69, 142],
                     [-1958.0, -5516.0, -17409.0, -25135.0, -60563.0], [0.068, 0.073, 0.0017, 0.028, 0.085])}


def two_digits(values):
    return [float(f"{v:.2g}") for v in values]


@pytest.mark.parametrize("below", [0.5, 3.0])
def test_the_restatement_reproduces_the_dead_region_table(below):
    f = dead_region_problem()
    y_best = f["y_best"] - below
    ei_idx, ei_val, log_idx, log_val, gaps = DEAD_REGION[below]
    ei = believer(f, 5, y_best=y_best)
    lg = log_believer(f, 5, y_best=y_best)
    print(below, "EI", ei["idx"].tolist(), ei["val"].tolist())
    print(below, "log", lg["idx"].tolist(), lg["val"].tolist(), lg["gap"].tolist())
    assert ei["idx"].tolist() == ei_idx and two_digits(ei["val"]) == ei_val
    assert lg["idx"].tolist() == log_idx
    # the table rounds to one decimal below 1000 and to integers above
    for got, want in zip(lg["val"], log_val):
        assert abs(got - want) <= (0.05 if abs(want) < 1000 else 0.5) * (1 + 1e-9), (got, want)
    assert two_digits(lg["gap"]) == gaps
    assert np.all(np.isfinite(lg["val"])) and np.all(np.diff(lg["val"]) < 0)
    # update_incumbent changes neither row: a believed mean never reaches these incumbents
    moved = log_believer(f, 5, y_best=y_best, update_incumbent=True)
    assert moved["idx"].tolist() == log_idx and moved["y_best"] == [y_best] * 5
    assert believer(f, 5, y_best=y_best, update_incumbent=True)["idx"].tolist() == ei_idx


@pytest.mark.parametrize("update", [False, True])
@pytest.mark.parametrize("name", ["causal_d2", "graph_ard_d4", "complete_bo_d3"])
def test_where_the_ei_is_representable_the_log_believer_picks_the_ei_believers_indices(name, update):
    f = load_fixture(name)
    ei = believer(f, 4, update_incumbent=update)
    lg = log_believer(f, 4, update_incumbent=update)
    print(name, update, ei["idx"].tolist(), lg["idx"].tolist(), "log gaps", lg["log_gap"].tolist())
    assert lg["idx"].tolist() == ei["idx"].tolist()
    assert np.all(lg["log_gap"] > 1e-6), lg["log_gap"]             # (measured: at least 1e-2)
    assert np.all(ei["val"] > 0)
    np.testing.assert_allclose(np.exp(lg["val"]), ei["val"], rtol=1e-9)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_prototyped_as_their_siblings():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, sibling in (("cbo_acq_sweep_batch_logei", "cbo_acq_sweep_batch"),
                          ("cbo_acq_sweep_sets_batch_logei", "cbo_acq_sweep_sets_batch")):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} not declared in include/cbo_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes == _lib.SIGNATURES[sibling][1]
        assert len(decl.group(1).split(",")) == len(argtypes)
        assert hasattr(lib, name), f"{name} not exported by libcbo_hip.so"
    assert _lib.ABI_VERSION == 5 and lib.cbo_abi_version() == 5
    # routed by name: no kind code
    assert "LOGBEI" not in _lib.ACQ_KIND_CODE and "LOGBEI" not in _lib.REFINE_KIND_CODE


BAD_SCALARS = ((dict(task=2), b"task"), (dict(task=-1), b"task"), (dict(jitter=np.nan), b"jitter"),
               (dict(jitter=np.inf), b"jitter"), (dict(cost=0.0), b"cost"), (dict(cost=-1.0), b"cost"),
               (dict(cost=np.nan), b"cost"), (dict(batch_size=0), b"batch_size"), (dict(batch_size=65), b"batch_size"),
               (dict(batch_size=-1), b"batch_size"), (dict(update=2), b"update_incumbent"))


def test_the_single_set_call_refuses_bad_scalars_and_null_handles():
    lib = _lib.load()
    vals, idxs = np.full(3, -7.0), np.full(3, -7, dtype=np.int64)

    def call(y_best=0.1, task=0, jitter=0.0, cost=1.0, batch_size=3, update=0):
        return lib.cbo_acq_sweep_batch_logei(None, None, y_best, task, jitter, cost, batch_size, update, _lib.dptr(vals),
                                             idxs.ctypes.data_as(_lib.c_int64_p), None, None, None)

    for kw, word in BAD_SCALARS + ((dict(y_best=np.nan), b"y_best"), (dict(y_best=-np.inf), b"y_best")):
        assert call(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    for B in (1, 3, 64):                                            # valid scalars: the NULL handles are what is refused
        assert call(batch_size=B) == _lib.CBO_ERR_INVALID
        assert not any(w in lib.cbo_last_error() for w in (b"task", b"jitter", b"cost", b"batch_size", b"update", b"y_best"))
    assert np.all(vals == -7.0) and np.all(idxs == -7)


def test_the_multi_set_call_refuses_bad_scalars_and_arrays_with_null_handle_arrays():
    lib = _lib.load()
    vals, idxs = np.full(6, -7.0), np.full(6, -7, dtype=np.int64)

    def call(n_sets=2, y_best=(0.1, 0.2), task=0, jitter=0.0, cost=None, costs=(1.0, 2.0), batch_size=3, update=0,
             outputs=True):
        if cost is not None:
            costs = (1.0, cost)
        arr = lambda a: None if a is None else _lib.dptr(np.array(a, dtype=np.float64))                          # noqa: E731
        return lib.cbo_acq_sweep_sets_batch_logei(n_sets, None, None, arr(y_best), task, jitter, arr(costs), batch_size,
                                                  update, _lib.dptr(vals) if outputs else None,
                                                  idxs.ctypes.data_as(_lib.c_int64_p) if outputs else None)

    bad = BAD_SCALARS + ((dict(n_sets=0), b"n_sets"), (dict(y_best=None), b"y_best"), (dict(costs=None), b"costs"),
                         (dict(outputs=False), b"best_vals"), (dict(y_best=(0.1, np.nan)), b"y_best"),
                         (dict(y_best=(np.inf, 0.2)), b"y_best"))
    for kw, word in bad:
        assert call(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    for B in (1, 3, 64):
        assert call(batch_size=B) == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert np.all(vals == -7.0) and np.all(idxs == -7)


# ---- the name ----------------------------------------------------------------------------------------------------------------
class _StubLibrary:
    """Records the multi-set calls; the batch calls report pick t of set i as (10 i + t, 100 + i + t)."""

    def __init__(self):
        self.calls = []

    def _batch(self, name, s, y_best, task, jitter, costs, batch_size, update, vals, idxs):
        self.calls.append((name, s, task, jitter, batch_size, update, np.ctypeslib.as_array(y_best, shape=(s,)).tolist(),
                           np.ctypeslib.as_array(costs, shape=(s,)).tolist()))
        v = np.ctypeslib.as_array(vals, shape=(s * batch_size,)).reshape(s, batch_size)
        ix = np.ctypeslib.as_array(idxs, shape=(s * batch_size,)).reshape(s, batch_size)
        for i in range(s):
            v[i] = 10.0 * i + np.arange(batch_size)
            ix[i] = 100 + i + np.arange(batch_size)
        return 0

    def cbo_acq_sweep_sets_batch(self, s, gps, cds, y_best, task, jitter, costs, batch_size, update, vals, idxs):
        return self._batch("cbo_acq_sweep_sets_batch", s, y_best, task, jitter, costs, batch_size, update, vals, idxs)

    def cbo_acq_sweep_sets_batch_logei(self, s, gps, cds, y_best, task, jitter, costs, batch_size, update, vals, idxs):
        return self._batch("cbo_acq_sweep_sets_batch_logei", s, y_best, task, jitter, costs, batch_size, update, vals, idxs)


def test_logbei_makes_exactly_one_call_and_reshapes_its_set_major_outputs(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    models, grids = [_Model(11), _Model(12, small=False)], [_Grid(21), _Grid(22)]
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    cache = {}
    xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "max", grids, cache=cache, acquisition="LOGBEI",
                                acquisition_param=0.25, batch_size=3, update_incumbent=True)
    assert stub.calls == [("cbo_acq_sweep_sets_batch_logei", 2, 1, 0.25, 3, 1, [0.3, 0.3], [1.0, 2.0])]
    assert [x.shape for x in xs] == [(3, 2), (3, 2)] and [y.shape for y in ys] == [(3, 1), (3, 1)]
    assert ys[0][:, 0].tolist() == [0.0, 1.0, 2.0] and ys[1][:, 0].tolist() == [10.0, 11.0, 12.0]
    assert xs[0][:, 0].tolist() == [0.0, 1.0, 2.0] and xs[1][:, 0].tolist() == [1.0, 2.0, 3.0]
    assert not models[1].stale and models[0].stale                   # (the general path fits a larger model)
    # the default jitter is 0; "EI" with a batch keeps today's call on the same cache entry
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, acquisition="LOGBEI", batch_size=2)
    assert stub.calls[-1] == ("cbo_acq_sweep_sets_batch_logei", 2, 0, 0.0, 2, 0, [0.3, 0.3], [1.0, 2.0])
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, batch_size=2)
    assert stub.calls[-1] == ("cbo_acq_sweep_sets_batch", 2, 0, 0.0, 2, 0, [0.3, 0.3], [1.0, 2.0]) and len(stub.calls) == 3
    # variable costs: a later pick's LOG value moves from the batch's cost to the point's own by the two logarithms
    var = {"X": lambda col: 1.0 + np.sum(np.abs(col))}
    grids1 = [_Grid(21)]

    class _LogEI:
        def __init__(self, *a):
            pass

        def sweep(self, x, cost, want_acq):
            return {"acq": np.array([[-5.0 - np.log(cost)]])}
    from cbo_with_oop_amd.utils_functions import pointwise_acquisitions
    monkeypatch.setattr(pointwise_acquisitions, "CausalLogExpectedImprovement", _LogEI)
    xs, ys = find_next_y_points(models[:1], 0.3, [["X"]], var, "min", grids1, acquisition="LOGBEI", batch_size=3)
    batch_cost = 1.0 + np.sum(np.abs(grids1[0].points[:, :1]))
    assert stub.calls[-1][0] == "cbo_acq_sweep_sets_batch_logei" and stub.calls[-1][-1] == [batch_cost]
    assert ys[0][0, 0] == -5.0 - np.log(1.0)
    assert ys[0][1, 0] == (1.0 + np.log(batch_cost)) - np.log(2.0) and ys[0][2, 0] == (2.0 + np.log(batch_cost)) - np.log(3.0)


def test_logbei_requires_a_batch_and_refuses_what_it_does_not_combine_with_before_the_library_is_loaded(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    obj = Untouchable()
    models, boxes = [_Model(11), _Model(12)], [[(0.0, 1.0)], [(0.0, 1.0)]]
    sweep = lambda **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj],      # noqa: E731
                                            acquisition="LOGBEI", **kw)
    with pytest.raises(ValueError, match="without a batch the acquisition is 'LOGEI'"):
        sweep()
    refused = (("constraints", dict(constraints=[[ProbabilityOfFeasibility(obj)], []])),
               ("hyper_samples", dict(hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])),
               ("refine", dict(refine=True, spaces=boxes)),
               ("refine_constrained", dict(refine_constrained=True, spaces=boxes)),
               ("device_prior", dict(device_prior=True)), ("cost_mode", dict(cost_mode="pointwise")),
               ("raw", dict(raw=True)))
    for word, kw in refused:
        with pytest.raises(ValueError, match=word):
            sweep(batch_size=3, **kw)
    for bad in (0, -2, True, 2.5, "three", 65):
        with pytest.raises(ValueError, match="batch_size"):
            sweep(batch_size=bad)
    for bad in (np.nan, np.inf, "x"):
        with pytest.raises(ValueError, match="jitter"):
            sweep(batch_size=3, acquisition_param=bad)
    with pytest.raises(ValueError, match="task"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "most", [obj, obj], acquisition="LOGBEI", batch_size=3)
    # the single-set function
    single = lambda **kw: find_next_y_point(obj, obj, 0.0, ["X"], obj, acquisition="LOGBEI", **kw)      # noqa: E731
    with pytest.raises(ValueError, match="without a batch the acquisition is 'LOGEI'"):
        single()
    for word, kw in (("constraints", dict(constraints=[ProbabilityOfFeasibility(obj)])), ("hyper_samples", dict(hyper_samples=4)),
                     ("cost_mode", dict(cost_mode="pointwise")), ("anchors", dict(anchors="uniform"))):
        with pytest.raises(ValueError, match=word):
            single(batch_size=3, **kw)
    # the path
    path = lambda **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes,  # noqa: E731
                                                      comm=None, acquisition="LOGBEI", **kw)
    with pytest.raises(ValueError, match="without a batch the acquisition is 'LOGEI'"):
        path()
    col = np.zeros((3, 1))
    for word, kw in (("constraints", dict(constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])),
                     ("hyper_samples", dict(hyper_samples=4)), ("refine", dict(refine=True)),
                     ("refine_constrained", dict(refine_constrained=True)), ("device_prior", dict(device_prior=True)),
                     ("cost_mode", dict(cost_mode="pointwise"))):
        with pytest.raises(ValueError, match=word):
            path(batch_size=3, **kw)
    kept = path(batch_size=3, update_incumbent=True, acquisition_param=0.5)
    assert kept.batch_size == 3 and kept.update_incumbent is True and kept._kind == ("LOGBEI", 0.5)

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], boxes, comm=Two(),
                                          acquisition="LOGBEI", batch_size=3)
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    # the agent
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data,      # noqa: E731
                                       acquisition="LOGBEI", **kw)
    with pytest.raises(ValueError, match="without a batch the acquisition is 'LOGEI'"):
        make()
    for word, kw in (("constraints", dict(constraints={"C": ("<=", 1.0)})), ("hyper_samples", dict(hyper_samples=5)),
                     ("refine", dict(refine=True)), ("cost_mode", dict(cost_mode="pointwise"))):
        with pytest.raises(ValueError, match=word):
            make(batch_size=3, **kw)
    agent = make(batch_size=3, update_incumbent=True)
    assert agent.batch_size == 3 and agent.update_incumbent is True and agent._kind == ("LOGBEI", 0.0)
    # ... and the other names keep refusing a batch, LOGEI included
    for name in ("LOGEI", "LCB", "PI", "MPEI", "VAR", "MES", "LOGCEI", "LOGMEI"):
        with pytest.raises(ValueError):
            find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj], acquisition=name, batch_size=3)
    with pytest.raises(ValueError, match="batch"):
        find_next_y_point(obj, obj, 0.0, ["X"], obj, acquisition="LOGEI", batch_size=2)
    from cbo_with_oop_amd.utils_functions.utils import checked_batch_size
    assert checked_batch_size(3, ("EI", None)) == 3 and checked_batch_size(3, ("LOGBEI", 0.0)) == 3
    for name in ("LOGEI", "PI", "LOGCEI", "LOGMEI", "MES"):
        with pytest.raises(ValueError, match="acquisition must be 'EI'"):
            checked_batch_size(3, (name, 0.0))


# ---- the classes -------------------------------------------------------------------------------------------------------------
class _PlainModel:
    causal = False


def test_the_calculator_accepts_the_log_ei_bare_and_over_a_cost_and_refuses_a_pointwise_cost(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    from cbo_with_oop_amd.utils_functions import (CausalGradientAcquisitionOptimizer, Cost, GreedyBatchPointCalculator,
                                                  PointwiseCost)
    from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import LogAcquisitionQuotient
    model = _PlainModel()
    log_ei = CausalLogExpectedImprovement(0.0, "min", model)
    opt = CausalGradientAcquisitionOptimizer([(0.0, 1.0)], grid_shape=[8])
    assert GreedyBatchPointCalculator(model, log_ei, opt, 3).batch_size == 3
    quotient = log_ei / Cost({"X": lambda col: 2.0}, ["X"])
    assert isinstance(quotient, LogAcquisitionQuotient)
    assert GreedyBatchPointCalculator(model, quotient, opt, np.int64(2)).batch_size == 2
    # the quotient hands the cost over as AcquisitionQuotient.sweep_batch does
    seen = {}
    monkeypatch.setattr(CausalLogExpectedImprovement, "sweep_batch",
                        lambda self, candidates, batch_size, **kw: seen.update(kw, batch_size=batch_size) or "result")
    assert quotient.sweep_batch(np.zeros((4, 1)), 2, update_incumbent=True) == "result"
    assert seen == dict(cost=2.0, batch_size=2, update_incumbent=True)
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "load", no_device)
    # a per-candidate cost has no batch form: refused at the latest when the batch is asked for, before any device call
    from functools import partial
    from cbo_with_oop_amd import graphs
    pointwise = log_ei / PointwiseCost({"X": partial(graphs.cost, 1.0, True)}, ["X"])
    opt._grid, opt._grid_model = _Grid(21), model
    with pytest.raises(ValueError, match="PointwiseCost"):
        GreedyBatchPointCalculator(model, pointwise, opt, 2).compute_next_points()
    opt._grid = None
    for bad in (0, 1.5, None, False):
        with pytest.raises(ValueError, match="batch_size"):
            log_ei.sweep_batch(np.zeros((4, 1)), bad)
    for other in (CausalGradientAcquisitionOptimizer([(0.0, 1.0)], grid_shape=[8], anchors="uniform"),):
        with pytest.raises(ValueError, match="anchors"):
            GreedyBatchPointCalculator(model, log_ei, other, 2)
