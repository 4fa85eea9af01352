"""CPU tests of greedy batch selection in the multi-set sweep and the agent: cbo_acq_sweep_sets_batch is
declared, exported and prototyped and refuses bad scalars and arrays without a device; the Python argument checks fire before
a device or a grid is touched; batch_size=None leaves find_next_y_points on today's call, and a positive batch_size takes the
one new call with its set-major outputs reshaped; the agent's monitor appends a batch's rows in order.  The values are
checked on the GPU (tests/test_sets_batch_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility, find_next_y_points


class Untouchable:
    """Argument checks must not touch grids or cost tables."""

    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


class _Model:
    def __init__(self, handle=11, small=True):
        self._handle = ctypes.c_void_p(handle)
        self.small, self.stale = small, True


class _Grid:
    def __init__(self, value, m=5):
        self._handle = ctypes.c_void_p(value)
        self.index_offset = 100
        self.points = np.arange(float(m))[:, None] * np.array([[1.0, -1.0]])


def test_the_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+cbo_acq_sweep_sets_batch\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, "cbo_acq_sweep_sets_batch not declared in include/cbo_hip.h"
    assert len(decl.group(1).split(",")) == 11
    assert hasattr(_lib.load(), "cbo_acq_sweep_sets_batch"), "not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_sets_batch"]
    assert restype is ctypes.c_int and len(argtypes) == 11
    # cbo_acq_sweep_sets' arguments with the batch size and the incumbent switch in front of the outputs
    sets = _lib.SIGNATURES["cbo_acq_sweep_sets"][1]
    assert argtypes == sets[:7] + [ctypes.c_int, ctypes.c_int] + sets[7:]
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5
    assert _lib.MAX_BATCH == 64 and re.search(r"#define\s+CBO_MAX_BATCH\s+64\b", text)


def test_the_library_refuses_bad_scalars_and_arrays_with_null_handle_arrays():
    lib = _lib.load()
    vals, idxs = np.full(6, -7.0), np.full(6, -7, dtype=np.int64)

    def call(n_sets=2, y_best=(0.1, 0.2), task=0, costs=(1.0, 2.0), batch_size=3, update=0, outputs=True):
        arr = lambda a: None if a is None else _lib.dptr(np.array(a, dtype=np.float64))                          # noqa: E731
        return lib.cbo_acq_sweep_sets_batch(n_sets, None, None, arr(y_best), task, 0.0, arr(costs), batch_size, update,
                                            _lib.dptr(vals) if outputs else None,
                                            idxs.ctypes.data_as(_lib.c_int64_p) if outputs else None)

    bad = ((dict(n_sets=0), b"n_sets"), (dict(n_sets=-3), b"n_sets"), (dict(y_best=None), b"y_best"),
           (dict(costs=None), b"costs"), (dict(outputs=False), b"best_vals"), (dict(task=2), b"task"), (dict(task=-1), b"task"),
           (dict(batch_size=0), b"batch_size"), (dict(batch_size=65), b"batch_size"), (dict(batch_size=-1), b"batch_size"),
           (dict(update=2), b"update_incumbent"), (dict(update=-1), b"update_incumbent"),
           (dict(costs=(1.0, 0.0)), b"cost"), (dict(costs=(-1.0, 1.0)), b"cost"), (dict(costs=(1.0, np.nan)), b"cost"),
           (dict(y_best=(0.1, np.nan)), b"y_best"), (dict(y_best=(np.inf, 0.2)), b"y_best"),
           (dict(y_best=(0.1, -np.inf)), b"y_best"))
    for kw, word in bad:
        assert call(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    # valid scalars: the NULL handle arrays are what is refused -- for a batch of one (cbo_acq_sweep_sets' route) too
    for B in (1, 3, 64):
        assert call(batch_size=B) == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert np.all(vals == -7.0) and np.all(idxs == -7)


def test_python_argument_checks_fire_before_a_device_or_a_grid_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    params = inspect.signature(find_next_y_points).parameters
    assert params["batch_size"].default is None and params["update_incumbent"].default is False
    obj = Untouchable()
    models = [_Model(11), _Model(12)]
    sweep = lambda batch, **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj],      # noqa: E731
                                                   batch_size=batch, **kw)
    for bad in (0, -2, True, 2.5, "three", [3]):
        with pytest.raises(ValueError, match="positive int"):
            sweep(bad)
    with pytest.raises(ValueError, match="at most 64"):
        sweep(65)
    for name in ("LCB", "PI", "MPEI", "VAR", "MES"):
        with pytest.raises(ValueError, match="acquisition must be 'EI'"):
            sweep(3, acquisition=name)
    with pytest.raises(ValueError, match="constraints"):
        sweep(3, constraints=[[ProbabilityOfFeasibility(obj)], []])
    with pytest.raises(ValueError, match="hyper_samples"):
        sweep(3, hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
    with pytest.raises(ValueError, match="raw"):
        sweep(3, raw=True)
    with pytest.raises(ValueError, match="task"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "most", [obj, obj], batch_size=3)
    # above a grid's size: the grids are read, the device is not
    costs = {"X": lambda col: 1.0, "Z": lambda col: 1.0}
    with pytest.raises(ValueError, match="exceeds the 5 candidates of set 1"):
        find_next_y_points(models, 0.0, [["X"], ["Z"]], costs, "min", [_Grid(21, 9), _Grid(22, 5)], batch_size=6)
    # the path and the agent
    path = lambda batch, **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj],   # noqa: E731
                                                             [obj, obj], comm=None, batch_size=batch, **kw)
    for bad in (0, -1, True, 65, 2.5, "ten"):
        with pytest.raises(ValueError, match="batch_size"):
            path(bad)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        path(3, acquisition="PI")
    col = np.zeros((3, 1))
    with pytest.raises(ValueError, match="constraints"):
        path(3, constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    with pytest.raises(ValueError, match="hyper_samples"):
        path(3, hyper_samples=4)
    kept = path(3, update_incumbent=True)
    assert kept.batch_size == 3 and kept.update_incumbent is True
    assert path(None).batch_size is None and path(None).update_incumbent is False

    class Two:
        world, rank = 2, 0
    other = cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], [obj, obj], comm=Two(),
                                          batch_size=3)
    with pytest.raises(ValueError, match="single process"):
        other.compute_best_acquisition_values(0.0)
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["batch_size"].default is None and sig["update_incumbent"].default is False


def test_the_agent_refuses_a_bad_batch_size_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data, **kw)  # noqa: E731
    for bad in (0, True, 65, "ten"):
        with pytest.raises(ValueError, match="batch_size"):
            make(batch_size=bad)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        make(batch_size=3, acquisition="LCB")
    with pytest.raises(ValueError, match="constraints"):
        make(batch_size=3, constraints={"C": ("<=", 1.0)})
    with pytest.raises(ValueError, match="hyper_samples"):
        make(batch_size=3, hyper_samples=5)
    agent = make(batch_size=3, update_incumbent=True)
    assert agent.batch_size == 3 and agent.update_incumbent is True and make().batch_size is None


class _StubLibrary:
    """Records the multi-set calls.  The plain call reports set i's winner as (10 + i, 100 + i); the batch call pick t of
    set i as (10 i + t, 100 + i + t)."""

    def __init__(self):
        self.calls = []

    def cbo_acq_sweep_sets(self, s, gps, cds, y_best, task, jitter, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets",))
        np.ctypeslib.as_array(vals, shape=(s,))[:] = 10.0 + np.arange(s)
        np.ctypeslib.as_array(idxs, shape=(s,))[:] = 100 + np.arange(s)
        return 0

    def cbo_acq_sweep_sets_batch(self, s, gps, cds, y_best, task, jitter, costs, batch_size, update, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets_batch", s, task, jitter, batch_size, update,
                           np.ctypeslib.as_array(y_best, shape=(s,)).tolist(), np.ctypeslib.as_array(costs, shape=(s,)).tolist()))
        v = np.ctypeslib.as_array(vals, shape=(s * batch_size,)).reshape(s, batch_size)
        ix = np.ctypeslib.as_array(idxs, shape=(s * batch_size,)).reshape(s, batch_size)
        for i in range(s):
            v[i] = 10.0 * i + np.arange(batch_size)
            ix[i] = 100 + i + np.arange(batch_size)
        return 0


def test_none_stays_on_todays_call_and_a_batch_size_takes_the_one_new_call(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    models, grids = [_Model(11), _Model(12, small=False)], [_Grid(21), _Grid(22)]
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    cache = {}
    xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, batch_size=None)
    assert [y.tolist() for y in ys] == [[[10.0]], [[11.0]]] and stub.calls == [("cbo_acq_sweep_sets",)]
    assert [x.tolist() for x in xs] == [[[0.0, -0.0]], [[1.0, -1.0]]]
    entry = cache["sweep_sets"]
    assert entry["batch_size"] is None
    # a batch: the one new call, set-major outputs as (B, d) points and (B, 1) values, on the same cache entry
    models[1].stale = True
    entry["trial_args"] = "made by a trial step"
    xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "max", grids, cache=cache, batch_size=3,
                                update_incumbent=True)
    assert stub.calls[-1] == ("cbo_acq_sweep_sets_batch", 2, 1, 0.0, 3, 1, [0.3, 0.3], [1.0, 2.0])
    assert [x.shape for x in xs] == [(3, 2), (3, 2)] and [y.shape for y in ys] == [(3, 1), (3, 1)]
    assert ys[0][:, 0].tolist() == [0.0, 1.0, 2.0] and ys[1][:, 0].tolist() == [10.0, 11.0, 12.0]
    assert xs[0][:, 0].tolist() == [0.0, 1.0, 2.0] and xs[1][:, 0].tolist() == [1.0, 2.0, 3.0]
    assert cache["sweep_sets"] is entry and "trial_args" not in entry and entry["batch_size"] == 3
    assert not models[1].stale and models[0].stale                   # (the general path fits a larger model)
    # ... and back: None drops the trial step's arguments again and takes today's call
    entry["trial_args"] = "made by a trial step"
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache)
    assert stub.calls[-1] == ("cbo_acq_sweep_sets",) and "trial_args" not in entry and entry["batch_size"] is None
    assert len(stub.calls) == 3
    # variable costs: the later picks are rescaled from the batch cost to the point's own (pick 0 takes today's re-evaluation)
    var = {"X": lambda col: 1.0 + np.sum(np.abs(col)), "Z": lambda col: 2.0}
    grids1 = [_Grid(21)]

    class _EI:
        def __init__(self, *a):
            pass

        def sweep(self, x, cost, want_acq):
            return {"acq": np.array([[-5.0 / cost]])}
    from cbo_with_oop_amd.utils_functions import utils
    monkeypatch.setattr(utils, "CausalExpectedImprovement", _EI)
    xs, ys = find_next_y_points(models[:1], 0.3, [["X"]], var, "min", grids1, batch_size=3)
    batch_cost = 1.0 + np.sum(np.abs(grids1[0].points[:, :1]))
    assert stub.calls[-1][-1] == [batch_cost]
    assert ys[0][0, 0] == -5.0 / 1.0 and ys[0][1, 0] == 1.0 * batch_cost / 2.0 and ys[0][2, 0] == 2.0 * batch_cost / 3.0


def test_the_stale_flag_follows_the_librarys_routing_at_the_cap(monkeypatch):
    """A small model with a grid above the one launch's cap: a batch of one is cbo_acq_sweep_sets' route, which takes the set
    in its launch and does not fit it -- ``stale`` stays; from a batch of two on the general path fits it inside the call."""
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    assert _lib.SMALL_BATCH_MAX_CANDS == 1024
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    for batch, wide_is_fitted in ((1, False), (2, True), (64, True)):
        models = [_Model(11), _Model(12), _Model(13, small=False)]
        grids = [_Grid(21, 1025), _Grid(22, 1024), _Grid(23, 1025)]
        xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"], ["X"]], costs, "min", grids, batch_size=batch)
        assert stub.calls[-1][0] == "cbo_acq_sweep_sets_batch" and stub.calls[-1][4] == batch
        assert [x.shape for x in xs] == [(batch, 2)] * 3
        assert models[0].stale is (not wide_is_fitted), batch     # above the cap: fitted only by a batch of two or more
        assert models[1].stale is True                            # at the cap: the one launch, never fitted
        assert models[2].stale is False                           # a larger model: the general path, always


class _StubModel:
    def __init__(self):
        self.data = []

    def set_data(self, x, y):
        self.data.append((x.copy(), y.copy()))


def test_the_monitor_appends_a_batch_in_order_and_sums_its_cost():
    class Agent:
        task = "min"
        intervention_names = ["X", "Z"]
        constraints = []
        batch_size = 3

    agent = Agent()
    agent.data_x = [np.array([[1.0]]), np.array([[2.0]])]
    agent.data_y = [np.array([[0.5]]), np.array([[0.7]])]
    agent.models = [_StubModel(), _StubModel()]
    agent.target_functions = [lambda x: 10.0 * x, lambda x: x - 4.0]
    mon = cbo_module._Monitor(agent)
    xs = [np.zeros((3, 1)), np.array([[3.0], [1.0], [2.0]])]
    mon.log_agent_performance(["Z"], 1, xs, 6.5)
    assert agent.data_x[1].tolist() == [[2.0], [3.0], [1.0], [2.0]]
    assert agent.data_y[1].tolist() == [[0.7], [-1.0], [-3.0], [-2.0]]
    assert agent.data_x[0].tolist() == [[1.0]] and len(agent.models[1].data) == 1 and not agent.models[0].data
    assert agent.models[1].data[0][0].shape == (4, 1)
    assert mon.current_best_x["Z"][-3:] == [3.0, 1.0, 2.0] and mon.current_best_y["Z"][-3:] == [-1.0, -3.0, -2.0]
    assert mon.global_opt[-1] == -3.0 and mon.cumulative_cost == 6.5 and mon.current_cost[-1] == 6.5
    picked_set, picked_x = mon.chosen[-1]
    assert picked_set == ["Z"] and picked_x.shape == (3, 1) and picked_x[:, 0].tolist() == [3.0, 1.0, 2.0]
    # the trial's cost is the sum of the batch's interventions' costs
    agent.costs = {"Z": lambda v: 1.0 + abs(float(v))}
    assert cbo_module.CBO.compute_cost(agent, ["Z"], 1, xs) == (1 + 3.0) + (1 + 1.0) + (1 + 2.0)
    # batch_size=None: every recorded field is what it is today
    agent.batch_size = None
    mon.log_agent_performance(["X"], 0, [np.array([[4.0]]), None], 1.0)
    assert agent.data_x[0].tolist() == [[1.0], [4.0]] and mon.chosen[-1][1].shape == (1, 1)
    assert cbo_module.CBO.compute_cost(agent, ["Z"], 1, xs) == 1 + 3.0
