"""CPU tests of the constrained acquisition in the multi-set sweep and the agent:
cbo_acq_sweep_sets_constrained is declared, exported and prototyped and refuses bad scalars and arrays without a device;
the Python argument checks fire before a device is touched; constraints=None leaves find_next_y_points on today's calls; and
the agent refuses a constrained target and a constrained manipulated node.  The values are checked on the GPU
(tests/test_sets_constrained_gpu.py)."""
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
    """Argument checks must not touch models, grids or cost tables."""

    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


def test_the_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+cbo_acq_sweep_sets_constrained\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, "cbo_acq_sweep_sets_constrained not declared in include/cbo_hip.h"
    assert len(decl.group(1).split(",")) == 15
    assert hasattr(_lib.load(), "cbo_acq_sweep_sets_constrained"), "not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_sets_constrained"]
    assert restype is ctypes.c_int and len(argtypes) == 15
    # cbo_acq_sweep_sets' arguments with the six constraint arrays in front of the outputs
    sets = _lib.SIGNATURES["cbo_acq_sweep_sets"][1]
    assert argtypes == sets[:7] + [_lib.c_int_p, _lib.c_void_pp, _lib.c_void_pp, _lib.c_double_p, _lib.c_double_p,
                                   _lib.c_int_p] + sets[7:]
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_the_library_refuses_bad_scalars_and_arrays_with_null_handle_arrays():
    lib = _lib.load()
    vals, idxs = np.full(2, -7.0), np.full(2, -7, dtype=np.int64)

    def call(n_sets=2, y_best=(0.1, 0.2), task=0, costs=(1.0, 2.0), n_con=(1, 2), value=(0.0, 0.1, 0.2),
             jitter=(0.0, 0.0, 0.01), sense=(0, 1, 0), outputs=True):
        arr = lambda a: None if a is None else _lib.dptr(np.array(a, dtype=np.float64))                          # noqa: E731
        ints = lambda a: None if a is None else np.array(a, dtype=np.int32).ctypes.data_as(_lib.c_int_p)        # noqa: E731
        return lib.cbo_acq_sweep_sets_constrained(n_sets, None, None, arr(y_best), task, 0.0, arr(costs), ints(n_con), None,
                                                  None, arr(value), arr(jitter), ints(sense),
                                                  _lib.dptr(vals) if outputs else None,
                                                  idxs.ctypes.data_as(_lib.c_int64_p) if outputs else None)

    bad = ((dict(n_sets=0), b"n_sets"), (dict(n_sets=-3), b"n_sets"), (dict(y_best=None), b"y_best"),
           (dict(costs=None), b"costs"), (dict(n_con=None), b"n_con"), (dict(outputs=False), b"best_vals"),
           (dict(task=2), b"task"), (dict(task=-1), b"task"),
           (dict(costs=(1.0, 0.0)), b"cost"), (dict(costs=(-1.0, 1.0)), b"cost"), (dict(costs=(1.0, np.nan)), b"cost"),
           (dict(n_con=(9, 0)), b"n_con"), (dict(n_con=(0, -1)), b"n_con"),
           (dict(value=None), b"con_value"), (dict(jitter=None), b"con_jitter"), (dict(sense=None), b"con_sense"),
           (dict(value=(0.0, np.nan, 0.2)), b"con_value"), (dict(value=(np.inf, 0.0, 0.2)), b"con_value"),
           (dict(jitter=(0.0, 0.0, -np.inf)), b"con_jitter"), (dict(jitter=(np.nan, 0.0, 0.0)), b"con_jitter"),
           (dict(sense=(0, 2, 0)), b"con_sense"), (dict(sense=(0, 1, -1)), b"con_sense"))
    for kw, word in bad:
        assert call(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    # valid scalars: the NULL handle arrays are what is refused -- also without any constraint, where the five constraint
    # arrays may be NULL
    assert call() == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert call(n_con=(0, 0), value=None, jitter=None, sense=None) == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert np.all(vals == -7.0) and np.all(idxs == -7)


def test_python_argument_checks_fire_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    params = inspect.signature(find_next_y_points).parameters
    assert list(params)[-1] == "constraints" and params["constraints"].default is None
    obj = Untouchable()
    pof = lambda **kw: ProbabilityOfFeasibility(obj, **kw)                                                    # noqa: E731
    sweep = lambda constraints, **kw: find_next_y_points([obj, obj], 0.0, [["X"], ["Z"]], obj, "min", [obj, obj],  # noqa: E731
                                                         constraints=constraints, **kw)
    with pytest.raises(ValueError, match="one entry per exploration set"):
        sweep([[pof()]])
    with pytest.raises(ValueError, match="one entry per exploration set"):
        sweep([[pof()], [], []])
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        sweep([[pof()], []], acquisition="LCB")
    with pytest.raises(ValueError, match="at most 8"):
        sweep([[], [pof() for _ in range(9)]])
    for kw in (dict(max_value=np.nan), dict(max_value=np.inf), dict(jitter=-np.inf), dict(jitter=np.nan), dict(jitter="some")):
        with pytest.raises(ValueError, match="max_value|jitter"):
            sweep([[pof(**kw)], []])
    with pytest.raises(ValueError, match="ProbabilityOfFeasibility"):
        sweep([[obj], []])
    with pytest.raises(ValueError, match="raw"):
        sweep([[pof()], []], raw=True)
    # the path: a list of (name, sense, value[, jitter]), at most 8, EI only
    path = lambda constraints, data=None, **kw: cbo_module.CBOAcquisitionPath(                                # noqa: E731
        obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], [obj, obj], comm=None, constraints=constraints,
        constraint_data_y=data, **kw)
    col = np.zeros((3, 1))
    for constraints, word in (([("C", "<", 0.0)], "sense"), ([("C", "<=", np.nan)], "finite"), ([("C", ">=", 0.0, np.inf)], "finite"),
                              ([("C", "<=")], "name, sense, value"), ([("C", "<=", 0.0)] * 9, "at most 8")):
        with pytest.raises(ValueError, match=word):
            path(constraints, [[col] * len(constraints)] * 2)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        path([("C", "<=", 0.0)], [[col], [col]], acquisition="PI")
    with pytest.raises(ValueError, match="constraint_data_y"):
        path([("C", "<=", 0.0)])
    with pytest.raises(ValueError, match="constraint_data_y"):
        path([("C", "<=", 0.0)], [[col]])
    with pytest.raises(ValueError, match="constraint_data_y"):
        path([("C", "<=", 0.0)], [[col], [col, col]])
    kept = path([("C", "<=", 0.5), ("A", ">=", -1.0, 0.01)], [[col, col], [col, col]])
    assert kept.constraints == [("C", "<=", 0.5, 0.0), ("A", ">=", -1.0, 0.01)] and kept.constraint_models == []
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        assert inspect.signature(cls.__init__).parameters["constraints"].default is None
    assert path(None).constraints == [] and path(None).set_constraints() is None


class _Handle:
    def __init__(self, value):
        self._handle = ctypes.c_void_p(value)
        self.small, self.stale = True, True
        self.index_offset = 0
        self.points = np.zeros((3, 1))


class _StubLibrary:
    """Records the multi-set calls; every one of them reports set i's winner as (10 + i, i)."""

    def __init__(self):
        self.calls = []

    def _answer(self, s, vals, idxs):
        np.ctypeslib.as_array(vals, shape=(s,))[:] = 10.0 + np.arange(s)
        np.ctypeslib.as_array(idxs, shape=(s,))[:] = np.arange(s)
        return 0

    def cbo_acq_sweep_sets(self, s, gps, cds, y_best, task, jitter, costs, vals, idxs):
        self.calls.append("cbo_acq_sweep_sets")
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_kind(self, s, gps, cds, kind, y_best, task, param, costs, vals, idxs):
        self.calls.append("cbo_acq_sweep_sets_kind")
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_constrained(self, *args):
        raise AssertionError("no constraint was given: the constrained call must not be taken")


def test_no_constraints_stay_on_todays_calls(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    models, grids = [_Handle(11), _Handle(12)], [_Handle(21), _Handle(22)]
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    cache = {}
    for constraints in (None, [[], []], [None, []]):
        xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, constraints=constraints)
        assert [y.tolist() for y in ys] == [[[10.0]], [[11.0]]] and stub.calls[-1] == "cbo_acq_sweep_sets"
        assert cache["sweep_sets"]["constraints"] is None and "con_grids" not in cache["sweep_sets"]
        find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, acquisition="LCB",
                           constraints=constraints)
        assert stub.calls[-1] == "cbo_acq_sweep_sets_kind"
    assert len(stub.calls) == 6


def test_the_agent_refuses_a_constrained_target_and_a_constrained_manipulated_node():
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda constraints: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data,  # noqa: E731
                                              constraints=constraints)
    with pytest.raises(ValueError, match="target"):
        make({"Y": ("<=", 0.0)})
    for node in ("B", "D", "E"):
        with pytest.raises(ValueError, match="manipulates"):
            make({"C": ("<=", 1.0), node: (">=", 0.0)})
    with pytest.raises(ValueError, match="sense"):
        make({"C": ("==", 1.0)})
    with pytest.raises(ValueError, match="finite"):
        make({"C": ("<=", np.inf)})
