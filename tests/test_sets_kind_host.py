"""CPU tests of the point-wise acquisitions in the multi-set sweep and the agent: cbo_acq_sweep_sets_kind and
cbo_trial_step_kind are declared, exported and prototyped and refuse bad arguments without a device; the Python argument
checks fire before a device is touched; and acquisition="EI" leaves find_next_y_points on cbo_acq_sweep_sets.  The values are
checked on the GPU (tests/test_sets_kind_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import find_next_y_point, find_next_y_points
from cbo_with_oop_amd.utils_functions.utils import sets_acquisition, winners_to_points


class Untouchable:
    """Argument checks must not touch models, grids or cost tables."""

    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


def test_entry_points_are_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("cbo_acq_sweep_sets_kind", 10), ("cbo_trial_step_kind", 17)):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert decl, f"{name} not declared in include/cbo_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args
    # the EI forms with the kind in front of y_best and the parameter in the jitter's place
    sets, kind = _lib.SIGNATURES["cbo_acq_sweep_sets"][1], _lib.SIGNATURES["cbo_acq_sweep_sets_kind"][1]
    assert kind == sets[:3] + [ctypes.c_int] + sets[3:]
    step, kind = _lib.SIGNATURES["cbo_trial_step"][1], _lib.SIGNATURES["cbo_trial_step_kind"][1]
    assert kind == step[:9] + [ctypes.c_int] + step[9:]
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_the_library_refuses_bad_arguments_before_any_device_work():
    lib = _lib.load()
    one = np.ones(1)
    chosen = ctypes.c_int(-1)
    for kind in (0, 5, -1):
        assert lib.cbo_acq_sweep_sets_kind(1, None, None, kind, _lib.dptr(one), 0, 0.0, _lib.dptr(one), None,
                                           None) == _lib.CBO_ERR_INVALID
        assert b"kind" in lib.cbo_last_error()
        assert lib.cbo_trial_step_kind(1, None, None, -1, 0, None, None, None, None, kind, _lib.dptr(one), 0, 0.0,
                                       _lib.dptr(one), None, None, ctypes.byref(chosen)) == _lib.CBO_ERR_INVALID
        assert b"kind" in lib.cbo_last_error()
    for kind, y_best, task, param, cost, word in ((1, 0.0, 0, -1.0, 1.0, b"beta"), (1, 0.0, 0, np.nan, 1.0, b"param"),
                                                  (2, np.inf, 0, 0.0, 1.0, b"y_best"), (2, 0.0, 3, 0.0, 1.0, b"task"),
                                                  (4, 0.0, 0, np.inf, 1.0, b"param"), (3, 0.0, 0, 0.0, 0.0, b"cost"),
                                                  (4, 0.0, 0, 0.0, np.nan, b"cost")):
        yb, cs = np.array([y_best]), np.array([cost])
        assert lib.cbo_acq_sweep_sets_kind(1, None, None, kind, _lib.dptr(yb), task, param, _lib.dptr(cs), None,
                                           None) == _lib.CBO_ERR_INVALID
        assert word in lib.cbo_last_error(), (kind, lib.cbo_last_error())
    # valid scalars: the NULL handle arrays are what is refused
    for kind in (1, 2, 3, 4):
        assert lib.cbo_acq_sweep_sets_kind(1, None, None, kind, _lib.dptr(one), 0, 0.0, _lib.dptr(one), None,
                                           None) == _lib.CBO_ERR_INVALID
        assert lib.cbo_trial_step_kind(1, None, None, -1, 0, None, None, None, None, kind, _lib.dptr(one), 0, 0.0,
                                       _lib.dptr(one), None, None, ctypes.byref(chosen)) == _lib.CBO_ERR_INVALID
    assert chosen.value == -1


def test_sets_acquisition_names_defaults_and_refusals():
    assert sets_acquisition() == ("EI", None)
    assert sets_acquisition("LCB") == ("LCB", 1.0) and sets_acquisition("LCB", 0.0) == ("LCB", 0.0)
    assert sets_acquisition("LCB", np.array([[2.5]])) == ("LCB", 2.5)
    assert sets_acquisition("PI") == ("PI", 0.0) and sets_acquisition("PI", -0.25) == ("PI", -0.25)
    assert sets_acquisition("MPEI") == ("MPEI", 0.0) and sets_acquisition("MPEI", 0.01) == ("MPEI", 0.01)
    assert sets_acquisition("VAR") == ("VAR", 0.0)
    for name in ("UCB", "lcb", "MES", "", None, 1):
        with pytest.raises(ValueError, match="acquisition") as info:
            sets_acquisition(name)
        for known in ("EI", "LCB", "PI", "MPEI", "VAR"):
            assert repr(known) in str(info.value)
    for beta in (-1.0, -1e-300, np.nan, np.inf, -np.inf, "wide"):
        with pytest.raises(ValueError, match="beta"):
            sets_acquisition("LCB", beta)
    for name in ("PI", "MPEI"):
        for jitter in (np.nan, np.inf, -np.inf, "some", []):
            with pytest.raises(ValueError, match="jitter"):
                sets_acquisition(name, jitter)
    for name in ("EI", "VAR"):
        with pytest.raises(ValueError, match="acquisition_param"):
            sets_acquisition(name, 1.0)


def test_python_argument_checks_fire_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    params = inspect.signature(find_next_y_points).parameters
    assert list(params)[:8] == ["models", "current_global_best", "evaluated_sets", "costs_functions", "task", "grids",
                                "cache", "raw"]
    assert params["acquisition"].default == "EI" and params["acquisition_param"].default is None
    assert list(inspect.signature(find_next_y_point).parameters)[-1] == "constraints"       # (the per-set form is as it was)
    obj = Untouchable()
    bad = (("UCB", None, "acquisition"), (None, None, "acquisition"), ("LCB", -0.5, "beta"), ("LCB", np.nan, "beta"),
           ("PI", np.inf, "jitter"), ("MPEI", np.nan, "jitter"), ("EI", 0.1, "acquisition_param"),
           ("VAR", 0.1, "acquisition_param"))
    for name, param, word in bad:
        with pytest.raises(ValueError, match=word):
            find_next_y_points([obj], 0.0, [["X"]], obj, "min", [obj], acquisition=name, acquisition_param=param)
        with pytest.raises(ValueError, match=word):
            cbo_module.CBOAcquisitionPath(obj, [["X"]], obj, "min", [obj], [obj], [obj], comm=None, acquisition=name,
                                          acquisition_param=param)
    with pytest.raises(ValueError, match="task"):
        find_next_y_points([obj], 0.0, [["X"]], obj, "smallest", [obj], acquisition="LCB")
    # the path and the agent take and keep the two arguments; the defaults are today's
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        params = inspect.signature(cls.__init__).parameters
        assert params["acquisition"].default == "EI" and params["acquisition_param"].default is None
    path = cbo_module.CBOAcquisitionPath(obj, [["X"]], obj, "min", [obj], [obj], [obj], comm=None)
    assert (path.acquisition, path.acquisition_param) == ("EI", None)
    path = cbo_module.CBOAcquisitionPath(obj, [["X"]], obj, "max", [obj], [obj], [obj], comm=None, acquisition="PI",
                                         acquisition_param=0.02)
    assert (path.acquisition, path.acquisition_param) == ("PI", 0.02)


class _Handle:
    def __init__(self, value):
        self._handle = ctypes.c_void_p(value)
        self.small, self.stale = True, True
        self.index_offset = 0


class _StubLibrary:
    """Records the multi-set calls; every one of them reports set i's winner as (10 + i, i)."""

    def __init__(self):
        self.calls = []

    def _answer(self, s, vals, idxs):
        np.ctypeslib.as_array(vals, shape=(s,))[:] = 10.0 + np.arange(s)
        np.ctypeslib.as_array(idxs, shape=(s,))[:] = np.arange(s)
        return 0

    def cbo_acq_sweep_sets(self, s, gps, cds, y_best, task, jitter, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets", s, task, jitter))
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_kind(self, s, gps, cds, kind, y_best, task, param, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets_kind", s, kind, task, param))
        return self._answer(s, vals, idxs)


def test_ei_stays_on_cbo_acq_sweep_sets_and_the_cache_records_the_kind(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    models, grids = [_Handle(11), _Handle(12)], [_Handle(21), _Handle(22)]

    class Fixed:
        values = [1.0, 2.0]
    table, cache = Fixed(), {}
    _, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], table, "min", grids, cache=cache, raw=True)
    assert ys == [(10.0, 0), (11.0, 1)]
    assert stub.calls == [("cbo_acq_sweep_sets", 2, 0, 0.0)] and cache["sweep_sets"]["kind"] == ("EI", None)
    _, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], table, "max", grids, cache=cache, raw=True, acquisition="EI")
    assert stub.calls[-1] == ("cbo_acq_sweep_sets", 2, 1, 0.0) and len(stub.calls) == 2
    _, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], table, "min", grids, cache=cache, raw=True, acquisition="LCB",
                               acquisition_param=2.0)
    assert ys == [(10.0, 0), (11.0, 1)]
    assert stub.calls[-1] == ("cbo_acq_sweep_sets_kind", 2, _lib.ACQ_KIND_CODE["LCB"], 0, 2.0)
    assert cache["sweep_sets"]["kind"] == ("LCB", 2.0)
    for name, code, param in (("PI", 2, 0.0), ("VAR", 3, 0.0), ("MPEI", 4, 0.0)):
        find_next_y_points(models, 0.3, [["X"], ["Z"]], table, "max", grids, cache=cache, raw=True, acquisition=name)
        assert stub.calls[-1] == ("cbo_acq_sweep_sets_kind", 2, code, 1, param)
    assert len(stub.calls) == 6
    # a changed kind rebuilds nothing but the call: with a cache that can be matched (not raw) the entry is the same object
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    for g in grids:
        g.points = np.zeros((3, 1))
    cache = {}
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache)
    entry = cache["sweep_sets"]
    xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, acquisition="VAR")
    assert cache["sweep_sets"] is entry and entry["kind"] == ("VAR", 0.0)
    assert [y.tolist() for y in ys] == [[[10.0]], [[11.0]]] and [x.shape for x in xs] == [(1, 1), (1, 1)]
    assert [c[0] for c in stub.calls[-2:]] == ["cbo_acq_sweep_sets", "cbo_acq_sweep_sets_kind"]


def test_winners_are_reevaluated_through_the_kinds_class(monkeypatch):
    """A variable cost makes the point cost differ from the batch cost: the winner's value is then the kind's acquisition
    class's at the point's own cost, not the causal EI's."""
    from cbo_with_oop_amd.utils_functions import utils
    seen = []

    class Recorder:
        def __init__(self, label):
            self.label = label

        def sweep(self, x, cost, want_acq):
            seen.append((self.label, x.tolist(), cost, want_acq))
            return {"acq": np.array([[42.0]])}

    def recorder(name, model, best, task, space, param=None):
        return Recorder((name, param, best, task))
    monkeypatch.setattr(utils, "_acquisition_for", recorder)

    class Grid:
        index_offset = 100
        points = np.array([[0.5], [2.0], [3.0]])

    class VariableCost:
        def evaluate(self, x):
            return float(1.0 + np.sum(np.abs(x)))
    st = {"costs": [VariableCost()], "batch_cost": np.array([6.5]), "vals": np.array([7.0]), "idxs": np.array([101]),
          "kind": ("LCB", 2.0)}
    xs, ys = winners_to_points(st, [Untouchable()], [Grid()], 0.3, "max")
    assert xs[0].tolist() == [[2.0]] and ys[0].tolist() == [[42.0]]
    assert seen == [(("LCB", 2.0, 0.3, "max"), [[2.0]], 3.0, True)]
    # an entry from before the kind was recorded is the EI's; an equal cost re-evaluates nothing
    del st["kind"]
    winners_to_points(st, [Untouchable()], [Grid()], 0.3, "max")
    assert seen[-1][0] == ("EI", None, 0.3, "max")
    st["batch_cost"] = np.array([3.0])
    xs, ys = winners_to_points(st, [Untouchable()], [Grid()], 0.3, "max")
    assert ys[0].tolist() == [[7.0]] and len(seen) == 2
