"""CPU tests of the hyper-parameter-marginalised EI in the multi-set sweep and the agent:
cbo_acq_sweep_sets_hyper is declared, exported and prototyped and refuses bad scalars and arrays without a device; the Python
argument checks fire before a device is touched; hyper_samples=None leaves find_next_y_points on today's calls, and a list of
rows takes the one new call with the rows it was given.  The values are checked on the GPU (tests/test_sets_hyper_gpu.py)."""
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
    """What the row check reads of a model: its lengthscales and whether its noise is fixed."""

    def __init__(self, n_ls=1, fix_noise=False, noise_var=1e-2, handle=11):
        self.lengthscale = np.ones(n_ls)
        self.fix_noise, self.noise_var = fix_noise, noise_var
        self._handle = ctypes.c_void_p(handle)
        self.small, self.stale = True, True

    def generate_hyperparameters_samples(self, *a, **k):
        raise AssertionError("the sampler was reached")


def test_the_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+cbo_acq_sweep_sets_hyper\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, "cbo_acq_sweep_sets_hyper not declared in include/cbo_hip.h"
    assert len(decl.group(1).split(",")) == 11
    assert hasattr(_lib.load(), "cbo_acq_sweep_sets_hyper"), "not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_sets_hyper"]
    assert restype is ctypes.c_int and len(argtypes) == 11
    # cbo_acq_sweep_sets' arguments with the sample counts and the row pointers behind the handle arrays
    sets = _lib.SIGNATURES["cbo_acq_sweep_sets"][1]
    assert argtypes == sets[:3] + [_lib.c_int_p, _lib.c_void_pp] + sets[3:]
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_the_library_refuses_bad_scalars_and_arrays_with_null_handle_arrays():
    lib = _lib.load()
    vals, idxs = np.full(2, -7.0), np.full(2, -7, dtype=np.int64)
    good = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 0.0]])

    def call(n_sets=2, counts=(2, 1), rows=(good, good), y_best=(0.1, 0.2), task=0, costs=(1.0, 2.0), outputs=True):
        arr = lambda a: None if a is None else _lib.dptr(np.array(a, dtype=np.float64))                          # noqa: E731
        cnt = None if counts is None else (ctypes.c_int * len(counts))(*counts)
        ptrs = None if rows is None else (ctypes.c_void_p * len(rows))(*[None if r is None else r.ctypes.data for r in rows])
        return lib.cbo_acq_sweep_sets_hyper(n_sets, None, None, cnt, ptrs, arr(y_best), task, 0.0, arr(costs),
                                            _lib.dptr(vals) if outputs else None,
                                            idxs.ctypes.data_as(_lib.c_int64_p) if outputs else None)

    bad = ((dict(n_sets=0), b"n_sets"), (dict(n_sets=-3), b"n_sets"), (dict(counts=None), b"n_samples"),
           (dict(rows=None), b"hyper"), (dict(y_best=None), b"y_best"), (dict(costs=None), b"costs"),
           (dict(outputs=False), b"best_vals"), (dict(task=2), b"task"), (dict(task=-1), b"task"),
           (dict(counts=(0, 1)), b"samples"), (dict(counts=(2, -1)), b"samples"), (dict(counts=(2, 257)), b"samples"),
           (dict(rows=(good, None)), b"hyper"), (dict(rows=(None, good)), b"hyper"),
           (dict(costs=(1.0, 0.0)), b"cost"), (dict(costs=(-1.0, 1.0)), b"cost"), (dict(costs=(1.0, np.nan)), b"cost"))
    for kw, word in bad:
        assert call(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    # valid scalars: the NULL handle arrays are what is refused (the rows' values wait for the models that size them)
    assert call() == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert call(counts=(2, 256)) == _lib.CBO_ERR_INVALID and b"gps" in lib.cbo_last_error()
    assert np.all(vals == -7.0) and np.all(idxs == -7)


def test_python_argument_checks_fire_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    params = inspect.signature(find_next_y_points).parameters
    assert params["hyper_samples"].default is None and list(params)[-1] == "constraints"
    obj = Untouchable()
    models = [_Model(1), _Model(3)]
    rows = [np.array([[1.0, 1.0, 1e-2]]), np.array([[1.0, 1.0, 2.0, 3.0, 1e-2], [2.0, 1.0, 2.0, 3.0, 0.0]])]
    sweep = lambda hyper, **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, "min", [obj, obj],      # noqa: E731
                                                   hyper_samples=hyper, **kw)
    with pytest.raises(ValueError, match="one entry per exploration set"):
        sweep(rows[:1])
    with pytest.raises(ValueError, match="one entry per exploration set"):
        sweep(rows + rows[:1])
    with pytest.raises(ValueError, match="a list with one"):
        sweep(rows[0])                                               # one array is not a list of arrays
    for bad in (0, -2, True):
        with pytest.raises(ValueError, match="positive int"):
            sweep(bad)
    with pytest.raises(ValueError, match="at most 256"):
        sweep(257)
    with pytest.raises(ValueError, match="columns"):
        sweep([rows[0], rows[1][:, :4]])                             # a bad shape: 4 columns for three lengthscales
    with pytest.raises(ValueError, match="columns"):
        sweep([rows[0][:, :2], rows[1]])                             # no noise column, and the noise is not fixed
    with pytest.raises(ValueError, match="set 1"):
        sweep([rows[0], np.zeros((2, 5, 1))])
    with pytest.raises(ValueError, match="at most 256"):
        sweep([np.tile(rows[0], (257, 1)), rows[1]])
    for r, c, bad in ((0, 0, 0.0), (0, 1, -1.0), (1, 3, np.nan), (0, 0, np.inf), (1, 4, -1e-12), (1, 4, np.nan)):
        broken = rows[1].copy()
        broken[r, c] = bad
        with pytest.raises(ValueError, match="set 1.*finite"):
            sweep([rows[0], broken])
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        sweep(rows, acquisition="LCB")
    with pytest.raises(ValueError, match="constraints"):
        sweep(rows, constraints=[[ProbabilityOfFeasibility(obj)], []])
    with pytest.raises(ValueError, match="raw"):
        sweep(rows, raw=True)
    # a fixed noise fills its own column: (H, 1 + L) rows pass the check (and then reach for the device)
    fixed = [_Model(1, fix_noise=True), _Model(3)]
    with pytest.raises(AssertionError, match="device library"):
        find_next_y_points(fixed, 0.0, [["X"], ["Z"]], {"X": lambda col: 1.0, "Z": lambda col: 1.0}, "min",
                           [_Grid(21), _Grid(22)], hyper_samples=[rows[0][:, :2], rows[1]])
    # the path and the agent: a positive int or a callable, EI only, no constraints
    path = lambda hyper, **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj],   # noqa: E731
                                                             [obj, obj], comm=None, hyper_samples=hyper, **kw)
    for bad in (0, -1, True, 257, 2.5, "ten", [rows[0]]):
        with pytest.raises(ValueError, match="hyper_samples"):
            path(bad)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        path(3, acquisition="PI")
    col = np.zeros((3, 1))
    with pytest.raises(ValueError, match="constraints"):
        path(3, constraints=[("C", "<=", 0.0)], constraint_data_y=[[col], [col]])
    sampler = lambda model, s: rows[s]                                                                         # noqa: E731
    kept = path(sampler)
    assert kept.hyper_samples is sampler and kept.hyper_rows == [None, None]
    assert path(4).hyper_samples == 4 and path(None).hyper_samples is None
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        assert inspect.signature(cls.__init__).parameters["hyper_samples"].default is None


def test_the_agent_refuses_bad_hyper_samples_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data, **kw)  # noqa: E731
    for bad in (0, True, 257, "ten"):
        with pytest.raises(ValueError, match="hyper_samples"):
            make(hyper_samples=bad)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        make(hyper_samples=5, acquisition="LCB")
    with pytest.raises(ValueError, match="constraints"):
        make(hyper_samples=5, constraints={"C": ("<=", 1.0)})
    agent = make(hyper_samples=5)
    assert agent.hyper_samples == 5 and agent.hyper_rows == [None] * len(es)


class _Grid:
    def __init__(self, value):
        self._handle = ctypes.c_void_p(value)
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
        self.calls.append(("cbo_acq_sweep_sets",))
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_kind(self, s, gps, cds, kind, y_best, task, param, costs, vals, idxs):
        self.calls.append(("cbo_acq_sweep_sets_kind",))
        return self._answer(s, vals, idxs)

    def cbo_acq_sweep_sets_hyper(self, s, gps, cds, counts, ptrs, y_best, task, jitter, costs, vals, idxs):
        rows = []
        for i in range(s):
            width = {11: 3, 12: 5}[gps[i]]
            flat = np.ctypeslib.as_array(ctypes.cast(ptrs[i], _lib.c_double_p), shape=(counts[i] * width,))
            rows.append(flat.reshape(counts[i], width).copy())
        self.calls.append(("cbo_acq_sweep_sets_hyper", task, jitter, rows))
        return self._answer(s, vals, idxs)


def test_none_stays_on_todays_calls_and_rows_take_the_one_new_call(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    models, grids = [_Model(1, fix_noise=True, noise_var=0.25, handle=11), _Model(3, handle=12)], [_Grid(21), _Grid(22)]
    models[1].small = False
    costs = {"X": lambda col: 1.0, "Z": lambda col: 2.0}
    cache = {}
    xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, hyper_samples=None)
    assert [y.tolist() for y in ys] == [[[10.0]], [[11.0]]] and stub.calls == [("cbo_acq_sweep_sets",)]
    entry = cache["sweep_sets"]
    assert entry["hyper_rows"] is None and "hyper_args" not in entry
    assert not models[1].stale                                      # (the general path of today's call fits a larger model)
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache, acquisition="LCB")
    assert stub.calls[-1] == ("cbo_acq_sweep_sets_kind",)
    # rows: the one new call, with the rows as given -- the fixed noise filling its own column -- on the same cache entry
    given = [np.array([[1.5, 0.7], [0.5, 2.0]]), np.array([[1.0, 1.0, 2.0, 3.0, 1e-2]])]
    models[1].stale = True
    entry["trial_args"] = "made by a trial step"
    xs, ys = find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "max", grids, cache=cache, hyper_samples=given)
    name, task, jitter, rows = stub.calls[-1]
    assert (name, task, jitter) == ("cbo_acq_sweep_sets_hyper", 1, 0.0)
    assert np.array_equal(rows[0], [[1.5, 0.7, 0.25], [0.5, 2.0, 0.25]]) and np.array_equal(rows[1], given[1])
    assert [y.tolist() for y in ys] == [[[10.0]], [[11.0]]] and [x.shape for x in xs] == [(1, 1), (1, 1)]
    assert cache["sweep_sets"] is entry and "trial_args" not in entry
    assert [r.tolist() for r in entry["hyper_rows"]] == [r.tolist() for r in rows]
    assert models[1].stale                                          # (the marginalised general path restores: not marked fitted)
    # ... and back: None drops the trial step's arguments again and takes today's call
    entry["trial_args"] = "made by a trial step"
    find_next_y_points(models, 0.3, [["X"], ["Z"]], costs, "min", grids, cache=cache)
    assert stub.calls[-1] == ("cbo_acq_sweep_sets",) and "trial_args" not in entry and entry["hyper_rows"] is None
    assert len(stub.calls) == 4
