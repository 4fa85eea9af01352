"""CPU tests of max-value entropy search in the multi-set sweep and the agent: cbo_acq_sweep_sets_mes and
cbo_gp_mes_gumbel_sets are declared, exported and prototyped and refuse bad scalars without a device; sets_acquisition accepts
"MES" in its documented forms and refuses the others; the Python argument checks fire before a device is touched; and
mes_sets_parameters draws from numpy's global generator in its documented order.  The values are checked on the GPU
(tests/test_sets_mes_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import find_next_y_points
from cbo_with_oop_amd.utils_functions import max_value_entropy as mve
from cbo_with_oop_amd.utils_functions.utils import sets_acquisition, sets_acquisition_or_default


class Untouchable:
    """Argument checks must not touch grids or cost tables."""

    def __getattr__(self, name):
        raise AssertionError(f"the object was asked for {name!r}")


class _Model:
    def __init__(self, X, handle, small=True, causal=False):
        self.X = np.asarray(X, dtype=np.float64)
        self._handle = ctypes.c_void_p(handle)
        self.small, self.stale, self.causal = small, True, causal


def test_the_entry_points_are_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("cbo_acq_sweep_sets_mes", 8), ("cbo_gp_mes_gumbel_sets", 6)):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert decl, f"{name} not declared in include/cbo_hip.h"
        assert len(decl.group(1).split(",")) == arity
        assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == arity
    sets = _lib.SIGNATURES["cbo_acq_sweep_sets"][1]
    # cbo_acq_sweep_sets' handle arrays, the sample counts and pointers, then its costs and outputs
    assert _lib.SIGNATURES["cbo_acq_sweep_sets_mes"][1] == sets[:3] + [_lib.c_int_p, _lib.c_void_pp] + sets[6:]
    assert _lib.SIGNATURES["cbo_gp_mes_gumbel_sets"][1] == sets[:3] + [_lib.c_double_p] * 3
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_the_library_refuses_bad_scalars_with_null_handle_arrays():
    lib = _lib.load()
    vals, idxs = np.full(2, -7.0), np.full(2, -7, dtype=np.int64)
    good = (np.array([-1.0, 0.5]), np.array([0.25]))

    def call(n_sets=2, counts=(2, 1), mins=good, costs=(1.0, 2.0), outputs=True):
        cnt = None if counts is None else (ctypes.c_int * len(counts))(*counts)
        ptrs = None if mins is None else (ctypes.c_void_p * len(mins))(*[None if r is None else r.ctypes.data for r in mins])
        cs = None if costs is None else _lib.dptr(np.array(costs, dtype=np.float64))
        return lib.cbo_acq_sweep_sets_mes(n_sets, None, None, cnt, ptrs, cs, _lib.dptr(vals) if outputs else None,
                                          idxs.ctypes.data_as(_lib.c_int64_p) if outputs else None)

    big = np.zeros(70)
    bad = ((dict(n_sets=0), b"n_sets"), (dict(n_sets=-3), b"n_sets"), (dict(counts=None), b"n_samples"),
           (dict(mins=None), b"mins"), (dict(costs=None), b"costs"), (dict(outputs=False), b"best_vals"),
           (dict(counts=(0, 1), mins=(big, big)), b"samples"), (dict(counts=(2, -1), mins=(big, big)), b"samples"),
           (dict(counts=(2, 65), mins=(big, big)), b"samples"), (dict(mins=(good[0], None)), b"mins"),
           (dict(mins=(np.array([0.1, np.nan]), good[1])), b"finite"), (dict(mins=(good[0], np.array([np.inf]))), b"finite"),
           (dict(costs=(1.0, 0.0)), b"cost"), (dict(costs=(-1.0, 1.0)), b"cost"), (dict(costs=(1.0, np.nan)), b"cost"))
    for kw, word in bad:
        assert call(**kw) == _lib.CBO_ERR_INVALID, kw
        assert word in lib.cbo_last_error(), (kw, lib.cbo_last_error())
    # valid scalars (the cap of 64 samples included): the NULL handle arrays are what is refused
    assert call() == _lib.CBO_ERR_INVALID
    assert call(counts=(64, 1), mins=(big, good[1])) == _lib.CBO_ERR_INVALID and b"samples" not in lib.cbo_last_error()
    assert np.all(vals == -7.0) and np.all(idxs == -7)
    q, a, b = np.full((2, 3), -7.0), np.full(2, -7.0), np.full(2, -7.0)
    for n_sets in (0, -1, 2):
        assert lib.cbo_gp_mes_gumbel_sets(n_sets, None, None, _lib.dptr(q), _lib.dptr(a), _lib.dptr(b)) == _lib.CBO_ERR_INVALID
    assert np.all(q == -7.0) and np.all(a == -7.0) and np.all(b == -7.0)


def test_sets_acquisition_accepts_mes():
    # emukit's defaults (10 samples, grid 5000) for a None: filled by what the public callers call; the bare helper, which
    # has always refused the name alone, has no default for it
    assert sets_acquisition_or_default("MES") == ("MES", (10, 5000))
    assert sets_acquisition_or_default("MES", None) == ("MES", (10, 5000))
    assert sets_acquisition_or_default("MES", (7, 37)) == ("MES", (7, 37))
    assert sets_acquisition_or_default("LCB") == ("LCB", 1.0) and sets_acquisition_or_default() == ("EI", None)
    with pytest.raises(ValueError, match="'MES' with acquisition_param"):
        sets_acquisition("MES")
    assert sets_acquisition("MES", (7, 37)) == ("MES", (7, 37))
    assert sets_acquisition("MES", [1, 1]) == ("MES", (1, 1))
    assert sets_acquisition("MES", (np.int64(64), np.int32(5))) == ("MES", (64, 5))
    answer = sets_acquisition("MES", (7, 37))
    assert sets_acquisition(answer) is answer                             # an earlier answer in the place of the name
    for bad in ((0, 10), (65, 10), (-1, 10), (10, 0), (10, -5)):
        with pytest.raises(ValueError, match="num_samples|grid_size"):
            sets_acquisition("MES", bad)
        with pytest.raises(ValueError):
            sets_acquisition(("MES", bad))
    for bad in ((10.0, 100), (10, 100.0), ("10", 100), (True, 100), (10, False), 10, (10,), (10, 100, 1), "10,100", 3.5,
                (None, 100), np.array([10.5, 100.0])):
        with pytest.raises(ValueError, match="pair of ints"):
            sets_acquisition("MES", bad)
    # the other kinds are as they were
    assert sets_acquisition("EI") == ("EI", None) and sets_acquisition("LCB") == ("LCB", 1.0)
    with pytest.raises(ValueError, match="'MES'"):
        sets_acquisition("mes")


def test_python_argument_checks_fire_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    obj = Untouchable()
    models = [_Model(np.zeros((3, 1)), 11), _Model(np.zeros((4, 1)), 12)]
    spaces = [[(-1.0, 1.0)], [(0.0, 2.0)]]
    sweep = lambda task="min", **kw: find_next_y_points(models, 0.0, [["X"], ["Z"]], obj, task, [obj, obj],      # noqa: E731
                                                        acquisition="MES", **kw)
    with pytest.raises(ValueError, match="task must be 'min'"):
        sweep(task="max", spaces=spaces)
    with pytest.raises(ValueError, match="task must be 'min'"):
        sweep(task="sideways", spaces=spaces)
    with pytest.raises(ValueError, match="spaces"):
        sweep()
    with pytest.raises(ValueError, match="spaces"):
        sweep(spaces=spaces[:1])
    with pytest.raises(ValueError, match="raw=True"):
        sweep(spaces=spaces, raw=True)
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        sweep(spaces=spaces, constraints=[[obj], []])
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        sweep(spaces=spaces, hyper_samples=[np.ones((1, 3)), np.ones((1, 3))])
    with pytest.raises(ValueError, match="acquisition must be 'EI'"):
        sweep(spaces=spaces, hyper_samples=3)
    for bad in ((0, 10), (65, 10), (10, 0), (2.5, 10), 7):
        with pytest.raises(ValueError):
            sweep(spaces=spaces, acquisition_param=bad)
    # empty constraint lists and hyper_samples=None are nothing: the call goes on to the device (and is stopped there)
    with pytest.raises(AssertionError, match="device library was reached|was asked for"):
        sweep(spaces=spaces, constraints=[[], []], hyper_samples=None)
    # the path and the agent refuse task 'max' at construction
    from cbo_with_oop_amd.CBO import CBOAcquisitionPath
    with pytest.raises(ValueError, match="task must be 'min'"):
        CBOAcquisitionPath(None, [["X"], ["Z"]], obj, "max", [None, None], [None, None], spaces, comm=None, acquisition="MES")
    with pytest.raises(ValueError, match="num_samples"):
        CBOAcquisitionPath(None, [["X"], ["Z"]], obj, "min", [None, None], [None, None], spaces, comm=None, acquisition="MES",
                           acquisition_param=(65, 10))
    path = CBOAcquisitionPath(None, [["X"], ["Z"]], obj, "min", [None, None], [None, None], spaces, comm=None,
                              acquisition="MES", acquisition_param=(5, 20))
    assert path._kind == ("MES", (5, 20)) and path.space_list is spaces
    path = CBOAcquisitionPath(None, [["X"], ["Z"]], obj, "min", [None, None], [None, None], spaces, comm=None,
                              acquisition="MES")
    assert path._kind == ("MES", (10, 5000)) and path.acquisition_param is None          # emukit's defaults


def test_mes_sets_parameters_draws_in_the_documented_order(monkeypatch):
    """gumbel_grid for the sets in order, ONE cbo_gp_mes_gumbel_sets call, gumbel_mins for the sets in order -- against a
    stubbed library that returns fixed a, b and records what it was handed."""
    events, closed = [], []
    fixed_a, fixed_b = np.array([-1.5, 0.25, 3.0]), np.array([0.5, 2.0, 0.125])

    class Grid:
        def __init__(self, points, model):
            events.append(("grid", model._handle.value, np.array(points)))
            self._handle = ctypes.c_void_p(100 + model._handle.value)

        def close(self):
            closed.append(self._handle.value)

    class Lib:
        def cbo_gp_mes_gumbel_sets(self, s, gps, cds, q, a, b):
            events.append(("call", s, [gps[i] for i in range(s)], [cds[i] for i in range(s)], np.random.get_state()[2]))
            for i in range(s):
                a[i], b[i] = fixed_a[i], fixed_b[i]
                q[3 * i], q[3 * i + 1], q[3 * i + 2] = i + 0.25, i + 0.5, i + 0.75
            return 0

    monkeypatch.setattr(mve, "CandidateGrid", Grid)
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    models = [_Model([[0.1], [0.2]], 1), _Model([[1.0, 2.0]], 2, small=False), _Model([[5.0], [6.0], [7.0]], 3)]
    spaces = [[(-1.0, 1.0)], [(0.0, 2.0), (3.0, 4.0)], [(-5.0, 5.0)]]
    np.random.seed(77)
    gumbels, mins = mve.mes_sets_parameters(models, spaces, num_samples=4, grid_size=6)
    # by hand, from the same seed
    np.random.seed(77)
    want_grids = [mve.gumbel_grid(spaces[i], 6, models[i].X) for i in range(3)]
    want_mins = [mve.gumbel_mins(4, fixed_a[i], fixed_b[i]) for i in range(3)]
    assert [e[0] for e in events] == ["grid", "grid", "grid", "call"]
    for i in range(3):
        assert events[i][1] == i + 1 and np.array_equal(events[i][2], want_grids[i])
        assert np.array_equal(events[i][2][:len(models[i].X)], models[i].X)       # the model's inputs on top
        assert np.array_equal(mins[i], want_mins[i]) and mins[i].shape == (4,)
        assert gumbels[i] == (i + 0.25, i + 0.5, i + 0.75, fixed_a[i], fixed_b[i])
    assert events[3][1:4] == (3, [1, 2, 3], [101, 102, 103])
    assert sorted(closed) == [101, 102, 103]                                        # built per call, closed afterwards
    assert models[1].stale is False and models[0].stale and models[2].stale        # the general path fitted the larger one
    # the other interleaving (per-set update_parameters: grid, minima, grid, minima) gives other numbers
    np.random.seed(77)
    other = []
    for i in range(3):
        mve.gumbel_grid(spaces[i], 6, models[i].X)
        other.append(mve.gumbel_mins(4, fixed_a[i], fixed_b[i]))
    assert not np.array_equal(other[1], mins[1])
    # refusals before anything is drawn or built
    state = np.random.get_state()[1].copy()
    n_events = len(events)
    for kw in (dict(num_samples=0), dict(num_samples=65), dict(grid_size=0)):
        with pytest.raises(ValueError):
            mve.mes_sets_parameters(models, spaces, **kw)
    with pytest.raises(ValueError):
        mve.mes_sets_parameters(models, spaces[:2])
    assert np.array_equal(np.random.get_state()[1], state) and len(events) == n_events
