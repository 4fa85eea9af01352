"""CPU tests of max-value entropy search: cbo_gp_mes_gumbel and cbo_acq_sweep_mes are declared, exported and prototyped,
MaxValueEntropySearch carries emukit's signature and defaults, its random draws consume numpy's global stream as emukit's
update_parameters does, and find_next_y_point(acquisition="MES") refuses what emukit's MES cannot do.  The values are
checked on the GPU (tests/test_mes_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import (AcquisitionQuotient, CausalGradientAcquisitionOptimizer, Cost,
                                              MaxValueEntropySearch, find_next_y_point)
from cbo_with_oop_amd.utils_functions.max_value_entropy import gumbel_grid, gumbel_mins


class StubModel:
    """Construction must not touch the model (emukit's __init__ only stores it)."""
    causal = False
    X = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])


@pytest.mark.parametrize("name,nargs", [("cbo_gp_mes_gumbel", 10), ("cbo_acq_sweep_mes", 10)])
def test_entry_points_are_declared_exported_and_prototyped(name, nargs):
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/cbo_hip.h"
    assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == nargs
    assert _lib.ABI_VERSION == 5


def test_sweep_prototype_types():
    argtypes = _lib.SIGNATURES["cbo_acq_sweep_mes"][1]
    assert argtypes[2] is ctypes.c_int                 # number of samples
    assert argtypes[4] is ctypes.c_double              # cost
    assert argtypes[9] is _lib.c_int64_p               # best_idx
    assert _lib.SIGNATURES["cbo_gp_mes_gumbel"][1][1] is ctypes.c_int64


def test_class_has_emukits_signature_and_defaults():
    params = inspect.signature(MaxValueEntropySearch.__init__).parameters
    assert list(params) == ["self", "model", "space", "num_samples", "grid_size"]
    assert params["num_samples"].default == 10 and params["grid_size"].default == 5000
    mes = MaxValueEntropySearch(StubModel(), [(0.0, 1.0), (0.0, 1.0)])
    assert mes.mins is None and mes.num_samples == 10 and mes.grid_size == 5000
    params = inspect.signature(MaxValueEntropySearch.sweep).parameters
    assert list(params) == ["self", "candidates", "cost", "want_acq", "want_posterior"]
    assert params["cost"].default == 1.0 and params["want_acq"].default is False
    assert params["want_posterior"].default is False


@pytest.mark.parametrize("bounds,grid_size,k", [([(-5.0, 5.0)], 7, 10), ([(-1.0, 2.0), (0.0, 10.0), (3.0, 4.0)], 50, 3),
                                                ([(0.0, 1.0), (-2.0, -1.0)], 5000, 64)])
def test_seeded_draws_follow_emukits_update_parameters(bounds, grid_size, k):
    X = np.arange(4 * len(bounds), dtype=np.float64).reshape(4, len(bounds))
    a, b = 0.37, -0.21
    np.random.seed(77)
    grid = gumbel_grid(bounds, grid_size, X)
    mins = gumbel_mins(k, a, b)
    after = np.random.rand()
    # numpy restatement: the grid (one uniform per parameter, model.X on top), then rand(num_samples), the transform
    np.random.seed(77)
    expect_grid = np.vstack([X, np.hstack([np.random.uniform(lo, hi, (grid_size, 1)) for lo, hi in bounds])])
    u = np.random.rand(k)
    expect_mins = np.log(-np.log(1 - u)) * b + a
    assert np.array_equal(grid, expect_grid)
    assert np.array_equal(mins, expect_mins)
    assert after == np.random.rand()
    # the grid's draws are the optimiser's uniform anchors
    np.random.seed(77)
    assert np.array_equal(CausalGradientAcquisitionOptimizer(bounds, anchors="uniform").sample_uniform(grid_size),
                          expect_grid[X.shape[0]:])


def test_no_gradients_and_refinement_is_refused():
    mes = MaxValueEntropySearch(StubModel(), [(0.0, 1.0), (0.0, 1.0)])
    assert mes.has_gradients is False
    q = mes / Cost({"a": lambda x: 1.0}, ["a"])
    assert isinstance(q, AcquisitionQuotient) and q.numerator is mes
    opt = CausalGradientAcquisitionOptimizer([(0.0, 1.0), (0.0, 1.0)], grid_shape=[4, 4])
    for acq in (mes, q):
        with pytest.raises(ValueError, match="no gradients"):
            opt.optimize(acq, refine=True)
    with pytest.raises(ValueError, match="no gradients"):
        CausalGradientAcquisitionOptimizer([(0.0, 1.0)], anchors="uniform").optimize(q)


def test_too_many_samples_are_refused_before_any_draw():
    mes = MaxValueEntropySearch(StubModel(), [(0.0, 1.0), (0.0, 1.0)], num_samples=65)
    np.random.seed(3)
    with pytest.raises(ValueError, match="num_samples"):
        mes.update_parameters()
    after = np.random.rand()
    np.random.seed(3)
    assert after == np.random.rand()


def test_find_next_y_point_refuses_what_mes_cannot_do():
    args = ([(0.0, 1.0)], StubModel(), 0.0, ["a"], {"a": lambda x: 1.0})
    with pytest.raises(ValueError, match="task"):
        find_next_y_point(*args, task="max", acquisition="MES")
    with pytest.raises(ValueError, match="gradients"):
        find_next_y_point(*args, anchors="uniform", acquisition="MES")
    with pytest.raises(ValueError, match="acquisition"):
        find_next_y_point(*args, acquisition="UCB")


def test_find_next_y_point_default_is_unchanged():
    params = inspect.signature(find_next_y_point).parameters
    assert params["acquisition"].default == "EI"
    assert list(params)[:10] == ["space", "model", "current_global_best", "evaluated_set", "costs_functions", "task",
                                 "grid_shape", "candidates", "anchors", "num_anchor_points"]
    assert params["task"].default == "min" and params["anchors"].default == "grid"
    # the argument checks of the default path draw nothing from numpy's global stream
    np.random.seed(11)
    with pytest.raises(ValueError):
        find_next_y_point([(0.0, 1.0)], StubModel(), 0.0, ["a"], {"a": lambda x: 1.0}, acquisition="UCB")
    after = np.random.rand()
    np.random.seed(11)
    assert after == np.random.rand()
