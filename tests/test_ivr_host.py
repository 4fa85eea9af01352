"""CPU tests of the integrated variance reduction: cbo_gp_integrated_variance_reduction is declared, exported and
prototyped, IntegratedVarianceReduction carries emukit's signature, and its integration points consume numpy's global
stream as emukit's space.sample_uniform does.  The values are checked on the GPU (tests/test_ivr_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import (AcquisitionQuotient, CausalGradientAcquisitionOptimizer, Cost,
                                              IntegratedVarianceReduction)

NAME = "cbo_gp_integrated_variance_reduction"


class StubModel:
    """Construction must not touch the model (emukit's __init__ only stores it)."""
    causal = False


def test_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text), f"{NAME} not declared in include/cbo_hip.h"
    assert hasattr(_lib.load(), NAME), f"{NAME} not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert len(argtypes) == 11
    assert argtypes[7] is ctypes.c_double          # cost
    assert _lib.ABI_VERSION == 5


def test_class_has_emukits_signature():
    params = inspect.signature(IntegratedVarianceReduction.__init__).parameters
    assert list(params) == ["self", "model", "space", "x_monte_carlo", "num_monte_carlo_points"]
    assert params["x_monte_carlo"].default is None
    assert params["num_monte_carlo_points"].default == 100000
    assert isinstance(params["num_monte_carlo_points"].default, int)
    ivr = IntegratedVarianceReduction(StubModel(), [(0.0, 1.0)], x_monte_carlo=np.array([[0.5]]))
    assert ivr.has_gradients is False
    params = inspect.signature(IntegratedVarianceReduction.sweep).parameters
    assert list(params) == ["self", "candidates", "cost", "want_acq"]
    assert params["cost"].default == 1.0 and params["want_acq"].default is False
    q = ivr / Cost({"a": lambda x: 1.0}, ["a"])
    assert isinstance(q, AcquisitionQuotient) and q.numerator is ivr


@pytest.mark.parametrize("bounds,n", [([(-5.0, 5.0)], 7), ([(-1.0, 2.0), (0.0, 10.0), (3.0, 4.0)], 50),
                                      ([(0.0, 1.0), (-2.0, -1.0)], 1000)])
def test_seeded_draws_follow_emukits_sample_uniform(bounds, n):
    np.random.seed(2024)
    ivr = IntegratedVarianceReduction(StubModel(), bounds, num_monte_carlo_points=n)
    after = np.random.rand()
    np.random.seed(2024)
    expect = np.hstack([np.random.uniform(lo, hi, (n, 1)) for lo, hi in bounds])
    assert np.array_equal(ivr._x_monte_carlo, expect)
    assert after == np.random.rand()
    # the same draws as the optimiser's uniform anchors
    np.random.seed(2024)
    assert np.array_equal(CausalGradientAcquisitionOptimizer(bounds, anchors="uniform").sample_uniform(n), expect)


def test_space_objects_are_accepted():
    class Param:
        def __init__(self, lo, hi):
            self.min, self.max = lo, hi

    class Space:
        parameters = [Param(-1.0, 1.0), Param(2.0, 3.0)]

    np.random.seed(5)
    ivr = IntegratedVarianceReduction(StubModel(), Space(), num_monte_carlo_points=20)
    np.random.seed(5)
    assert np.array_equal(ivr._x_monte_carlo, np.hstack([np.random.uniform(-1.0, 1.0, (20, 1)),
                                                         np.random.uniform(2.0, 3.0, (20, 1))]))


def test_out_of_domain_integration_points_raise():
    bounds = [(0.0, 1.0), (-1.0, 1.0)]
    ok = np.array([[0.0, -1.0], [1.0, 1.0], [0.5, 0.0]])
    assert np.array_equal(IntegratedVarianceReduction(StubModel(), bounds, x_monte_carlo=ok)._x_monte_carlo, ok)
    for bad in (np.array([[1.5, 0.0]]), np.array([[0.5, -1.01]]), np.array([[np.nan, 0.0]])):
        with pytest.raises(ValueError, match="domain"):
            IntegratedVarianceReduction(StubModel(), bounds, x_monte_carlo=np.vstack([ok, bad]))
    with pytest.raises(ValueError):
        IntegratedVarianceReduction(StubModel(), bounds, x_monte_carlo=np.zeros((3, 3)))


def test_refinement_needs_gradients():
    ivr = IntegratedVarianceReduction(StubModel(), [(0.0, 1.0)], x_monte_carlo=np.array([[0.5]]))
    opt = CausalGradientAcquisitionOptimizer([(0.0, 1.0)])
    with pytest.raises(ValueError, match="gradients"):
        opt.optimize(ivr, refine=True)
    with pytest.raises(ValueError, match="gradients"):
        opt.optimize(ivr / Cost({"a": lambda x: 1.0}, ["a"]), refine=True)
    with pytest.raises(ValueError, match="gradients"):
        CausalGradientAcquisitionOptimizer([(0.0, 1.0)], anchors="uniform").optimize(ivr)
