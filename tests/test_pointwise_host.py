"""CPU tests of the point-wise acquisitions (LCB, PI, plug-in EI, model variance): cbo_acq_sweep_kind and
cbo_gp_plugin_incumbent are declared, exported and prototyped, the four classes only store their arguments and refuse bad
ones, find_next_y_point knows the four names and keeps refusing the others, and the host gradients agree with central finite
differences on a closed-form stub model.  The values are checked on the GPU (tests/test_pointwise_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import (AcquisitionProduct, AcquisitionQuotient, CausalExpectedImprovement,
                                              CausalMeanPluginExpectedImprovement, CausalNegativeLowerConfidenceBound,
                                              CausalProbabilityOfImprovement, Cost, ModelVariance,
                                              ProbabilityOfFeasibility, find_next_y_point)
from cbo_with_oop_amd.utils_functions.causal_optimizer import _numerator, has_gradients

NAMES = ("LCB", "PI", "MPEI", "VAR")


class Untouchable:
    """Construction and argument checks must not touch the model."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was asked for {name!r}")


def test_entry_points_are_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    assert re.search(r"CBO_ACQ_LCB\s*=\s*1\s*,\s*CBO_ACQ_PI\s*=\s*2\s*,\s*CBO_ACQ_VAR\s*=\s*3\s*,\s*CBO_ACQ_MPEI\s*=\s*4", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+cbo_acq_sweep_kind\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, "cbo_acq_sweep_kind not declared in include/cbo_hip.h"
    assert len(decl.group(1).split(",")) == 12
    decl = re.search(r"\bint\s+cbo_gp_plugin_incumbent\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 3
    lib = _lib.load()
    assert hasattr(lib, "cbo_acq_sweep_kind") and hasattr(lib, "cbo_gp_plugin_incumbent"), "not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_kind"]
    assert restype is ctypes.c_int and len(argtypes) == 12
    assert argtypes[2] is ctypes.c_int and argtypes[3] is ctypes.c_double and argtypes[4] is ctypes.c_int
    assert argtypes[5] is ctypes.c_double and argtypes[6] is ctypes.c_double and argtypes[11] is _lib.c_int64_p
    restype, argtypes = _lib.SIGNATURES["cbo_gp_plugin_incumbent"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_int, _lib.c_double_p]
    assert _lib.ACQ_KIND_CODE == {"LCB": 1, "PI": 2, "VAR": 3, "MPEI": 4}
    assert _lib.ABI_VERSION == 5 and lib.cbo_abi_version() == 5


def test_invalid_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    out = ctypes.c_double()
    for kind in (0, 5, -1):
        assert lib.cbo_acq_sweep_kind(None, None, kind, 0.0, 0, 0.0, 1.0, None, None, None, None, None) == _lib.CBO_ERR_INVALID
        assert b"kind" in lib.cbo_last_error()
    for kind in (1, 2, 3, 4):
        assert lib.cbo_acq_sweep_kind(None, None, kind, 0.0, 0, 0.0, 1.0, None, None, None, None, None) == _lib.CBO_ERR_INVALID
    assert lib.cbo_gp_plugin_incumbent(None, 0, ctypes.byref(out)) == _lib.CBO_ERR_INVALID
    assert lib.cbo_last_error()


def test_classes_store_their_arguments_and_refuse_bad_ones():
    model = Untouchable()
    params = inspect.signature(CausalNegativeLowerConfidenceBound.__init__).parameters
    assert list(params) == ["self", "task", "model", "beta"] and params["beta"].default == 1.0
    params = inspect.signature(CausalProbabilityOfImprovement.__init__).parameters
    assert list(params) == ["self", "current_global_min", "task", "model", "jitter"] and params["jitter"].default == 0.0
    params = inspect.signature(CausalMeanPluginExpectedImprovement.__init__).parameters
    assert list(params) == ["self", "task", "model", "jitter"] and params["jitter"].default == 0.0
    assert list(inspect.signature(ModelVariance.__init__).parameters) == ["self", "model"]
    state = np.random.get_state()
    lcb = CausalNegativeLowerConfidenceBound("min", model)
    assert lcb.model is model and lcb.beta == 1.0 and lcb.task == "min"
    assert CausalNegativeLowerConfidenceBound("max", model, beta=0.0).beta == 0.0
    pi = CausalProbabilityOfImprovement(0.3, "max", model, jitter=0.01)
    assert pi.model is model and pi.current_global_min == 0.3 and pi.jitter == 0.01 and pi.task == "max"
    mpei = CausalMeanPluginExpectedImprovement("min", model)
    assert mpei.model is model and mpei.jitter == 0.0
    assert ModelVariance(model).model is model
    for beta in (-1.0, -1e-300, np.nan, np.inf, -np.inf, "wide", None):
        with pytest.raises(ValueError, match="beta"):
            CausalNegativeLowerConfidenceBound("min", model, beta=beta)
    for jitter in (np.nan, np.inf, None):
        with pytest.raises(ValueError, match="jitter"):
            CausalProbabilityOfImprovement(0.0, "min", model, jitter=jitter)
        with pytest.raises(ValueError, match="jitter"):
            CausalMeanPluginExpectedImprovement("min", model, jitter=jitter)
    for cls, args in ((CausalNegativeLowerConfidenceBound, ()), (CausalMeanPluginExpectedImprovement, ())):
        with pytest.raises(ValueError, match="task"):
            cls("smallest", model, *args)
    with pytest.raises(ValueError, match="task"):
        CausalProbabilityOfImprovement(0.0, "MIN", model)
    for acq in (lcb, pi, mpei, ModelVariance(model)):
        assert acq.has_gradients is True
        params = inspect.signature(acq.sweep).parameters
        assert list(params) == ["candidates", "cost", "want_acq", "want_posterior"]
        assert params["cost"].default == 1.0 and params["want_acq"].default is False
        assert params["want_posterior"].default is False
    # a non-finite incumbent is refused when it is used, before the device is
    with pytest.raises(ValueError, match="current_global_min"):
        CausalProbabilityOfImprovement(np.nan, "min", model)._scalars()
    new = np.random.get_state()
    assert state[0] == new[0] and np.array_equal(state[1], new[1]) and state[2:] == new[2:]


def test_quotients_and_products():
    model = Untouchable()
    cost = Cost({"X": lambda col: 2.0}, ["X"])
    for acq in (CausalNegativeLowerConfidenceBound("min", model), CausalProbabilityOfImprovement(0.0, "min", model),
                CausalMeanPluginExpectedImprovement("max", model), ModelVariance(model)):
        quot = acq / cost
        assert isinstance(quot, AcquisitionQuotient) and quot.numerator is acq and quot.denominator is cost
        assert quot.model is model and _numerator(quot) is acq and has_gradients(quot)
        # a product with a probability of feasibility has no device pass: it keeps being refused
        with pytest.raises(ValueError):
            AcquisitionProduct([acq, ProbabilityOfFeasibility(model)])
        with pytest.raises(ValueError):
            CausalExpectedImprovement(0.0, "min", model) * acq


def test_find_next_y_point_argument_checks():
    params = list(inspect.signature(find_next_y_point).parameters)
    assert params[:10] == ["space", "model", "current_global_best", "evaluated_set", "costs_functions", "task",
                           "grid_shape", "candidates", "anchors", "num_anchor_points"]
    sig = inspect.signature(find_next_y_point).parameters
    assert sig["acquisition"].default == "EI" and sig["task"].default == "min" and sig["anchors"].default == "grid"
    model = Untouchable()
    space, sets, costs = [(-1.0, 1.0)], ["X"], {"X": lambda col: 1.0}
    state = np.random.get_state()
    for name in ("UCB", "ucb", "lcb", "EI2", "", None):
        with pytest.raises(ValueError, match="acquisition") as info:
            find_next_y_point(space, model, 0.0, sets, costs, acquisition=name)
        for known in NAMES:
            assert repr(known) in str(info.value)
    pof = ProbabilityOfFeasibility(model)
    for name in NAMES:
        with pytest.raises(ValueError, match="constraints"):
            find_next_y_point(space, model, 0.0, sets, costs, acquisition=name, constraints=[pof])
        with pytest.raises(ValueError, match="batch"):
            find_next_y_point(space, model, 0.0, sets, costs, acquisition=name, batch_size=2)
        with pytest.raises(ValueError, match="hyper-parameter"):
            find_next_y_point(space, model, 0.0, sets, costs, acquisition=name, hyper_samples=np.ones((2, 3)))
        with pytest.raises(ValueError, match="hyper-parameter"):
            find_next_y_point(space, model, 0.0, sets, costs, acquisition=name, hyper_samples=4, anchors="uniform")
    new = np.random.get_state()
    assert state[0] == new[0] and np.array_equal(state[1], new[1]) and state[2:] == new[2:]


class ClosedFormModel:
    """mean = sin(x0) + x1^2, variance = 0.2 + 0.1 cos(x0 x1)^2: predict and its gradients in closed form."""

    def predict(self, x):
        return (np.sin(x[:, :1]) + x[:, 1:2] ** 2), 0.2 + 0.1 * np.cos(x[:, :1] * x[:, 1:2]) ** 2

    def get_prediction_gradients(self, x):
        dmean = np.hstack([np.cos(x[:, :1]), 2 * x[:, 1:2]])
        p = x[:, :1] * x[:, 1:2]
        dvar = -0.2 * np.cos(p) * np.sin(p) * np.hstack([x[:, 1:2], x[:, :1]])
        return dmean, dvar


@pytest.mark.parametrize("task", ["min", "max"])
def test_host_gradients_agree_with_finite_differences(task):
    model = ClosedFormModel()
    acqs = [CausalNegativeLowerConfidenceBound(task, model, beta=1.7), CausalProbabilityOfImprovement(0.4, task, model, 0.02),
            ModelVariance(model)]
    x = np.random.default_rng(5).uniform(-1.0, 1.0, (6, 2))
    h = 1e-6
    for acq in acqs:
        f, df = acq.evaluate_with_gradients(x)
        assert f.shape == (6, 1) and df.shape == (6, 2)
        for k in range(2):
            e = np.zeros(2)
            e[k] = h
            fd = (acq.evaluate_with_gradients(x + e)[0] - acq.evaluate_with_gradients(x - e)[0])[:, 0] / (2 * h)
            np.testing.assert_allclose(df[:, k], fd, rtol=1e-6, atol=1e-8)
    # the formulas' values
    mean, var = model.predict(x)
    sd = np.sqrt(var)
    f = acqs[0].evaluate_with_gradients(x)[0]
    np.testing.assert_array_equal(f, -(mean - 1.7 * sd) if task == "min" else mean + 1.7 * sd)
    np.testing.assert_array_equal(acqs[2].evaluate_with_gradients(x)[0], var)
