"""CPU tests of the joint-posterior surface: the two covariance entry points are declared, exported and prototyped, and
HipGaussianProcess carries GPy's and emukit's covariance methods.  Their results are checked on the GPU
(tests/test_covariance_gpu.py)."""
import inspect
import os
import re

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess

COV_SYMBOLS = ("cbo_gp_predict_cov", "cbo_gp_cov_between")


def test_covariance_entry_points_are_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in COV_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/cbo_hip.h"
        assert hasattr(lib, name), f"{name} not exported by libcbo_hip.so"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype"
    assert len(_lib.SIGNATURES["cbo_gp_predict_cov"][1]) == 8
    assert len(_lib.SIGNATURES["cbo_gp_cov_between"][1]) == 8


def test_model_has_the_gpy_and_emukit_covariance_methods():
    for name in ("posterior_covariance_between_points", "predict_with_full_covariance", "predict_covariance",
                 "get_covariance_between_points", "calculate_variance_reduction"):
        assert callable(getattr(HipGaussianProcess, name, None)), name
    params = inspect.signature(HipGaussianProcess.predict).parameters
    assert list(params)[:3] == ["self", "x", "include_likelihood"]
    assert params["include_likelihood"].default is True
    assert params["full_cov"].default is False
    assert inspect.signature(HipGaussianProcess.predict_covariance).parameters["with_noise"].default is True
