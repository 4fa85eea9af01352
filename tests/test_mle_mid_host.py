"""CPU tests of the device MLE for models of 129..256 observations: the entry point's declaration and
binding, and the ``device_rows`` checks of the Python layers, which come before the library is loaded."""
import importlib
import os
import re

import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib

gpf = importlib.import_module("cbo_with_oop_amd.GaussianProcessFactory")       # (the package exports the class by that name)


def test_the_entry_point_is_declared_and_bound():
    import ctypes
    header = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"int cbo_gp_mle_sets_rows\(int n_models, cbo_gp \*const \*gps, const cbo_mle_run \*runs, int max_rows, "
                     r"int \*model_status_out\);", header)
    assert "cbo_gp_mle_sets_rows" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["cbo_gp_mle_sets_rows"]
    old = _lib.SIGNATURES["cbo_gp_mle_sets"][1]
    assert restype is ctypes.c_int and argtypes == old[:3] + [ctypes.c_int] + old[3:]
    assert int(re.search(r"#define CBO_HIP_ABI_VERSION (\d+)", header).group(1)) == 5


@pytest.fixture
def no_library(monkeypatch):
    """Loading the library is an error: what follows must be decided on the host alone."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def test_device_rows_is_checked_before_the_library_is_loaded(no_library):
    for bad in (0, 129, 512, True):
        with pytest.raises(ValueError, match="device_rows"):
            gpf.checked_mle_device_rows(bad)
        with pytest.raises(ValueError, match="device_rows"):
            gpf.checked_mle_device_rows(bad, "host")
    with pytest.raises(ValueError, match="device_rows"):
        gpf.checked_mle_device_rows(256, "host")
    assert gpf.checked_mle_device_rows(128, "host") == 128
    assert gpf.checked_mle_device_rows(128) == 128 and gpf.checked_mle_device_rows(256, "device") == 256


def test_every_layer_refuses_a_bad_device_rows_before_any_device_call(no_library):
    from cbo_with_oop_amd.CBO import CBO, CBOAcquisitionPath
    from cbo_with_oop_amd.utils_functions.utils import fit_gaussian_process, fit_gaussian_processes
    for bad in (0, 129, 512, True):
        with pytest.raises(ValueError, match="device_rows"):
            gpf.optimize_together([object()], optimizer="device", device_rows=bad)
        with pytest.raises(ValueError, match="device_rows"):
            gpf.mle_runs_device([object()], [[1.0, 1.0]], 3, device_rows=bad)
        with pytest.raises(ValueError, match="device_rows"):
            fit_gaussian_process(None, None, None, optimizer="device", device_rows=bad)
        with pytest.raises(ValueError, match="device_rows"):
            fit_gaussian_processes([], [], [], optimizer="device", device_rows=bad)
        with pytest.raises(ValueError, match="device_rows"):
            CBOAcquisitionPath(None, [["X"]], None, "min", [], [], [None], mle_optimizer="device", mle_device_rows=bad)
        with pytest.raises(ValueError, match="device_rows"):
            CBO(None, None, None, None, mle_optimizer="device", mle_device_rows=bad)
    # 256 chooses what the device launch takes: with the host optimiser it is refused
    with pytest.raises(ValueError, match="device_rows"):
        gpf.optimize_together([object()], device_rows=256)
    with pytest.raises(ValueError, match="device_rows"):
        fit_gaussian_processes([], [], [], device_rows=256)
    with pytest.raises(ValueError, match="device_rows"):
        CBO(None, None, None, None, mle_device_rows=256)
    with pytest.raises(ValueError, match="device_rows"):
        gpf.HipGaussianProcess.optimize(object(), device_rows=256)
    with pytest.raises(ValueError, match="device_rows"):
        gpf.HipGaussianProcess.optimize_restarts(object(), num_restarts=2, device_rows=512)
    # the defaults pass, with either optimiser
    assert gpf.optimize_together([], device_rows=128) == []
    assert gpf.optimize_together([], optimizer="device", device_rows=256) == []
