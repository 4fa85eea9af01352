"""CPU tests of the joint posterior samples: cbo_gp_posterior_samples is declared, exported and prototyped, HipGaussianProcess
carries GPy's two sampling methods, and the host-drawn normals and likelihood noise consume numpy's global stream exactly
as GPy does.  The samples themselves are checked on the GPU (tests/test_posterior_samples_gpu.py)."""
import inspect
import os
import re

import numpy as np

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess, gaussian_likelihood_samples, standard_normals


def test_samples_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "cbo_gp_posterior_samples"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/cbo_hip.h"
    assert hasattr(_lib.load(), name), f"{name} not exported by libcbo_hip.so"
    assert len(_lib.SIGNATURES[name][1]) == 10
    assert _lib.ABI_VERSION == 5


def test_model_has_gpys_sampling_methods():
    params = inspect.signature(HipGaussianProcess.posterior_samples_f).parameters
    assert list(params)[:3] == ["self", "X", "size"]
    assert params["size"].default == 10
    params = inspect.signature(HipGaussianProcess.posterior_samples).parameters
    assert list(params)[:5] == ["self", "X", "size", "Y_metadata", "likelihood"]
    assert params["size"].default == 10
    assert params["Y_metadata"].default is None and params["likelihood"].default is None


def test_normals_leave_the_stream_where_multivariate_normal_does():
    for size, M in ((1, 1), (10, 7), (33, 130)):
        np.random.seed(1234)
        z = standard_normals(size, M)
        after = np.random.rand()
        np.random.seed(1234)
        x = np.random.multivariate_normal(np.zeros(M), np.eye(M), size)
        expect = np.random.rand()
        assert z.shape == (size, M)
        assert after == expect
        # with the identity covariance the draws are the normals themselves (up to the SVD's signs)
        assert np.allclose(np.abs(x), np.abs(z))


def test_likelihood_noise_consumes_one_normal_per_element_in_order():
    f = np.arange(12.0).reshape(4, 3) * 0.5
    np.random.seed(99)
    y = gaussian_likelihood_samples(f, 0.25)
    after = np.random.rand()
    np.random.seed(99)
    expect = np.array([np.random.normal(fj, 0.5, size=1) for fj in f.flatten()]).reshape(f.shape)
    assert np.array_equal(y, expect)
    assert after == np.random.rand()
