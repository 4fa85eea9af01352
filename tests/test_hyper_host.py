"""Host tests of the hyper-parameter-marginalised causal EI (cbo_acq_sweep_hyper): the sampler
(`hmc_sample`, GPy's HMC restated) against an independent restatement of its recipe written here, the argument checks of the
Python layer, and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def header_text():
    with open(os.path.join(ROOT, "include", "cbo_hip.h")) as fh:
        return fh.read()


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def softplus(x):
    return np.log1p(np.exp(x))


def softplus_inverse(theta):
    return np.log(np.expm1(theta))


def stub_target(x):
    """f = |x|^2 / 2, grad f = x: a standard normal in the transformed space."""
    return 0.5 * float(np.dot(x, x)), x.copy()


def recipe(theta0, num_samples, hmc_iters, stepsize):
    """GPy's HMC with M = I on the stub target, written from the recipe (not from the code under test): the chain lives on
    x = log(exp(theta) - 1); per sample one multivariate_normal draw, H_old, the row, leapfrog steps, H_new, one rand()."""
    x = softplus_inverse(np.asarray(theta0, dtype=np.float64))
    P = x.size
    rows = np.empty((num_samples, P))
    const = P * np.log(2 * np.pi) / 2
    for i in range(num_samples):
        p = np.random.multivariate_normal(np.zeros(P), np.eye(P))
        H_old = 0.5 * float(x @ x) + const + float(p @ p) / 2
        x_old = x.copy()
        rows[i] = softplus(x)
        for _ in range(hmc_iters):
            p = p - stepsize / 2 * x
            x = x + stepsize * p
            p = p - stepsize / 2 * x
        H_new = 0.5 * float(x @ x) + const + float(p @ p) / 2
        accept = min(1.0, np.exp(H_old - H_new))
        if np.random.rand() < accept:
            rows[i] = softplus(x)
        else:
            x = x_old
    return rows


@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("stepsize", [0.1, 0.9])
def test_hmc_sample_follows_the_recipe_draw_for_draw(seed, stepsize):
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_sample
    theta0 = np.array([1.0, 0.5, 2.0])
    np.random.seed(seed)
    got = hmc_sample(stub_target, theta0, 40, 6, stepsize)
    after = np.random.rand()
    np.random.seed(seed)
    want = recipe(theta0, 40, 6, stepsize)
    assert got.shape == (40, 3)
    assert np.max(np.abs(got - want)) <= 1e-12
    assert after == np.random.rand()                       # the same number of draws was taken from the global generator


def test_a_rejected_step_restores_the_parameters():
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_sample
    theta0 = np.array([1.0, 2.0])
    np.random.seed(3)
    rows = hmc_sample(stub_target, theta0, 4, 3, 1e200)    # x explodes, f = inf, H_new = inf: never accepted
    assert np.allclose(rows, np.tile(theta0, (4, 1)), rtol=1e-15, atol=0)
    # ... and the chain goes on from the restored state: a sane step afterwards moves from theta0
    calls = []

    def target(x):
        calls.append(x.copy())
        return stub_target(x)

    np.random.seed(3)
    hmc_sample(target, theta0, 2, 1, 1e200)
    assert np.allclose(calls[0], softplus_inverse(theta0))
    # sample 1's first proposal starts from the restored x: x0 + stepsize * (p - stepsize / 2 * x0)
    np.random.seed(3)
    p0 = np.random.multivariate_normal(np.zeros(2), np.eye(2))
    np.random.rand()
    p1 = np.random.multivariate_normal(np.zeros(2), np.eye(2))
    x0 = softplus_inverse(theta0)
    with np.errstate(over="ignore"):
        assert np.array_equal(calls[2], x0 + 1e200 * (p1 - 1e200 / 2 * x0))
    assert not np.array_equal(p0, p1)


def test_burn_in_and_thinning_leave_n_samples_rows():
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_sample
    n_samples, n_burnin, subsample_interval = 7, 13, 3
    np.random.seed(0)
    rows = hmc_sample(stub_target, np.array([1.0]), n_burnin + n_samples * subsample_interval, 2, 0.1)
    assert rows[n_burnin::subsample_interval].shape == (n_samples, 1)


# ---- argument checks of the Python layer (no device is touched before they fire) -----------------------------------------
class _Model:
    causal = False
    fix_noise = False
    noise_var = 1e-2
    lengthscale = np.array([1.0])


def _ei(model):
    from cbo_with_oop_amd import CausalExpectedImprovement
    return CausalExpectedImprovement(0.0, "min", model)


SAMPLES = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 2e-2]])


def test_integrated_acquisition_accepts_the_causal_ei_bare_or_over_a_cost():
    from cbo_with_oop_amd import IntegratedHyperParameterAcquisition
    from cbo_with_oop_amd.utils_functions import Cost
    a = IntegratedHyperParameterAcquisition(_Model(), _ei, samples=SAMPLES)
    assert a.n_samples == 2 and a.has_gradients is False and np.array_equal(a.samples, SAMPLES)
    b = IntegratedHyperParameterAcquisition(_Model(), lambda m: _ei(m) / Cost({"X": lambda col: 1.0}, ["X"]), samples=SAMPLES)
    assert b.n_samples == 2


def test_integrated_acquisition_rejects_other_acquisitions_naming_what_is_supported():
    from cbo_with_oop_amd import IntegratedHyperParameterAcquisition
    from cbo_with_oop_amd.utils_functions import AcquisitionQuotient, MaxValueEntropySearch

    class Other:
        pass

    mes = MaxValueEntropySearch.__new__(MaxValueEntropySearch)
    mes.model = _Model()
    for generator in (lambda m: Other(), lambda m: mes, lambda m: AcquisitionQuotient(mes, None)):
        with pytest.raises(TypeError, match="CausalExpectedImprovement"):
            IntegratedHyperParameterAcquisition(_Model(), generator, samples=SAMPLES)


@pytest.mark.parametrize("samples", [np.ones((2, 2)), np.ones((2, 4)), np.ones((0, 3)), np.ones((257, 3))])
def test_integrated_acquisition_rejects_samples_of_the_wrong_shape(samples):
    from cbo_with_oop_amd import IntegratedHyperParameterAcquisition
    with pytest.raises(ValueError):
        IntegratedHyperParameterAcquisition(_Model(), _ei, samples=samples)


def test_a_fixed_noise_model_takes_samples_without_the_noise_column():
    from cbo_with_oop_amd import IntegratedHyperParameterAcquisition

    class Fixed(_Model):
        fix_noise = True
        noise_var = 1e-2

    a = IntegratedHyperParameterAcquisition(Fixed(), _ei, samples=SAMPLES[:, :2])
    assert np.array_equal(a.samples, np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 1e-2]]))


@pytest.mark.parametrize("n_samples", [0, -1, 2.5, True, None])
def test_integrated_acquisition_rejects_a_sample_count_that_is_no_positive_int(n_samples):
    from cbo_with_oop_amd import IntegratedHyperParameterAcquisition
    with pytest.raises(ValueError):
        IntegratedHyperParameterAcquisition(_Model(), _ei, n_samples=n_samples)


@pytest.mark.parametrize("kwargs", [dict(acquisition="MES"), dict(constraints=[]), dict(constraints=[object()]),
                                    dict(batch_size=2), dict(anchors="uniform"), dict(hyper_samples=0),
                                    dict(hyper_samples=-3), dict(hyper_samples=True)])
def test_find_next_y_point_rejects_what_hyper_samples_cannot_be_combined_with(kwargs):
    from cbo_with_oop_amd import find_next_y_point
    kw = dict(hyper_samples=SAMPLES)
    kw.update(kwargs)
    with pytest.raises(ValueError):
        find_next_y_point([(0.0, 1.0)], _Model(), 0.0, ["X"], {"X": lambda col: 1.0}, **kw)


# ---- the binding -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_marginalised_sweep():
    text = header_text()
    m = re.search(r"int\s+cbo_acq_sweep_hyper\s*\(([^;]*)\)\s*;", text)
    assert m, "include/cbo_hip.h does not declare cbo_acq_sweep_hyper"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 11
    assert re.search(r"#define\s+CBO_MAX_HYPER_SAMPLES\s+256\b", text)
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)


def test_lib_binds_the_marginalised_sweep_with_its_signature():
    from cbo_with_oop_amd import _lib
    P, I64P = _lib.c_double_p, _lib.c_int64_p
    assert "cbo_acq_sweep_hyper" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_hyper"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, P, ctypes.c_double, ctypes.c_int, ctypes.c_double,
                        ctypes.c_double, P, P, I64P]
    assert _lib.MAX_HYPER_SAMPLES == 256 and _lib.ABI_VERSION == 5
