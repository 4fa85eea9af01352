"""Host checks of the leave-one-out interface (cbo_gp_loo, cbo_gp_loo_batch): the header declares both functions and the
binding knows them, the ABI version has not moved, and the closed form the device implements (loo_support.closed_form)
agrees with n brute-force refits on n - 1 points on the committed fixtures.

That last check also yields the tolerances of tests/test_loo_gpu.py.  G_FIXTURE[name] is the largest gap between closed form
and brute force on the fixture (mean relative to the scale of |y|, variance relative, lpd absolute: loo_support.gap) -- the
reference's own error; the GPU tolerance of a fixture is 10 x that (the device's summation orders and exponential against
numpy's), at least 1e-12.  The figures were produced by

    python -c "import sys; sys.path[:0] = ['tests', '.']; import test_loo_host as t; t.print_gaps()"

(numpy 2 / scipy with OpenBLAS, x86-64).  toy_bo_d2 is in: its noise is 1e-10, but its 20 points are far apart (condition
number of Ky 6.4) and the two forms agree on it to 7e-16, far better than the 1e-6 below which it may be used.
coral_max_d3 is the ill-conditioned one (condition number 4e9, left-out variances down to 2e-8): the brute-force variance
there is a difference of O(1) numbers, which is where its 1.6e-2 comes from.
G_SYNTHETIC[n] is the same figure for loo_support.synthetic(n) at noise 1e-2, the data of the general-path tests."""
import os
import re

import numpy as np
import pytest

import loo_support as S
from conftest import ROOT, load_fixture

G_FIXTURE = {"graph_ard_d4": 4.650e-14, "coral_max_d3": 1.646e-02, "causal_d2": 8.070e-14, "toy_bo_d2": 6.661e-16}
G_SYNTHETIC = {100: 1.459e-13, 128: 3.344e-13, 129: 2.820e-13, 200: 5.227e-13, 300: 7.687e-13, 515: 2.541e-12, 700: 4.340e-12,
               1100: 3.924e-12}
TOL_FLOOR = 1e-12


def gpu_tolerance(g):
    return max(10.0 * g, TOL_FLOOR)


def fixture_gap(name):
    Ky, r, y = S.fixture_system(load_fixture(name))
    return S.gap(S.closed_form(Ky, r, y), S.brute_force(Ky, r, y), y)


def synthetic_gap(n):
    X, y = S.synthetic(n)
    Ky, r, yy = S.ky_and_residual(X, y, noise_var=S.SYNTHETIC_NOISE)
    return S.gap(S.closed_form(Ky, r, yy), S.brute_force(Ky, r, yy), yy)


def print_gaps():
    for name in S.FIXTURE_NAMES:
        print(f"{name}: {fixture_gap(name):.3e}")
    for n in G_SYNTHETIC:
        print(f"synthetic {n}: {synthetic_gap(n):.3e}")


def test_header_declares_and_binding_knows_both_functions():
    from cbo_with_oop_amd import _lib
    with open(os.path.join(ROOT, "include", "cbo_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint\s+cbo_gp_loo\s*\(\s*cbo_gp\s*\*\s*gp\s*,\s*double\s*\*\s*mean_out\s*,\s*double\s*\*\s*var_out\s*,"
                     r"\s*double\s*\*\s*lpd_out\s*,\s*double\s*\*\s*sum_lpd_out\s*\)\s*;", header)
    assert re.search(r"\bint\s+cbo_gp_loo_batch\s*\(\s*int\s+n_models\s*,\s*cbo_gp\s*\*\s*const\s*\*\s*gps\s*,\s*double\s*\*"
                     r"\s*sum_lpd\s*,\s*double\s*\*\s*lpd_cat\s*,\s*int\s*\*\s*status\s*\)\s*;", header)
    assert len(_lib.SIGNATURES["cbo_gp_loo"][1]) == 5 and len(_lib.SIGNATURES["cbo_gp_loo_batch"][1]) == 5
    lib = _lib.load()                        # raises if the built library lacks a bound symbol
    assert lib.cbo_gp_loo.restype is not None and lib.cbo_gp_loo_batch.restype is not None


def test_abi_version_is_still_5():
    from cbo_with_oop_amd import _lib
    with open(os.path.join(ROOT, "include", "cbo_hip.h")) as fh:
        assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", fh.read())
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_python_surface_exists():
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.utils_functions import model_check
    assert all(callable(getattr(HipGaussianProcess, name)) for name in ("loo", "loo_predict", "loo_score"))
    assert callable(model_check.loo_scores) and callable(model_check.prefer_causal_prior)
    assert model_check.loo_scores([]) == []
    with pytest.raises(ValueError):
        model_check.prefer_causal_prior([object()], [])


@pytest.mark.parametrize("name", S.FIXTURE_NAMES)
def test_closed_form_agrees_with_brute_force(name):
    """The formula itself, on the CPU.  The three well-conditioned fixtures agree to far better than 1e-6, the bound below
    which a fixture may serve as one; every fixture reproduces its recorded figure to a factor of two (a rounding-error
    figure moves by about that much between BLAS builds; a figure of a few units in the last place by a few more)."""
    g = fixture_gap(name)
    print(f"{name}: closed form against brute force {g:.3e} (recorded {G_FIXTURE[name]:.3e})")
    if name != "coral_max_d3":
        assert g < 1e-6
    assert g <= max(2.0 * G_FIXTURE[name], 100 * np.finfo(np.float64).eps)


def test_closed_form_is_the_textbook_identity_on_a_case_done_by_hand():
    """n = 2, Ky = [[2, 1], [1, 2]], r = y = (1, 0): Ky^-1 = [[2, -1], [-1, 2]] / 3, alpha = (2, -1) / 3, c = (2, 2) / 3."""
    Ky = np.array([[2.0, 1.0], [1.0, 2.0]])
    y = np.array([1.0, 0.0])
    mean, var, lpd = S.closed_form(Ky, y, y)
    np.testing.assert_allclose(mean, [0.0, 0.5], atol=1e-15)
    np.testing.assert_allclose(var, [1.5, 1.5], rtol=1e-15)
    np.testing.assert_allclose(lpd, -0.5 * S.LOG_2PI - 0.5 * np.log(1.5) - 0.5 * np.array([1.0, 0.25]) / 1.5, rtol=1e-14)
    for a, b in zip(S.brute_force(Ky, y, y), (mean, var, lpd)):
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-15)
