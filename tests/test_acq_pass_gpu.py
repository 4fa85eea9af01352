"""GPU test of the EI pass (cbo_acq_sweep: acq_kernel, the candidate pass of csrc/acq_pass.h) at the sizes where the pass
changes path: a single candidate, an odd handful, one lane short of and one past a workgroup's span (256 lanes, two
candidates each), a ragged middle size, and past the grid-stride wrap of the 2048 workgroups with an odd tail.

acq is compared against oracle.gp_oracle.expected_improvement on the DEVICE's own mean and variance, over the cost, with the
bound test_parity_gpu.py::test_expected_improvement_over_the_whole_range_of_u uses for that comparison -- on the terms, since
u Phi(u) + phi(u) cancels in the lower tail: 48 eps (1 + u^2) s (|u| Phi(u) + phi(u)), over the cost as the values are.  The
winner is numpy's arg-max of the device's own values (lowest index on ties, NaN maximal), offset by the set's index_offset."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.stats

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 511, 513, 1000, 2 * 2048 * 256 + 3]


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


@pytest.fixture(scope="module")
def models(lib):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(3)
    X = rng.uniform(-2.0, 2.0, (40, 2))
    y = np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((40, 1))
    mf = lambda a: 0.3 * np.sin(a).sum(1, keepdims=True)
    va = lambda a: 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = HipGaussianProcess(X, y, variance=1.0, lengthscale=0.7, noise_var=1e-3)
        causal = HipGaussianProcess(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-4, mean_function=mf,
                                    variance_adjustment=va)
    return {"plain": plain, "causal": causal}


def sweep(lib, g, cands, y_best, task, cost):
    """cbo_acq_sweep: (acq, mean, var, best_val, best_idx)."""
    m = len(cands)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    lib.check(lib.load().cbo_acq_sweep(g._handle, cands._handle, float(y_best), lib.TASK_CODE[task], 0.0, float(cost),
                                       lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi)))
    return acq, mean, var, bv.value, bi.value


@pytest.mark.parametrize("m", SIZES)
def test_ei_pass_against_the_oracle_at_the_tail_sizes(lib, models, m):
    from cbo_with_oop_amd import CandidateGrid
    eps = np.finfo(float).eps
    pts = np.random.default_rng(m).uniform(-2.5, 2.5, (m, 2))
    for name, task, offset, cost in (("plain", "min", 0, 1.0), ("plain", "max", 0, 3.0), ("causal", "min", 1000, 3.0),
                                     ("causal", "max", 0, 1.0)):
        g = models[name]
        cands = CandidateGrid(pts, g, index_offset=offset)
        y_best = float(np.median(g.Y))
        acq, mean, var, bv, bi = sweep(lib, g, cands, y_best, task, cost)
        # without per-candidate outputs (the other instantiation of the kernel): the same winner
        wv, wi = ctypes.c_double(), ctypes.c_int64()
        lib.check(lib.load().cbo_acq_sweep(g._handle, cands._handle, y_best, lib.TASK_CODE[task], 0.0, cost, None, None,
                                           None, ctypes.byref(wv), ctypes.byref(wi)))
        cands.close()
        assert np.all(np.isfinite(mean)) and np.all(var > 0)
        ref = O.expected_improvement(mean, var, y_best, task) / cost
        s = np.sqrt(var)
        u = (y_best - mean) / s
        terms = s * (np.abs(u) * scipy.stats.norm.cdf(u) + scipy.stats.norm.pdf(u))
        bound = (48 * eps * (1.0 + u * u) * terms + 1e-300) / cost
        worst = float(np.max(np.abs(acq - ref) / bound))
        print(f"m={m} {name} {task} cost={cost}: worst |acq - oracle| / bound {worst:.3g}")
        assert worst <= 1.0, (name, task, worst)
        top = int(np.argmax(acq))
        assert bi == top + offset and bv == acq[top], (name, task, bi, top)
        assert wi.value == bi and wv.value == bv
