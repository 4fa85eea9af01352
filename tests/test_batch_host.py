"""Host tests of greedy batch selection (cbo_acq_sweep_batch, the Kriging believer): the ABI, the argument
checks of the Python layer, and the two identities the device path rests on, checked on a golden fixture against a numpy
restatement of emukit's GreedyBatchPointCalculator loop -- `believer` below, which the GPU tests compare the device with.

The restatement is emukit's loop on the fp64 oracle: fit on the data, sweep, arg-max; then the picked point joins the data
with y_new = predict(x_new)[0] (a full refit, as emukit's model.set_data does) and the loop picks again.

Tolerance of the identities.  Both sides are backward-stable fp64 solves with the same Ky (the refit's is Ky bordered by
one row): each carries a relative error of a modest multiple of n eps cond(Ky) in its solution (Higham, Accuracy and
Stability, Thm 10.4: Cholesky solves satisfy (A + dA) x = b with |dA| <= c n eps |A|).  The bound used is
IDENTITY_C n eps cond(Ky_augmented) with IDENTITY_C = 4 (two solves per side), times the scale of the quantity: max|y - m|
+ max|mean| for the mean, the prior variance for the variance."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_fixture
from oracle import gp_oracle as O

EPS = 2.220446049250313e-16
IDENTITY_C = 4.0


def model_args(f):
    return dict(variance=float(f["variance"]), lengthscale=f["lengthscale_arg"], noise_var=float(f["noise_var"]))


def believer(f, batch_size, y_best=None, task=None, cost=None, update_incumbent=False, ei_jitter=0.0, Xs=None, mXs=None,
             vXs=None):
    """emukit's GreedyBatchPointCalculator on the oracle.  f: a golden fixture (X, y, priors, hyper-parameters); Xs (with
    mXs, vXs for a causal model) default to the fixture's candidates.  Returns a dict: idx (B,), val (B,), gap (B,) -- the
    relative distance between the best and the runner-up acquisition at every pick -- acq / mean / var at the last pick,
    the data every pick was fitted on (`data`: list of (X, y, mX, vX)) and the incumbent every pick saw (`y_best`)."""
    X, y, mX, vX = f["X"], f["y"], f["mX"], f["vX"]
    if Xs is None:
        Xs, mXs, vXs = f["Xs"], f["mXs"], f["vXs"]
    y_best = float(f["y_best"]) if y_best is None else float(y_best)
    task = f["task"] if task is None else task
    cost = float(f["cost"]) if cost is None else float(cost)
    out = dict(idx=[], val=[], gap=[], data=[], y_best=[])
    for _ in range(batch_size):
        post = O.fit(X, y, mX, vX, **model_args(f))
        acq, val, idx, mean, var = O.acquisition_sweep(post, Xs, y_best, mXs, vXs, task, cost, ei_jitter)
        a = acq[:, 0]
        runner_up = np.max(np.delete(a, idx)) if a.size > 1 else -np.inf
        out["gap"].append(abs(val - runner_up) / max(abs(val), 1e-300))
        out["idx"].append(idx); out["val"].append(val); out["data"].append((X, y, mX, vX)); out["y_best"].append(y_best)
        out.update(acq=acq, mean=mean, var=var)
        y_new = float(mean[idx, 0])                                   # model.predict(x_new)[0]
        X = np.vstack([X, Xs[idx:idx + 1]])
        y = np.vstack([y, [[y_new]]])
        if mX is not None:
            mX = np.vstack([mX, mXs[idx:idx + 1]])
            vX = np.vstack([vX, vXs[idx:idx + 1]])
        if update_incumbent:
            y_best = min(y_best, y_new) if task == "min" else max(y_best, y_new)
    out["idx"] = np.array(out["idx"], dtype=np.int64)
    out["val"] = np.array(out["val"])
    out["gap"] = np.array(out["gap"])
    return out


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def header_text():
    with open(os.path.join(ROOT, "include", "cbo_hip.h")) as fh:
        return fh.read()


def test_header_declares_the_batch_sweep():
    text = header_text()
    m = re.search(r"int\s+cbo_acq_sweep_batch\s*\(([^;]*)\)\s*;", text)
    assert m, "include/cbo_hip.h does not declare cbo_acq_sweep_batch"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 13
    assert re.search(r"#define\s+CBO_MAX_BATCH\s+64\b", text)


def test_lib_binds_the_batch_sweep_with_its_signature():
    from cbo_with_oop_amd import _lib
    P, I64P = _lib.c_double_p, _lib.c_int64_p
    assert "cbo_acq_sweep_batch" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_batch"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                        ctypes.c_int, ctypes.c_int, P, I64P, P, P, P]


def test_abi_version_is_still_5():
    from cbo_with_oop_amd import _lib
    assert _lib.ABI_VERSION == 5
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", header_text())


# ---- argument checks of the Python layer (no device is touched before they fire) -----------------------------------------
class _Model:
    causal = False


def _ei():
    from cbo_with_oop_amd import CausalExpectedImprovement
    return CausalExpectedImprovement(0.0, "min", _Model())


def _optimizer(anchors="grid"):
    from cbo_with_oop_amd.utils_functions import CausalGradientAcquisitionOptimizer
    return CausalGradientAcquisitionOptimizer([(0.0, 1.0)], grid_shape=[8], anchors=anchors)


@pytest.mark.parametrize("batch_size", [0, -1, 2.0, "3", None, True])
def test_calculator_rejects_a_batch_size_that_is_no_positive_int(batch_size):
    from cbo_with_oop_amd.utils_functions import GreedyBatchPointCalculator
    with pytest.raises(ValueError):
        GreedyBatchPointCalculator(_Model(), _ei(), _optimizer(), batch_size)


def test_calculator_accepts_the_causal_ei_bare_or_over_a_cost():
    from cbo_with_oop_amd.utils_functions import Cost, GreedyBatchPointCalculator
    ei = _ei()
    assert GreedyBatchPointCalculator(_Model(), ei, _optimizer(), 3).batch_size == 3
    quotient = ei / Cost({"X": lambda col: 1.0}, ["X"])
    assert GreedyBatchPointCalculator(_Model(), quotient, _optimizer(), np.int64(2)).batch_size == 2


def test_calculator_rejects_other_acquisitions():
    from cbo_with_oop_amd.utils_functions import (AcquisitionProduct, AcquisitionQuotient, GreedyBatchPointCalculator,
                                                  MaxValueEntropySearch)

    class Other:
        model = _Model()

    ei = _ei()
    mes = MaxValueEntropySearch.__new__(MaxValueEntropySearch)
    mes.model = _Model()
    product = AcquisitionProduct.__new__(AcquisitionProduct)
    for acquisition in (Other(), mes, product, AcquisitionQuotient(mes, None), AcquisitionQuotient(ei, Other())):
        with pytest.raises(ValueError):
            GreedyBatchPointCalculator(_Model(), acquisition, _optimizer(), 2)


def test_calculator_rejects_uniform_anchors():
    from cbo_with_oop_amd.utils_functions import GreedyBatchPointCalculator
    with pytest.raises(ValueError):
        GreedyBatchPointCalculator(_Model(), _ei(), _optimizer("uniform"), 2)


@pytest.mark.parametrize("kwargs", [dict(acquisition="MES"), dict(constraints=[]), dict(constraints=[object()]),
                                    dict(anchors="uniform"), dict(batch_size=0), dict(batch_size=2.5),
                                    dict(batch_size=True)])
def test_find_next_y_point_rejects_what_a_batch_cannot_be_combined_with(kwargs):
    from cbo_with_oop_amd import find_next_y_point
    kw = dict(batch_size=3)
    kw.update(kwargs)
    with pytest.raises(ValueError):
        find_next_y_point([(0.0, 1.0)], _Model(), 0.0, ["X"], {"X": lambda col: 1.0}, **kw)


def test_sweep_batch_rejects_a_batch_size_that_is_no_positive_int():
    for bad in (0, 1.5, None, False):
        with pytest.raises(ValueError):
            _ei().sweep_batch(np.zeros((4, 1)), bad)


# ---- the two identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["graph_ard_d4", "causal_d2", "toy_c1_Z50"])
def test_a_believed_point_leaves_the_mean_and_lowers_the_variance_by_the_rank_one_term(name):
    f = load_fixture(name)
    b = believer(f, 2)
    (X0, y0, mX0, vX0), (X1, y1, mX1, vX1) = b["data"]
    p = int(b["idx"][0])
    Xs, mXs, vXs = f["Xs"], f["mXs"], f["vXs"]
    post0 = O.fit(X0, y0, mX0, vX0, **model_args(f))
    post1 = O.fit(X1, y1, mX1, vX1, **model_args(f))
    assert post0.tries == 0 and post1.tries == 0
    mean0, var0 = O.predict(post0, Xs, mXs, vXs, include_noise=False)
    mean1, var1 = O.predict(post1, Xs, mXs, vXs, include_noise=False)
    # the contract's update from the ORIGINAL model's quantities
    from scipy.linalg import solve_triangular
    causal = vX0 is not None
    Kx = O.causal_K(X0, Xs, vX0, vXs if causal else None, post0.variance, post0.lengthscale, False)
    V = solve_triangular(post0.L, Kx, lower=True)
    q = np.sum(V * V, 0)
    kdiag = post0.variance + (float(vXs[p, 0]) if causal else 0.0)
    s2 = max(kdiag - q[p], 1e-15) + post0.noise_var + 1e-8
    kp = O.causal_K(Xs[p:p + 1], Xs, vXs[p:p + 1] if causal else None, vXs if causal else None, post0.variance,
                    post0.lengthscale, False)[0]
    c = kp - V[:, p] @ V
    w = c / np.sqrt(s2)
    kss = post0.variance + (vXs[:, 0] if causal else 0.0)
    var_formula = np.clip(kss - (q + w * w), 1e-15, np.inf)
    Ky1 = post1.L @ post1.L.T
    bound = IDENTITY_C * X1.shape[0] * EPS * np.linalg.cond(Ky1)
    resid = y0 - (mX0 if mX0 is not None else 0.0)
    mean_scale = np.max(np.abs(resid)) + np.max(np.abs(mean0))
    mean_err = np.max(np.abs(mean1 - mean0))
    var_err = np.max(np.abs(var1[:, 0] - var_formula))
    print(f"{name}: |mean change| {mean_err:.3e} (bound {bound * mean_scale:.3e}), |var - formula| {var_err:.3e} "
          f"(bound {bound * np.max(kss):.3e})")
    assert mean_err <= bound * mean_scale
    assert var_err <= bound * np.max(kss)
    # ... and the believed point itself is known to within its noise afterwards
    assert var1[p, 0] < var0[p, 0] and var1[p, 0] <= 2.0 * (post0.noise_var + 1e-8) + bound * np.max(kss)
