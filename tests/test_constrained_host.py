"""CPU tests of the constrained acquisition: cbo_acq_sweep_constrained is declared, exported and prototyped,
ProbabilityOfFeasibility carries emukit's signature and defaults, products flatten into one objective and its constraints,
what has no device pass is refused, and the host gradients (ProbabilityOfFeasibility's own, the product rule) agree with
central finite differences on closed-form stub models.  The values are checked on the GPU (tests/test_constrained_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import (AcquisitionProduct, AcquisitionQuotient, CausalExpectedImprovement,
                                              CausalGradientAcquisitionOptimizer, Cost, IntegratedVarianceReduction,
                                              MaxValueEntropySearch, ProbabilityOfFeasibility, find_next_y_point)
from cbo_with_oop_amd.utils_functions.causal_optimizer import _numerator, _values_and_gradients, has_gradients


class Untouchable:
    """Construction must not touch the model (emukit's __init__ only stores it)."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was asked for {name!r}")


def test_entry_point_is_declared_exported_and_prototyped():
    text = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"#define\s+CBO_HIP_ABI_VERSION\s+5\b", text)
    assert re.search(r"#define\s+CBO_MAX_CONSTRAINTS\s+8\b", text)
    assert re.search(r"CBO_CON_LE\s*=\s*0\s*,\s*CBO_CON_GE\s*=\s*1", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+cbo_acq_sweep_constrained\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl, "cbo_acq_sweep_constrained not declared in include/cbo_hip.h"
    assert len(decl.group(1).split(",")) == 17
    assert hasattr(_lib.load(), "cbo_acq_sweep_constrained"), "not exported by libcbo_hip.so"
    restype, argtypes = _lib.SIGNATURES["cbo_acq_sweep_constrained"]
    assert restype is ctypes.c_int and len(argtypes) == 17
    assert argtypes[6] is ctypes.c_int and argtypes[7] is _lib.c_void_pp and argtypes[8] is _lib.c_void_pp
    assert argtypes[11] is _lib.c_int_p and argtypes[16] is _lib.c_int64_p
    assert _lib.ABI_VERSION == 5 and _lib.load().cbo_abi_version() == 5


def test_invalid_arguments_are_refused_before_any_device_work():
    """What can be refused without a context: the count, a lone gp / cands, no objective and no constraint."""
    lib = _lib.load()
    call = lambda n_con: lib.cbo_acq_sweep_constrained(None, None, 0.0, 0, 0.0, 1.0, n_con, None, None, None, None, None,
                                                       None, None, None, None, None)
    for n_con in (-1, 9, 0, 1):
        assert call(n_con) == _lib.CBO_ERR_INVALID


def test_classes_have_emukits_signature_and_defaults():
    params = inspect.signature(ProbabilityOfFeasibility.__init__).parameters
    assert list(params) == ["self", "model", "jitter", "max_value", "sense"]
    assert params["jitter"].default == 0.0 and params["max_value"].default == 0.0
    assert params["sense"].default == "<=" and params["sense"].kind is inspect.Parameter.KEYWORD_ONLY
    model = Untouchable()
    pof = ProbabilityOfFeasibility(model)
    assert pof.model is model and pof.jitter == 0.0 and pof.max_value == 0.0 and pof.sense == "<="
    assert ProbabilityOfFeasibility(model, 0.1, 2.0, sense=">=").sense == ">="
    assert pof.has_gradients is True
    with pytest.raises(ValueError):
        ProbabilityOfFeasibility(model, sense="<")
    params = inspect.signature(ProbabilityOfFeasibility.sweep).parameters
    assert list(params) == ["self", "candidates", "cost", "want_acq"] and params["cost"].default == 1.0
    params = inspect.signature(AcquisitionProduct.sweep).parameters
    assert list(params) == ["self", "candidates", "cost", "want_acq", "want_terms"]
    assert params["cost"].default == 1.0 and params["want_acq"].default is False and params["want_terms"].default is False
    assert list(inspect.signature(find_next_y_point).parameters)[-1] == "constraints"
    assert inspect.signature(find_next_y_point).parameters["constraints"].default is None


def test_products_flatten_into_one_objective_and_its_constraints_in_order():
    m0, m1, m2, m3 = (Untouchable() for _ in range(4))
    ei = CausalExpectedImprovement(0.5, "min", m0)
    a, b, c = (ProbabilityOfFeasibility(m, max_value=v) for m, v in ((m1, 1.0), (m2, 2.0), (m3, 3.0)))
    p = ei * a * b
    assert isinstance(p, AcquisitionProduct) and p.objective is ei and p.constraints == [a, b] and p.factors == [ei, a, b]
    assert p.model is m0 and p.has_gradients
    assert (ei * (a * b) * c).factors == [ei, a, b, c]
    assert ((a * b) * (ei * c)).factors == [ei, a, b, c]        # the objective leads, the constraints keep their order
    q = a * b
    assert q.objective is None and q.factors == [a, b] and q.model is m1
    cost = Cost({"X": lambda col: 2.0}, ["X"])
    quot = p / cost
    assert isinstance(quot, AcquisitionQuotient) and quot.numerator is p and quot.denominator is cost and quot.model is m0
    assert isinstance(a / cost, AcquisitionQuotient) and (a / cost).numerator.factors == [a]
    assert _numerator(quot) is p and has_gradients(quot)


def test_products_without_a_device_pass_are_refused():
    m = Untouchable()
    ei = CausalExpectedImprovement(0.5, "min", m)
    pof = ProbabilityOfFeasibility(m)
    with pytest.raises(ValueError):
        ei * ei
    with pytest.raises(ValueError):
        (ei * pof) * CausalExpectedImprovement(0.1, "min", m)
    with pytest.raises(ValueError):
        pof * IntegratedVarianceReduction.__new__(IntegratedVarianceReduction)
    with pytest.raises(ValueError):
        ei * MaxValueEntropySearch.__new__(MaxValueEntropySearch)
    with pytest.raises(ValueError):
        AcquisitionProduct([pof] * 9)
    from cbo_with_oop_amd.utils_functions.causal_acquisition_functions import CandidateGrid
    grid = CandidateGrid.__new__(CandidateGrid)
    with pytest.raises(ValueError):
        (ei * pof).sweep([grid])                                    # one grid for two factors


def test_find_next_y_point_refuses_mes_and_uniform_anchors_with_constraints():
    m = Untouchable()
    cons = [ProbabilityOfFeasibility(m)]
    costs = {"X": lambda col: 1.0}
    with pytest.raises(ValueError):
        find_next_y_point([(0.0, 1.0)], m, 0.0, ["X"], costs, acquisition="MES", constraints=cons)
    with pytest.raises(ValueError):
        find_next_y_point([(0.0, 1.0)], m, 0.0, ["X"], costs, anchors="uniform", constraints=cons)


# ---- gradients against central finite differences --------------------------------------------------------------------
# Closed-form stub models in the variable t = w . x.  Bounds of |phi|, |phi'|, |phi''| of the standard normal density:
# phi(0) = 0.39895, |phi'| = |u| phi <= phi(1) = 0.24198, |phi''| = |u^2 - 1| phi <= phi(0).
P0, P1, P2 = 0.39895, 0.24198, 0.39895
H = 1e-6


class PofStub:
    """sd(x) = c + b sin(w2 . x) and mean(x) = value - jitter - sd(x) g(x) with g = B sin(w . x): then the standardised
    distance u = (value - (mean + jitter)) / sd IS g(x), and the probability of feasibility is Phi(B sin t).  The variance
    varies, so both terms of the gradient (dmean/dx and u dsd/dx) are exercised."""

    def __init__(self, w, w2, B, value, jitter, c=1.5, b=0.5):
        self.w, self.w2, self.B, self.value, self.jitter, self.c, self.b = np.asarray(w), np.asarray(w2), B, value, jitter, c, b

    def _parts(self, x):
        t, t2 = x @ self.w, x @ self.w2
        sd, g = self.c + self.b * np.sin(t2), self.B * np.sin(t)
        dsd = self.b * np.cos(t2)[:, None] * self.w2[None, :]
        dg = self.B * np.cos(t)[:, None] * self.w[None, :]
        return sd, g, dsd, dg

    def predict(self, x):
        sd, g, _, _ = self._parts(x)
        return (self.value - self.jitter - sd * g)[:, None], (sd * sd)[:, None]

    def get_prediction_gradients(self, x):
        sd, g, dsd, dg = self._parts(x)
        return -(dsd * g[:, None] + sd[:, None] * dg), 2 * sd[:, None] * dsd

    def derivative_bounds(self, k):
        """(|f|, |f'|, |f''|, |f'''|) bounds of f = Phi(g), g = B sin t, along coordinate k (dt/dx_k = w_k):
        f' = phi g', f'' = phi' g'^2 + phi g'', f''' = phi'' g'^3 + 3 phi' g' g'' + phi g''' with |g^(j)| <= B |w_k|^j."""
        B, w = self.B, abs(self.w[k])
        return (1.0, P0 * B * w, (P1 * B * B + P0 * B) * w ** 2, (P2 * B ** 3 + 3 * P1 * B * B + P0 * B) * w ** 3)


class EiStub:
    """Constant sd = s, mean(x) = A sin(w . x): EI = s E(u), E(u) = u Phi(u) + phi(u), u = (y_best - mean) / s."""

    def __init__(self, w, A, s):
        self.w, self.A, self.s = np.asarray(w), A, s

    def predict(self, x):
        t = x @ self.w
        return (self.A * np.sin(t))[:, None], np.full((x.shape[0], 1), self.s * self.s)

    def get_prediction_gradients(self, x):
        t = x @ self.w
        return self.A * np.cos(t)[:, None] * self.w[None, :], np.zeros(x.shape)

    def derivative_bounds(self, k, y_best):
        """E' = Phi <= 1, E'' = phi, E''' = phi'; |u^(j)| <= a |w_k|^j with a = A / s, |u| <= |y_best| / s + a,
        E(u) <= |u| + phi(0):  f''' = s (E''' u'^3 + 3 E'' u' u'' + E' u''')."""
        a, w, s = self.A / self.s, abs(self.w[k]), self.s
        return (s * (abs(y_best) / s + a + P0), s * a * w, s * (P0 * a * a + a) * w ** 2,
                s * (P1 * a ** 3 + 3 * P0 * a * a + a) * w ** 3)


def product_bounds(a, b):
    """Leibniz: bounds of (fg), (fg)', (fg)'', (fg)''' from those of f and g."""
    return (a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[0] * b[2] + 2 * a[1] * b[1] + a[2] * b[0],
            a[0] * b[3] + 3 * a[1] * b[2] + 3 * a[2] * b[1] + a[3] * b[0])


def central_differences(acq, X, k):
    e = np.zeros(X.shape[1])
    e[k] = H
    return (acq.evaluate_with_gradients(X + e)[0][:, 0] - acq.evaluate_with_gradients(X - e)[0][:, 0]) / (2 * H)


POINTS = np.random.default_rng(11).uniform(-1.0, 1.0, (64, 2))


@pytest.mark.parametrize("sense", ["<=", ">="])
def test_probability_of_feasibility_gradients_agree_with_central_differences(sense):
    """h = 1e-6; the tolerance is the truncation bound h^2 max|f'''| of the stub (the central difference's own error is
    h^2 |f'''| / 6; its rounding, eps |f| / h = 2e-10, lies below the bound for this stub, whose w makes f''' of the
    order of a thousand).  The bound is derived in PofStub.derivative_bounds, not measured."""
    stub = PofStub(w=[6.0, -5.0], w2=[1.0, 2.0], B=2.0, value=0.7, jitter=0.2)
    pof = ProbabilityOfFeasibility(stub, 0.2, 0.7, sense=sense)
    f, df = pof.evaluate_with_gradients(POINTS)
    assert f.shape == (64, 1) and df.shape == (64, 2)
    import scipy.stats
    g = 2.0 * np.sin(POINTS @ stub.w)
    np.testing.assert_allclose(f[:, 0], scipy.stats.norm.cdf(g if sense == "<=" else -g), rtol=0, atol=1e-14)
    assert f.min() < 0.2 and f.max() > 0.8                         # the stub is not a flat function
    for k in range(2):
        tol = H * H * stub.derivative_bounds(k)[3]
        err = np.abs(df[:, k] - central_differences(pof, POINTS, k))
        print(f"pof {sense} d/dx{k}: worst {err.max():.3e}, tolerance {tol:.3e}")
        assert np.all(err <= tol), (k, err.max(), tol)
        assert np.abs(df[:, k]).max() > 1e4 * tol                 # the comparison resolves the gradient


def test_product_gradients_agree_with_central_differences():
    """EI * PoF * PoF (one '<=', one '>=') over a cost: the product rule on the host against central differences, h = 1e-6,
    tolerance h^2 max|f'''| with the bound composed by Leibniz' rule from the factors' own (derivative_bounds)."""
    y_best = 0.3
    obj = EiStub(w=[4.0, 3.0], A=1.2, s=0.8)
    s1 = PofStub(w=[6.0, -5.0], w2=[1.0, 2.0], B=2.0, value=0.7, jitter=0.2)
    s2 = PofStub(w=[-3.0, 7.0], w2=[2.0, -1.0], B=1.5, value=-0.4, jitter=0.0)
    prod = (CausalExpectedImprovement(y_best, "min", obj) * ProbabilityOfFeasibility(s1, 0.2, 0.7)
            * ProbabilityOfFeasibility(s2, 0.0, -0.4, sense=">="))
    f, df = prod.evaluate_with_gradients(POINTS)
    parts = [fac.evaluate_with_gradients(POINTS)[0] for fac in prod.factors]
    np.testing.assert_array_equal(f, (parts[0] * parts[1]) * parts[2])
    for k in range(2):
        bounds = product_bounds(product_bounds(obj.derivative_bounds(k, y_best), s1.derivative_bounds(k)),
                                s2.derivative_bounds(k))
        tol = H * H * bounds[3]
        err = np.abs(df[:, k] - central_differences(prod, POINTS, k))
        print(f"product d/dx{k}: worst {err.max():.3e}, tolerance {tol:.3e}")
        assert np.all(err <= tol), (k, err.max(), tol)
        assert np.abs(df[:, k]).max() > 1e3 * tol
    # under a cost: the quotient rule of AcquisitionQuotient and the optimiser's batched form
    quot = prod / Cost({"a": lambda col: 1.5, "b": lambda col: 0.5}, ["a", "b"])
    fq, dfq = quot.evaluate_with_gradients(POINTS)
    np.testing.assert_array_equal(fq, f / 2.0)
    np.testing.assert_array_equal(dfq, df / 2.0)
    vals, grads = _values_and_gradients(quot, POINTS)
    np.testing.assert_array_equal(vals, f[:, 0] / 2.0)
    np.testing.assert_array_equal(grads, df / 2.0)
    assert isinstance(CausalGradientAcquisitionOptimizer([(-1.0, 1.0)] * 2), CausalGradientAcquisitionOptimizer)
