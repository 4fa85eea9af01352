"""Point-wise acquisitions on the MI355X path: lower confidence bound, probability of improvement, mean-plug-in Expected
Improvement and model variance, each over a candidate grid in ONE device call with the arg-max (``cbo_acq_sweep_kind``,
include/cbo_hip.h; kernels_pointwise.hip).

emukit is not installed here: the classes restate emukit 0.4's
``emukit.bayesian_optimization.acquisitions.NegativeLowerConfidenceBound``, ``ProbabilityOfImprovement`` and
``MeanPluginExpectedImprovement`` and ``emukit.experimental_design.acquisitions.ModelVariance`` from memory, and parity is
unpinned.  ``task`` is this package's addition, as for ``CausalExpectedImprovement``: ``'max'`` mirrors the
formula (upper confidence bound, ``cdf(-u)``, the maximum of the means).

Posterior mean and variance are ``model.predict``'s (likelihood noise included), bit for bit.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from .. import _lib
from .causal_acquisition_functions import AcquisitionQuotient, CandidateGrid, CausalExpectedImprovement


def _finite(value, what):
    try:
        value = float(np.asarray(value, dtype=np.float64).reshape(-1)[0])
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"{what} must be a finite number, not {value!r}") from None
    if not math.isfinite(value):
        raise ValueError(f"{what} must be a finite number, not {value!r}")
    return value


def _task(task):
    if task not in _lib.TASK_CODE:
        raise ValueError(f"task must be 'min' or 'max', not {task!r}")
    return task


class _PointwiseAcquisition:
    """What the four classes share: the device sweep, ``evaluate`` and the quotient with a ``Cost``.  A subclass names its
    kind and supplies ``_scalars() -> (y_best, task, param)`` and ``evaluate_with_gradients``."""
    kind = None
    has_gradients = True

    def _scalars(self):
        raise NotImplementedError

    def sweep(self, candidates, cost=1.0, want_acq=False, want_posterior=False):
        """Score every candidate and pick the best: dict(best_val, best_idx, acq, mean, var), as
        ``CausalExpectedImprovement.sweep``.  ``candidates`` is a CandidateGrid (device resident) or an (M,d) array."""
        y_best, task, param = self._scalars()
        own = not isinstance(candidates, CandidateGrid)
        grid = CandidateGrid(candidates, self.model) if own else candidates
        m = len(grid)
        acq = np.empty(m) if want_acq else None
        mean = np.empty(m) if want_posterior else None
        var = np.empty(m) if want_posterior else None
        best_val = ctypes.c_double(0.0)
        best_idx = ctypes.c_int64(-1)
        try:
            self.model.ensure_fitted()
            _lib.check(_lib.load().cbo_acq_sweep_kind(
                self.model._handle, grid._handle, _lib.ACQ_KIND_CODE[self.kind], y_best, _lib.TASK_CODE[task], param,
                float(cost), _lib.dptr(acq), _lib.dptr(mean), _lib.dptr(var), ctypes.byref(best_val),
                ctypes.byref(best_idx)))
        finally:
            if own:
                grid.close()
        col = lambda a: None if a is None else a[:, None]      # noqa: E731
        return {"best_val": best_val.value, "best_idx": best_idx.value, "acq": col(acq), "mean": col(mean),
                "var": col(var)}

    def evaluate(self, x):
        """(M,1) acquisition values: emukit's ``evaluate``."""
        return self.sweep(_lib.as_f64(x), cost=1.0, want_acq=True)["acq"]

    def _posterior_and_gradients(self, x):
        """(mean, sd, dmean/dx, dsd/dx) at x from the device, as emukit's ``evaluate_with_gradients`` start."""
        mean, variance = self.model.predict(x)
        standard_deviation = np.sqrt(variance)
        dmean_dx, dvariance_dx = self.model.get_prediction_gradients(x)
        return mean, standard_deviation, dmean_dx, dvariance_dx / (2 * standard_deviation)

    def __truediv__(self, cost):
        """``acquisition / Cost(...)``: the existing AcquisitionQuotient (the cost divides inside the device call)."""
        return AcquisitionQuotient(self, cost)


class CausalNegativeLowerConfidenceBound(_PointwiseAcquisition):
    """emukit ``NegativeLowerConfidenceBound``: ``-(mean - beta * sd)`` (task ``'min'``), ``mean + beta * sd`` -- the upper
    confidence bound -- for ``'max'``.  Restated from memory, parity unpinned.

    Caveat: the value can be negative, and a quotient with a ``Cost`` divides it by the cost all the same, as emukit's
    ``Quotient`` does.  Among negative values the division then FAVOURS the costly intervention (-1 / 10 > -1 / 1).  This
    restates emukit and is not "fixed" here."""
    kind = "LCB"

    def __init__(self, task, model, beta=1.0):
        self.task = _task(task)
        self.model = model
        self.beta = _finite(beta, "beta")
        if self.beta < 0.0:
            raise ValueError(f"beta must not be negative, not {beta!r}")

    def _scalars(self):
        return 0.0, self.task, self.beta

    def evaluate_with_gradients(self, x):
        """(value (M,1), gradient (M,d)): emukit's ``lcb = -(mean - beta sd)``, ``dlcb/dx = -(dmean/dx - beta dsd/dx)``;
        posterior and gradients from the device, the closing arithmetic in numpy."""
        x = _lib.as_f64(x)
        mean, standard_deviation, dmean_dx, dstandard_deviation_dx = self._posterior_and_gradients(x)
        if self.task == "min":
            return -(mean - self.beta * standard_deviation), -(dmean_dx - self.beta * dstandard_deviation_dx)
        return mean + self.beta * standard_deviation, dmean_dx + self.beta * dstandard_deviation_dx


class CausalProbabilityOfImprovement(_PointwiseAcquisition):
    """emukit ``ProbabilityOfImprovement``: ``cdf((y_best - (mean + jitter)) / sd)`` (task ``'min'``), ``cdf`` of the negated
    argument for ``'max'``.  ``current_global_min`` is the incumbent, as for ``CausalExpectedImprovement``.  Restated from
    memory, parity unpinned."""
    kind = "PI"

    def __init__(self, current_global_min, task, model, jitter=0.0):
        self.current_global_min = current_global_min
        self.task = _task(task)
        self.model = model
        self.jitter = _finite(jitter, "jitter")

    def _scalars(self):
        return _finite(self.current_global_min, "current_global_min"), self.task, self.jitter

    def evaluate_with_gradients(self, x):
        """(value (M,1), gradient (M,d)): emukit's ``dcdf/dx = -pdf(u) (dmean/dx + u dsd/dx) / sd``, the sign flipped for
        ``'max'``."""
        import scipy.stats
        x = _lib.as_f64(x)
        mean, standard_deviation, dmean_dx, dstandard_deviation_dx = self._posterior_and_gradients(x)
        mean = mean + self.jitter
        u = (_finite(self.current_global_min, "current_global_min") - mean) / standard_deviation
        dcdf_dx = -scipy.stats.norm.pdf(u) * (dmean_dx + u * dstandard_deviation_dx) / standard_deviation
        if self.task == "min":
            return scipy.stats.norm.cdf(u), dcdf_dx
        return scipy.stats.norm.cdf(-u), -dcdf_dx


class CausalMeanPluginExpectedImprovement(_PointwiseAcquisition):
    """emukit ``MeanPluginExpectedImprovement``: the Expected Improvement whose incumbent is the best posterior MEAN at the
    model's own inputs, ``min(model.predict(model.X)[0])`` (``max`` for task ``'max'``) -- the EI that is correct for a model
    with observation noise.  The incumbent is formed and consumed on the device.  Restated from memory, parity unpinned."""
    kind = "MPEI"

    def __init__(self, task, model, jitter=0.0):
        self.task = _task(task)
        self.model = model
        self.jitter = _finite(jitter, "jitter")

    def _scalars(self):
        return 0.0, self.task, self.jitter

    def incumbent(self):
        """The plug-in incumbent (``cbo_gp_plugin_incumbent``): ``model.predict(model.X)[0]``'s min or max, bit for bit."""
        out = ctypes.c_double(0.0)
        self.model.ensure_fitted()
        _lib.check(_lib.load().cbo_gp_plugin_incumbent(self.model._handle, _lib.TASK_CODE[self.task], ctypes.byref(out)))
        return out.value

    def evaluate_with_gradients(self, x):
        """(improvement (M,1), gradient (M,d)): ``CausalExpectedImprovement``'s formulas with the plug-in incumbent held
        constant, as emukit has it."""
        return CausalExpectedImprovement(self.incumbent(), self.task, self.model,
                                         self.jitter).evaluate_with_gradients(x)


class ModelVariance(_PointwiseAcquisition):
    """emukit ``ModelVariance`` (experimental design, uncertainty sampling): the predictive variance.  Restated from memory,
    parity unpinned."""
    kind = "VAR"

    def __init__(self, model):
        self.model = model

    def _scalars(self):
        return 0.0, "min", 0.0

    def evaluate_with_gradients(self, x):
        """(variance (M,1), d variance / d x (M,d)), both from the device."""
        x = _lib.as_f64(x)
        _, variance = self.model.predict(x)
        _, dvariance_dx = self.model.get_prediction_gradients(x)
        return variance, dvariance_dx
