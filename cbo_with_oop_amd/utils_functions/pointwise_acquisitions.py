"""Point-wise acquisitions on the MI355X path: lower confidence bound, probability of improvement, mean-plug-in Expected
Improvement and model variance, each over a candidate grid in ONE device call with the arg-max (``cbo_acq_sweep_kind``,
include/cbo_hip.h; kernels_pointwise.hip).

emukit is not installed here: the classes restate emukit 0.4's
``emukit.bayesian_optimization.acquisitions.NegativeLowerConfidenceBound``, ``ProbabilityOfImprovement`` and
``MeanPluginExpectedImprovement`` and ``emukit.experimental_design.acquisitions.ModelVariance`` from memory, and parity is
unpinned.  ``task`` is this package's addition, as for ``CausalExpectedImprovement``: ``'max'`` mirrors the
formula (upper confidence bound, ``cdf(-u)``, the maximum of the means).

Posterior mean and variance are ``model.predict``'s (likelihood noise included), bit for bit.

``CausalLogExpectedImprovement`` (``cbo_acq_sweep_logei``) is the logarithm of the causal EI computed without
underflow: a strict order and a gradient where the EI itself is an exact 0.0.  Its quotient with a ``Cost`` is
``LogAcquisitionQuotient``, ``log EI - log cost``.
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


_LOG_SQRT_2PI = 0.918938533204672741780      # log sqrt(2 pi)
_LOG_SQRT_HALF_PI = 0.225791352644727432363  # log sqrt(pi / 2)
_SQRT_HALF_PI = 1.25331413731550025121       # sqrt(pi / 2)
_LOGEI_SERIES = (-3.0, 15.0, -105.0, 945.0, -10395.0, 135135.0, -2027025.0, 34459425.0)   # (-1)^k (2k + 1)!!


def _log_h_parts(u):
    """(log h, A, B) for ``h(u) = pdf(u) + u cdf(u)``, ``A = cdf / h``, ``B = pdf / h``: the device's ``log_h_of`` (cbo_device.h,
    DESIGN.md §4x) in numpy with scipy's ``ndtr`` and ``erfcx``, range by range."""
    import scipy.special as sp
    u = np.asarray(u, dtype=np.float64)
    shape, u = u.shape, u.reshape(-1)
    log_h, a, b = np.full(u.shape, np.nan), np.full(u.shape, np.nan), np.full(u.shape, np.nan)
    with np.errstate(all="ignore"):
        near = u > -1.0
        un = u[near]
        pdf, cdf = np.exp(-(un * un) / 2.0) * 0.3989422804014327, sp.ndtr(un)
        h = pdf + un * cdf
        log_h[near], a[near], b[near] = np.log(h), cdf / h, pdf / h
        mid = (u <= -1.0) & (u > -30.0)
        um = u[mid]
        erfcx = sp.erfcx(-um * 7.07106781186547524401E-1)
        x = np.log(erfcx * -um) + _LOG_SQRT_HALF_PI                   # log w, w = 1 - h / pdf
        w = np.exp(x)
        close = x > -0.693147180559945309417
        one_minus_w = np.where(close, -np.expm1(x), 1.0 - w)
        log_h[mid] = (-(um * um) / 2.0 - _LOG_SQRT_2PI) + np.where(close, np.log(one_minus_w), np.log1p(-w))
        # A and B: 1 / (1 - w) down to u = -1.5, where the cancellation in 1 - w (w = 0.77 there) still leaves them good to
        # 2e-15; below, the Mills ratio's continued fraction R(t) = 1 / (t + 1 / (t + 2 / (t + ...))), t = -u, evaluated
        # from its 224th term backwards (every step contracts the error; the truncation, ~exp(-1.7 t sqrt N), is below 1e-16 from
        # t = 1.5 on): with
        # K = 1 / (t + 2 / (t + 3 / ...)),  h / pdf = K / (t + K),  B = (t + K) / K,  A = 1 / K -- no cancellation anywhere.
        # (The device forms B = 1 / (1 - w) in the whole range: 5e-13 relative at u = -30, far inside what a search needs.)
        t = -um
        k_cf = np.zeros(um.shape)
        for k in range(224, 0, -1):
            k_cf = k / (t + k_cf)
        cf = um <= -1.5
        b[mid] = np.where(cf, (t + k_cf) / k_cf, 1.0 / one_minus_w)
        a[mid] = np.where(cf, 1.0 / k_cf, _SQRT_HALF_PI * erfcx * b[mid])
        far = u <= -30.0
        uf = u[far]
        u2 = uf * uf
        t = 1.0 / u2
        series = np.full(uf.shape, _LOGEI_SERIES[-1])
        for c in _LOGEI_SERIES[-2::-1]:
            series = series * t + c
        series = series * t
        log_h[far] = ((-u2 / 2.0 - _LOG_SQRT_2PI) - 2.0 * np.log(-uf)) + np.log1p(series)
        b[far] = u2 / (1.0 + series)
        a[far] = _SQRT_HALF_PI * sp.erfcx(-uf * 7.07106781186547524401E-1) * b[far]
    return log_h.reshape(shape), a.reshape(shape), b.reshape(shape)


class CausalLogExpectedImprovement(_PointwiseAcquisition):
    """The logarithm of the Expected Improvement, computed without underflow (Ament et al. 2023, "Unexpected improvements to
    expected improvement"; BoTorch's ``LogExpectedImprovement``): ``log h(u) + log sd`` with ``h(u) = pdf(u) + u cdf(u)`` and
    ``u = (y_best - (mean + jitter)) / sd`` (``cbo_acq_sweep_logei``).  Where the EI is an exact 0.0 in double
    precision -- ``u < -38.6``: most of a grid once a noise-free model has a few dozen observations -- this is still finite,
    strictly ordered and has a gradient; where the EI is representable its arg-max is the same.

    ``task='max'`` is the MIRROR, ``u = ((mean - jitter) - y_best) / sd`` -- the improvement of a maximiser.  It is not the
    logarithm of ``CausalExpectedImprovement``'s ``'max'`` value: that is the reference's ``-EI`` with the minimiser's ``u``, a
    negative number, which has no logarithm.

    ``acquisition / Cost(...)`` is ``log EI - log cost`` (``LogAcquisitionQuotient``): the logarithm of the quotient."""
    kind = _lib.LOGEI

    def __init__(self, current_global_min, task, model, jitter=0.0):
        self.current_global_min = current_global_min
        self.task = _task(task)
        self.model = model
        self.jitter = _finite(jitter, "jitter")

    def _scalars(self):
        return _finite(self.current_global_min, "current_global_min"), self.task, self.jitter

    @staticmethod
    def standardised(mean, sd, y_best, task="min", jitter=0.0):
        """u of the formula above."""
        mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
        if _task(task) == "min":
            return (y_best - (mean + jitter)) / sd
        return ((mean - jitter) - y_best) / sd

    @staticmethod
    def log_h(u):
        """``log(pdf(u) + u cdf(u))`` in the device's three ranges."""
        return _log_h_parts(u)[0]

    @staticmethod
    def gradient_coefficients(u):
        """``(A, B) = (cdf / h, pdf / h)``: ``d logEI = (-A d mean + B d sd) / sd`` (``d mean``'s sign flipped for ``'max'``)."""
        return _log_h_parts(u)[1:]

    @staticmethod
    def log_ei(mean, sd, y_best, task="min", jitter=0.0):
        """The device formula in numpy / scipy (the host reference; cost 1): ``log h(u) + log sd``."""
        u = CausalLogExpectedImprovement.standardised(mean, sd, y_best, task, jitter)
        with np.errstate(all="ignore"):
            return _log_h_parts(u)[0] + np.log(np.asarray(sd, dtype=np.float64))

    def sweep(self, candidates, cost=1.0, want_acq=False, want_posterior=False):
        """``_PointwiseAcquisition.sweep`` through ``cbo_acq_sweep_logei``: ``acq`` is ``log EI - log cost``."""
        y_best, task, jitter = self._scalars()
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
            _lib.check(_lib.load().cbo_acq_sweep_logei(
                self.model._handle, grid._handle, y_best, _lib.TASK_CODE[task], jitter, float(cost), _lib.dptr(acq),
                _lib.dptr(mean), _lib.dptr(var), ctypes.byref(best_val), ctypes.byref(best_idx)))
        finally:
            if own:
                grid.close()
        col = lambda a: None if a is None else a[:, None]      # noqa: E731
        return {"best_val": best_val.value, "best_idx": best_idx.value, "acq": col(acq), "mean": col(mean),
                "var": col(var)}

    def sweep_batch(self, candidates, batch_size, cost=1.0, update_incumbent=False, want_acq=False, want_posterior=False):
        """Greedy batch selection (the Kriging believer) on the log EI in ONE device call (``cbo_acq_sweep_batch_logei``,
        DESIGN.md §4ad): ``CausalExpectedImprovement.sweep_batch``'s picks, its arguments and its result dictionary, every
        pick scored by ``log EI - log cost`` -- finite and ordered where the EI of every pick is an exact 0.0 and the EI
        form returns candidate 0 ``batch_size`` times.  Pick 0 is ``sweep``'s result, bit for bit."""
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f"batch_size must be a positive int, not {batch_size!r}")
        batch_size = int(batch_size)
        y_best, task, jitter = self._scalars()
        own = not isinstance(candidates, CandidateGrid)
        grid = CandidateGrid(candidates, self.model) if own else candidates
        m = len(grid)
        acq = np.empty(m) if want_acq else None
        mean = np.empty(m) if want_posterior else None
        var = np.empty(m) if want_posterior else None
        best_vals = np.empty(batch_size)
        best_idxs = np.empty(batch_size, dtype=np.int64)
        try:
            self.model.ensure_fitted()
            _lib.check(_lib.load().cbo_acq_sweep_batch_logei(
                self.model._handle, grid._handle, y_best, _lib.TASK_CODE[task], jitter, float(cost), batch_size,
                int(bool(update_incumbent)), _lib.dptr(best_vals), best_idxs.ctypes.data_as(_lib.c_int64_p), _lib.dptr(acq),
                _lib.dptr(mean), _lib.dptr(var)))
        finally:
            if own:
                grid.close()
        col = lambda a: None if a is None else a[:, None]      # noqa: E731
        return {"best_val": best_vals, "best_idx": best_idxs, "acq": col(acq), "mean": col(mean), "var": col(var)}

    def evaluate_with_gradients(self, x):
        """(log EI (M,1), d log EI / d x (M,d)): posterior and its gradients from the device, ``A`` and ``B`` on the host."""
        x = _lib.as_f64(x)
        mean, standard_deviation, dmean_dx, dstandard_deviation_dx = self._posterior_and_gradients(x)
        y_best, task, jitter = self._scalars()
        u = self.standardised(mean, standard_deviation, y_best, task, jitter)
        log_h, a, b = _log_h_parts(u)
        sign = 1.0 if task == "min" else -1.0
        gradient = (-sign * a * dmean_dx + b * dstandard_deviation_dx) / standard_deviation
        return log_h + np.log(standard_deviation), gradient

    def __truediv__(self, cost):
        from .cost_functions import PointwiseCost
        if isinstance(cost, PointwiseCost):              # (every candidate over its own cost)
            from .causal_acquisition_functions import PointCostQuotient
            return PointCostQuotient(self, cost)
        return LogAcquisitionQuotient(self, cost)


class LogAcquisitionQuotient(AcquisitionQuotient):
    """``CausalLogExpectedImprovement(...) / Cost(...)``: the logarithm of the quotient, ``log EI - log cost``.  ``sweep`` hands
    the cost to the device call as ``AcquisitionQuotient`` does (the call subtracts its logarithm), and so does
    ``sweep_batch`` (inherited); with the reference's zero cost gradient the gradient is ``d log EI`` itself."""
    is_log = True

    def evaluate_with_gradients(self, x):
        x = _lib.as_f64(x)
        f, df = self.numerator.evaluate_with_gradients(x)
        return f - math.log(float(self.denominator.evaluate(x))), df


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
