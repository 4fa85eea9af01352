"""emukit's integrated variance reduction on the MI355X path.

emukit 0.4's ``emukit.experimental_design.acquisitions.IntegratedVarianceReduction`` scores a candidate x by the mean,
over Monte-Carlo integration points drawn uniformly from the space, of the model's
``calculate_variance_reduction(x, X_mc) = cov(x, X_mc)^2 / var(x)``, one model call per candidate.  Here every candidate
goes to the device in one call (``cbo_gp_integrated_variance_reduction``, include/cbo_hip.h): the covariance with the
integration points is squared and summed inside the product and never stored, and the arg-max is taken there too.
emukit is not installed here: the class restates emukit 0.4 from memory, and parity is unpinned.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib
from ..GaussianProcessFactory import _column
from .causal_acquisition_functions import AcquisitionQuotient, CandidateGrid
from .causal_optimizer import sample_uniform


class IntegratedVarianceReduction:
    def __init__(self, model, space, x_monte_carlo=None, num_monte_carlo_points=int(1e5)):
        """emukit's signature.  ``space``: an emukit ParameterSpace or a list of (lo, hi), as ``space_bounds`` accepts.
        Without ``x_monte_carlo``, ``num_monte_carlo_points`` integration points are drawn as emukit's
        ``space.sample_uniform`` draws them, from numpy's global generator (``sample_uniform``); a supplied
        ``x_monte_carlo`` outside the space raises ``ValueError``.  Restated from memory, parity unpinned."""
        from .utils import space_bounds
        self.model = model
        self.space = space
        self.bounds = space_bounds(space)
        if x_monte_carlo is None:
            self._x_monte_carlo = sample_uniform(self.bounds, int(num_monte_carlo_points))
        else:
            x = np.asarray(x_monte_carlo, dtype=np.float64)
            if x.ndim != 2 or x.shape[1] != len(self.bounds):
                raise ValueError(f"x_monte_carlo must be (N, {len(self.bounds)})")
            lo = np.array([b[0] for b in self.bounds], dtype=np.float64)
            hi = np.array([b[1] for b in self.bounds], dtype=np.float64)
            if not np.all((lo <= x) & (x <= hi)):
                raise ValueError("Some or all of the points in x_monte_carlo are out of the valid domain.")
            self._x_monte_carlo = x
        self._prior_int = None       # causal models: v(X_mc), evaluated on first use

    def _integration_points(self):
        x = _lib.as_f64(self._x_monte_carlo)
        pv = None
        if self.model.causal:
            if self._prior_int is None:
                self._prior_int = _column(self.model.variance_adjustment(x), x.shape[0], "variance_adjustment")
            pv = self._prior_int
        return x, pv

    def sweep(self, candidates, cost=1.0, want_acq=False):
        """Score every candidate and pick the best, as ``CausalExpectedImprovement.sweep``: returns dict(best_val,
        best_idx, acq, mean, var), mean and var None.  ``candidates`` is a CandidateGrid or an (M,d) array; the value is
        emukit's ``evaluate`` divided by ``cost``."""
        pts = candidates.points if isinstance(candidates, CandidateGrid) else candidates
        x = _lib.as_f64(pts)
        if x.ndim != 2 or x.shape[1] != len(self.bounds):
            raise ValueError(f"candidates must be (M, {len(self.bounds)})")
        m = x.shape[0]
        pv = _column(self.model.variance_adjustment(x), m, "variance_adjustment") if self.model.causal else None
        xi, pvi = self._integration_points()
        acq = np.empty(m) if want_acq else None
        best_val = ctypes.c_double(0.0)
        best_idx = ctypes.c_int64(-1)
        self.model.ensure_fitted()
        _lib.check(_lib.load().cbo_gp_integrated_variance_reduction(
            self.model._handle, m, _lib.dptr(x), _lib.dptr(pv), xi.shape[0], _lib.dptr(xi), _lib.dptr(pvi), float(cost),
            _lib.dptr(acq), ctypes.byref(best_val), ctypes.byref(best_idx)))
        return {"best_val": best_val.value, "best_idx": best_idx.value, "acq": None if acq is None else acq[:, None],
                "mean": None, "var": None}

    def evaluate(self, x):
        """(M,1): ``np.mean(model.calculate_variance_reduction(x[[i]], x_monte_carlo))`` for every row, in one device
        call.  Restated from memory, parity unpinned."""
        return self.sweep(x, want_acq=True)["acq"]

    @property
    def has_gradients(self):
        return False

    def __truediv__(self, cost):
        """``IntegratedVarianceReduction(...) / Cost(...)``: emukit's Quotient, here the existing AcquisitionQuotient (the
        cost divides inside the device call)."""
        return AcquisitionQuotient(self, cost)
