"""emukit's max-value entropy search on the MI355X path.

emukit 0.4's ``emukit.bayesian_optimization.acquisitions.MaxValueEntropySearch`` (Wang & Jegelka 2017) fits a Gumbel
distribution to the minimum of the model over a random grid (``update_parameters``), draws ``num_samples`` minima from it,
and scores a candidate by the mean over those samples of the entropy term of its predictive distribution (``evaluate``).
Here both steps run on the device: the grid's predictive mean and variance never leave it, the three bisections of the
Gumbel fit run there (``cbo_gp_mes_gumbel``), and every candidate of a sweep is scored, with the arg-max, in the EI sweep's
path (``cbo_acq_sweep_mes``; include/cbo_hip.h).  The host only draws the random numbers from numpy's global generator and
applies the Gumbel transform to them.  emukit is not installed here: the class restates emukit 0.4 from memory, and parity
is unpinned.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib
from ..GaussianProcessFactory import _column
from .causal_acquisition_functions import AcquisitionQuotient, CandidateGrid
from .causal_optimizer import sample_uniform

MAX_SAMPLES = 64            # cbo_acq_sweep_mes takes at most 64 Gumbel samples


def gumbel_grid(bounds, grid_size, X):
    """The grid of ``update_parameters``: ``space.sample_uniform(grid_size)`` on numpy's global generator
    (``sample_uniform``), with the model's inputs stacked on top, ``np.vstack([model.X, grid])``."""
    grid = sample_uniform(bounds, int(grid_size))
    return np.vstack([np.asarray(X, dtype=np.float64), grid])


def gumbel_mins(num_samples, a, b):
    """``update_parameters``' last step: ``u = np.random.rand(num_samples)`` from the global generator, then the Gumbel
    quantile function ``log(-log(1 - u)) * b + a``."""
    u = np.random.rand(int(num_samples))
    return np.log(-np.log(1 - u)) * b + a


def mes_sets_parameters(models, spaces, num_samples=10, grid_size=5000):
    """``MaxValueEntropySearch.update_parameters`` for every exploration set of a trial with ONE device call for all the
    Gumbel fits (``cbo_gp_mes_gumbel_sets``).  Returns ``(gumbels, mins)``, one entry per set:
    ``(q25, q50, q75, a, b)`` and the ``num_samples`` minima drawn from that Gumbel.

    The draws on numpy's global generator come in a fixed order:
      1. ``gumbel_grid(space_bounds(spaces[i]), grid_size, models[i].X)`` for the sets 0..S-1 in order;
      2. the one ``cbo_gp_mes_gumbel_sets`` call (it draws nothing);
      3. ``gumbel_mins(num_samples, a[i], b[i])`` for the sets 0..S-1 in order.
    (Per-set ``update_parameters`` calls interleave grid and minima set by set: the same seed gives other numbers.)
    The grids' ``CandidateGrid``s are built for this call and closed after it: their points change every trial.  Models of
    at most 128 observations on the fp64 path need no fit; the others are fitted inside the call if they were not."""
    from .utils import space_bounds
    s = len(models)
    if len(spaces) != s:
        raise ValueError(f"spaces must have one entry per exploration set ({s}), not {len(spaces)}")
    if not 0 < int(num_samples) <= MAX_SAMPLES:
        raise ValueError(f"num_samples must be in 1..{MAX_SAMPLES}")
    if int(grid_size) < 1:
        raise ValueError("grid_size must be at least 1")
    points = [gumbel_grid(space_bounds(spaces[i]), grid_size, models[i].X) for i in range(s)]
    quantiles, a, b = np.empty((s, 3)), np.empty(s), np.empty(s)
    grids = []
    try:
        for i in range(s):
            grids.append(CandidateGrid(points[i], models[i]))
        gps = (ctypes.c_void_p * s)(*[m._handle for m in models])
        cds = (ctypes.c_void_p * s)(*[g._handle for g in grids])
        _lib.check(_lib.load().cbo_gp_mes_gumbel_sets(s, gps, cds, _lib.dptr(quantiles), _lib.dptr(a), _lib.dptr(b)))
    finally:
        for g in grids:
            g.close()
    for m in models:
        if not m.small:
            m.stale = False             # (the general path fitted it on the way)
    gumbels = [(float(quantiles[i, 0]), float(quantiles[i, 1]), float(quantiles[i, 2]), float(a[i]), float(b[i]))
               for i in range(s)]
    mins = [gumbel_mins(num_samples, a[i], b[i]) for i in range(s)]
    return gumbels, mins


class MaxValueEntropySearch:
    def __init__(self, model, space, num_samples=10, grid_size=5000):
        """emukit's signature.  ``space``: an emukit ParameterSpace or a list of (lo, hi), as ``space_bounds`` accepts.
        Construction only stores its arguments; the Gumbel fit runs on the first ``evaluate`` / ``sweep`` or on
        ``update_parameters``.  Restated from memory, parity unpinned."""
        from .utils import space_bounds
        self.model = model
        self.space = space
        self.bounds = space_bounds(space)
        self.num_samples = num_samples
        self.grid_size = grid_size
        self.mins = None
        self.gumbel = None          # (q25, q50, q75, a, b) of the last fit

    def update_parameters(self):
        """Draw the grid (model.X on top), fit the Gumbel on the device, draw ``num_samples`` minima from it."""
        if not 0 < int(self.num_samples) <= MAX_SAMPLES:
            raise ValueError(f"num_samples must be in 1..{MAX_SAMPLES}")
        grid = _lib.as_f64(gumbel_grid(self.bounds, self.grid_size, self.model.X))
        m = grid.shape[0]
        pm, pv = None, None
        if self.model.causal:
            pm = _column(self.model.mean_function(grid), m, "mean_function")
            pv = _column(self.model.variance_adjustment(grid), m, "variance_adjustment")
        q = np.empty(3)
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self.model.ensure_fitted()
        _lib.check(_lib.load().cbo_gp_mes_gumbel(self.model._handle, m, _lib.dptr(grid), _lib.dptr(pm), _lib.dptr(pv),
                                                 _lib.dptr(q), ctypes.byref(a), ctypes.byref(b), None, None))
        self.gumbel = (float(q[0]), float(q[1]), float(q[2]), a.value, b.value)
        self.mins = gumbel_mins(self.num_samples, a.value, b.value)

    def sweep(self, candidates, cost=1.0, want_acq=False, want_posterior=False):
        """Score every candidate and pick the best, as ``CausalExpectedImprovement.sweep``: returns dict(best_val,
        best_idx, acq, mean, var).  ``candidates`` is a CandidateGrid (device resident) or an (M,d) array; the value is
        emukit's ``evaluate`` divided by ``cost``."""
        if self.mins is None:
            self.update_parameters()
        mins = _lib.as_f64(np.asarray(self.mins, dtype=np.float64).reshape(-1))
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
            _lib.check(_lib.load().cbo_acq_sweep_mes(self.model._handle, grid._handle, mins.shape[0], _lib.dptr(mins),
                                                     float(cost), _lib.dptr(acq), _lib.dptr(mean), _lib.dptr(var),
                                                     ctypes.byref(best_val), ctypes.byref(best_idx)))
        finally:
            if own:
                grid.close()
        col = lambda v: None if v is None else v[:, None]
        return {"best_val": best_val.value, "best_idx": best_idx.value, "acq": col(acq), "mean": col(mean),
                "var": col(var)}

    def evaluate(self, x):
        """(M,1): emukit's ``evaluate``, fitting the Gumbel first if it has not been.  Restated from memory, parity
        unpinned."""
        return self.sweep(x, want_acq=True)["acq"]

    @property
    def has_gradients(self):
        return False

    def __truediv__(self, cost):
        """``MaxValueEntropySearch(...) / Cost(...)``: emukit's Quotient, here the existing AcquisitionQuotient (the cost
        divides inside the device call)."""
        return AcquisitionQuotient(self, cost)
