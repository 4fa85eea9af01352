"""The causal EI marginalised over hyper-parameter posterior samples on the MI355X path.

emukit's ``IntegratedHyperParameterAcquisition(model, acquisition_generator, n_samples)`` draws hyper-parameter samples
with GPy's HMC (``GPyModelWrapper.generate_hyperparameters_samples``) and averages the acquisition over them:
``for sample in samples: model.fix_model_hyperparameters(sample); acquisition_value += acquisition.evaluate(x)``, then
``acquisition_value / n_samples``.  Here the whole average over a candidate grid, with the arg-max, is ONE device call
(``cbo_acq_sweep_hyper``, include/cbo_hip.h); the sampler is host logic driven by the device likelihood.
emukit and GPy are not installed here: both classes are restated from memory (emukit 0.4, GPy 1.10), parity unpinned.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib
from ..GaussianProcessFactory import logexp_f, logexp_finv
from .causal_acquisition_functions import AcquisitionQuotient, CandidateGrid, CausalExpectedImprovement


def hmc_sample(objective_and_grad, theta0, num_samples, hmc_iters, stepsize):
    """GPy ``inference.mcmc.HMC(model, M=None, stepsize).sample(num_samples, hmc_iters)`` with the unit mass matrix.

    ``theta0``: the model's (positive) parameters; the chain runs on their Logexp transform x = finv(theta), as GPy's runs on
    ``model.optimizer_array``; ``objective_and_grad(x)`` -> (f, df/dx), the model's ``_objective(x, transform="logexp")``.
    Per sample: p ~ N(0, I) by one ``np.random.multivariate_normal(zeros, I)`` call; H_old = f(x) + P log(2 pi) / 2 +
    p.p / 2; the row records the current parameters; ``hmc_iters`` leapfrog steps (p -= stepsize / 2 * grad, x += stepsize
    * p, p -= stepsize / 2 * grad); H_new; accepted with probability min(1, exp(H_old - H_new)) against one
    ``np.random.rand()``: the row becomes the new parameters, otherwise x is restored.  Returns (num_samples, P) rows of
    untransformed parameters theta = f(x).  The objective is evaluated once per position (GPy's model caches likewise).
    Restated from memory: parity with GPy unpinned."""
    x = np.array(logexp_finv(np.asarray(theta0, dtype=np.float64)), dtype=np.float64).reshape(-1)
    size = x.size
    identity = np.eye(size)
    params = np.empty((int(num_samples), size))
    f, g = objective_and_grad(x)
    g = np.asarray(g, dtype=np.float64)

    def hamiltonian(fx, p):
        return fx + size * np.log(2 * np.pi) / 2.0 + np.dot(p, p) / 2.0

    for i in range(int(num_samples)):
        p = np.random.multivariate_normal(np.zeros(size), identity)
        h_old = hamiltonian(f, p)
        x_old, f_old, g_old = x.copy(), f, g
        params[i] = logexp_f(x)
        with np.errstate(over="ignore", invalid="ignore"):
            for _ in range(int(hmc_iters)):
                p = p + (-stepsize / 2.0) * g
                x = x + stepsize * p
                f, g = objective_and_grad(x)
                g = np.asarray(g, dtype=np.float64)
                p = p + (-stepsize / 2.0) * g
            h_new = hamiltonian(f, p)
            k = 1.0 if h_old > h_new else np.exp(h_old - h_new)
        if np.random.rand() < k:
            params[i] = logexp_f(x)
        else:
            x, f, g = x_old, f_old, g_old
    return params


def hmc_draws(size, num_samples):
    """The random numbers ``hmc_sample`` consumes for a chain of ``num_samples`` samples over ``size`` parameters, drawn from
    numpy's global generator in its own order -- per sample one ``np.random.multivariate_normal(zeros, I)``, then one
    ``np.random.rand()``; the chain's course never changes what is drawn.  Returns (momenta (num_samples, size), uniforms
    (num_samples,))."""
    size, num_samples = int(size), int(num_samples)
    identity = np.eye(size)
    momenta = np.empty((num_samples, size))
    uniforms = np.empty(num_samples)
    for i in range(num_samples):
        momenta[i] = np.random.multivariate_normal(np.zeros(size), identity)
        uniforms[i] = np.random.rand()
    return momenta, uniforms


def hmc_sample_from_draws(objective_and_grad, theta0, momenta, uniforms, hmc_iters, stepsize):
    """``hmc_sample``'s arithmetic with the draws handed in (``hmc_draws``): the same chain, bit for bit, without touching
    the generator -- the host form of the chain ``cbo_gp_hmc_sets`` runs on the device (csrc/hmc_chain.h), and the fallback
    for a chain the device declined.  Returns (rows (num_samples, P), accept flags (num_samples,) bool, accept
    probabilities k (num_samples,))."""
    x = np.array(logexp_finv(np.asarray(theta0, dtype=np.float64)), dtype=np.float64).reshape(-1)
    size = x.size
    momenta = np.asarray(momenta, dtype=np.float64).reshape(-1, size)
    uniforms = np.asarray(uniforms, dtype=np.float64).reshape(-1)
    num_samples = uniforms.size
    if momenta.shape[0] != num_samples:
        raise ValueError("momenta must hold one row per uniform")
    params = np.empty((num_samples, size))
    accepted = np.zeros(num_samples, dtype=bool)
    ks = np.empty(num_samples)
    f, g = objective_and_grad(x)
    g = np.asarray(g, dtype=np.float64)

    def hamiltonian(fx, p):
        return fx + size * np.log(2 * np.pi) / 2.0 + np.dot(p, p) / 2.0

    for i in range(num_samples):
        p = momenta[i].copy()
        h_old = hamiltonian(f, p)
        x_old, f_old, g_old = x.copy(), f, g
        params[i] = logexp_f(x)
        with np.errstate(over="ignore", invalid="ignore"):
            for _ in range(int(hmc_iters)):
                p = p + (-stepsize / 2.0) * g
                x = x + stepsize * p
                f, g = objective_and_grad(x)
                g = np.asarray(g, dtype=np.float64)
                p = p + (-stepsize / 2.0) * g
            h_new = hamiltonian(f, p)
            k = 1.0 if h_old > h_new else np.exp(h_old - h_new)
        ks[i] = k
        if uniforms[i] < k:
            params[i] = logexp_f(x)
            accepted[i] = True
        else:
            x, f, g = x_old, f_old, g_old
    return params, accepted, ks


def _hyper_rows(model, samples):
    """(H, 2 + L) rows of (variance, lengthscale x L, noise variance) for ``cbo_acq_sweep_hyper`` from (H, P) samples in
    GPy's parameter order; a model whose noise is fixed has no noise column (P = 1 + L): its own noise fills it."""
    rows = np.atleast_2d(np.asarray(samples, dtype=np.float64))
    n_ls = model.lengthscale.size
    if rows.ndim != 2 or rows.shape[0] < 1:
        raise ValueError("samples must be (H, P) with H >= 1")
    if rows.shape[1] == 1 + n_ls and model.fix_noise:
        rows = np.hstack([rows, np.full((rows.shape[0], 1), model.noise_var)])
    if rows.shape[1] != 2 + n_ls:
        raise ValueError(f"samples must have {2 + n_ls} columns (variance, {n_ls} lengthscale(s), noise variance), "
                         f"not {rows.shape[1]}")
    if rows.shape[0] > _lib.MAX_HYPER_SAMPLES:
        raise ValueError(f"at most {_lib.MAX_HYPER_SAMPLES} samples, not {rows.shape[0]}")
    return np.ascontiguousarray(rows)


class IntegratedHyperParameterAcquisition:
    """emukit's ``IntegratedHyperParameterAcquisition`` for the causal EI: its signature plus ``samples``, an (H, P) array
    that skips the sampler.  ``acquisition_generator(model)`` must return a ``CausalExpectedImprovement`` or that over a
    ``Cost``; the average over the samples runs on the device, the model is not touched when it is small.
    ``sampler="device"`` draws the samples by the one-launch HMC; ``"host"`` (default) is the host chain.

    A generator returning a ``CausalLogExpectedImprovement`` (bare, or over a ``Cost``: ``LogAcquisitionQuotient``) selects the
    log form (``cbo_acq_sweep_hyper_log``): ``log((1 / H) sum_h EI_h) - log cost`` -- the LOGARITHM OF THE
    AVERAGE the EI form computes, finite and ordered where that average is an exact 0.0.  It is not the average of the
    logarithms, which is what emukit's class would form from such a generator.  ``is_log`` tells the two apart."""

    def __init__(self, model, acquisition_generator, n_samples=10, n_burnin=100, subsample_interval=10, step_size=1e-1,
                 leapfrog_steps=20, samples=None, sampler="host"):
        if sampler not in ("host", "device"):
            raise ValueError(f"sampler must be 'host' or 'device', not {sampler!r}")
        self.sampler = sampler
        self.model = model
        self.acquisition_generator = acquisition_generator
        acquisition = acquisition_generator(model)
        from .pointwise_acquisitions import CausalLogExpectedImprovement
        inner = acquisition.numerator if isinstance(acquisition, AcquisitionQuotient) else acquisition
        self.is_log = isinstance(inner, CausalLogExpectedImprovement)
        if not self.is_log and not isinstance(inner, CausalExpectedImprovement):
            raise TypeError("IntegratedHyperParameterAcquisition supports CausalExpectedImprovement and "
                            f"CausalExpectedImprovement / Cost, not {type(acquisition).__name__}")
        if samples is None and (isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1):
            raise ValueError(f"n_samples must be a positive int, not {n_samples!r}")
        self.acquisition = acquisition
        self._ei = inner
        self._cost = acquisition.denominator if isinstance(acquisition, AcquisitionQuotient) else None
        self.n_samples = int(n_samples)
        self.n_burnin = int(n_burnin)
        self.subsample_interval = int(subsample_interval)
        self.step_size = float(step_size)
        self.leapfrog_steps = int(leapfrog_steps)
        if samples is None:
            self.update_parameters()
        else:
            self.samples = _hyper_rows(model, samples)
            self.n_samples = self.samples.shape[0]

    def update_parameters(self):
        """Redraw the samples (emukit: ``model.generate_hyperparameters_samples(...)``)."""
        self.samples = _hyper_rows(self.model, self.model.generate_hyperparameters_samples(
            self.n_samples, self.n_burnin, self.subsample_interval, self.step_size, self.leapfrog_steps,
            **({} if self.sampler == "host" else {"sampler": self.sampler})))

    def sweep(self, candidates, cost=None, want_acq=False):
        """dict(best_val, best_idx, acq, mean, var) as ``CausalExpectedImprovement.sweep`` returns it (mean and var are
        None: they differ per sample) from ONE ``cbo_acq_sweep_hyper`` call (``cbo_acq_sweep_hyper_log`` for a log
        generator).  ``cost``: the batch's scalar cost; by default the generator's ``Cost`` over the candidates, or 1."""
        model = self.model
        own = not isinstance(candidates, CandidateGrid)
        grid = CandidateGrid(candidates, model) if own else candidates
        if cost is None:
            cost = 1.0 if self._cost is None else float(self._cost.evaluate(grid.points))
        acq = np.empty(len(grid)) if want_acq else None
        best_val = ctypes.c_double(0.0)
        best_idx = ctypes.c_int64(-1)
        try:
            lib = _lib.load()
            _lib.check((lib.cbo_acq_sweep_hyper_log if self.is_log else lib.cbo_acq_sweep_hyper)(
                model._handle, grid._handle, self.samples.shape[0], _lib.dptr(self.samples),
                float(np.asarray(self._ei.current_global_min).reshape(-1)[0]), _lib.TASK_CODE[self._ei.task],
                float(self._ei.jitter), float(cost), _lib.dptr(acq), ctypes.byref(best_val), ctypes.byref(best_idx)))
        finally:
            if own:
                grid.close()
        return {"best_val": best_val.value, "best_idx": best_idx.value, "acq": None if acq is None else acq[:, None],
                "mean": None, "var": None}

    def evaluate(self, x):
        """(M,1) marginalised acquisition: one device call."""
        return self.sweep(x, want_acq=True)["acq"]

    @property
    def has_gradients(self):
        return False
