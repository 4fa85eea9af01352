"""Priors on a model's hyper-parameters: GPy's ``priors.Gaussian`` / ``LogGaussian`` / ``Gamma`` / ``InverseGamma``
(``lnpdf``, ``lnpdf_grad``, ``rvs``) for ``HipGaussianProcess.set_prior`` -- the host form of csrc/hyper_prior.h, written
with the same formulas in the same order; the device evaluates that header (``cbo_gp_log_prior_batch`` and the stage inside
``cbo_gp_hmc_sets`` / ``cbo_gp_mle_sets``).  GPy is not installed here: restated from memory, parity with GPy unpinned; the
densities are tested against ``scipy.stats``.

``log_jacobian`` / ``log_jacobian_grad`` are the Logexp constraint's term GPy's ``log_prior()`` adds for every parameter that
has a prior: ``log(expm1(theta)) - theta`` and ``1 / expm1(theta)``, both 0 above paramz's limit of 36."""
from __future__ import annotations

import math

import numpy as np

from .. import _lib

_LOGEXP_LIM = 36.0
PARAMETER_NAMES = ("variance", "lengthscale", "noise_var")


def log_jacobian(theta):
    """log |d theta / d x| of Logexp at theta."""
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return np.where(theta > _LOGEXP_LIM, 0.0, np.log(np.expm1(theta)) - theta)


def log_jacobian_grad(theta):
    """Its derivative with respect to theta."""
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(over="ignore", divide="ignore"):
        return np.where(theta > _LOGEXP_LIM, 0.0, 1.0 / np.expm1(theta))


class Prior:
    """``kind`` (``_lib.PRIOR_*``), the two parameters and the density's constant: what ``cbo_hyper_prior`` carries."""
    kind = _lib.PRIOR_NONE
    p0 = p1 = constant = 0.0

    def _set(self, p0, p1, names):
        self.p0, self.p1 = float(p0), float(p1)
        for v, n in zip((self.p0, self.p1), names):
            if not math.isfinite(v):
                raise ValueError(f"{type(self).__name__}: {n} must be finite, not {v!r}")

    def descriptor(self):
        """The ``cbo_hyper_prior`` of this prior (the constant, ``lgamma`` included, computed here on the host)."""
        return _lib.CboHyperPrior(self.kind, 0, self.p0, self.p1, self.constant)

    def __eq__(self, other):
        return type(self) is type(other) and (self.p0, self.p1) == (other.p0, other.p1)

    def __hash__(self):
        return hash((type(self).__name__, self.p0, self.p1))

    def __repr__(self):
        return f"{type(self).__name__}({self.p0!r}, {self.p1!r})"


class Gaussian(Prior):
    """N(mu, sigma^2) on theta."""
    kind = _lib.PRIOR_GAUSSIAN

    def __init__(self, mu, sigma):
        self._set(mu, sigma, ("mu", "sigma"))
        if not self.p1 > 0.0:
            raise ValueError(f"{type(self).__name__}: sigma must be positive, not {sigma!r}")
        self.mu, self.sigma = self.p0, self.p1
        self.constant = -0.5 * math.log(2.0 * math.pi * (self.sigma * self.sigma))

    def lnpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        u = x - self.mu
        return self.constant - (u * u) / (2.0 * (self.sigma * self.sigma))

    def lnpdf_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        return -((x - self.mu) / (self.sigma * self.sigma))

    def rvs(self, n):
        return np.random.randn(int(n)) * self.sigma + self.mu


class LogGaussian(Gaussian):
    """log theta ~ N(mu, sigma^2)."""
    kind = _lib.PRIOR_LOGGAUSSIAN

    def lnpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        L = np.log(x)
        u = L - self.mu
        return (self.constant - (u * u) / (2.0 * (self.sigma * self.sigma))) - L

    def lnpdf_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        return -(((np.log(x) - self.mu) / (self.sigma * self.sigma) + 1.0) / x)

    def rvs(self, n):
        return np.exp(np.random.randn(int(n)) * self.sigma + self.mu)


class _ShapeAndRate(Prior):
    """The two parameters and the constant Gamma and InverseGamma share: a log(b) - lgamma(a)."""

    def __init__(self, a, b):
        self._set(a, b, ("a", "b"))
        if not self.p0 > 0.0 or not self.p1 > 0.0:
            raise ValueError(f"{type(self).__name__}: a and b must be positive, not {a!r}, {b!r}")
        self.a, self.b = self.p0, self.p1
        self.constant = self.a * math.log(self.b) - math.lgamma(self.a)


class Gamma(_ShapeAndRate):
    """Gamma with shape a and rate b: density b^a / Gamma(a) theta^(a-1) exp(-b theta)."""
    kind = _lib.PRIOR_GAMMA

    @classmethod
    def from_EV(cls, E, V):
        """The Gamma with expectation E and variance V: a = E^2 / V, b = E / V."""
        E, V = float(E), float(V)
        return cls(E * E / V, E / V)

    def lnpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        return (self.constant + (self.a - 1.0) * np.log(x)) - self.b * x

    def lnpdf_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        return (self.a - 1.0) / x - self.b

    def rvs(self, n):
        return np.random.gamma(shape=self.a, scale=1.0 / self.b, size=int(n))


class InverseGamma(_ShapeAndRate):
    """Inverse gamma with shape a and scale b: density b^a / Gamma(a) theta^(-a-1) exp(-b / theta)."""
    kind = _lib.PRIOR_INVGAMMA

    def lnpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        return (self.constant - (self.a + 1.0) * np.log(x)) - self.b / x

    def lnpdf_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        return self.b / (x * x) - (self.a + 1.0) / x

    def rvs(self, n):
        return 1.0 / np.random.gamma(shape=self.a, scale=1.0 / self.b, size=int(n))


def checked_priors(priors, fix_noise=False):
    """A dict name -> prior (``None`` or empty: no priors) checked on the host: names among ``PARAMETER_NAMES``, values
    ``Prior`` instances, no prior on the noise variance of a model whose noise is fixed.  Returns a new dict in the
    parameters' order."""
    priors = dict(priors or {})
    for name, prior in priors.items():
        if name not in PARAMETER_NAMES:
            raise ValueError(f"a prior goes on one of {PARAMETER_NAMES}, not {name!r}")
        if not isinstance(prior, Prior) or prior.kind not in (_lib.PRIOR_GAUSSIAN, _lib.PRIOR_LOGGAUSSIAN, _lib.PRIOR_GAMMA,
                                                              _lib.PRIOR_INVGAMMA):
            raise ValueError(f"the prior on {name!r} must be a Gaussian, LogGaussian, Gamma or InverseGamma, not {prior!r}")
        if name == "noise_var" and fix_noise:
            raise ValueError("the noise variance of this model is fixed: it takes no prior")
    return {name: priors[name] for name in PARAMETER_NAMES if name in priors}


def per_parameter(priors, n_ls, with_noise=True):
    """The prior of every row entry (variance, lengthscale x n_ls, noise variance when ``with_noise``), None where there is
    none: one lengthscale prior covers every ARD lengthscale."""
    priors = priors or {}
    row = [priors.get("variance")] + [priors.get("lengthscale")] * int(n_ls)
    return row + ([priors.get("noise_var")] if with_noise else [])


def log_prior_host(priors, theta):
    """(log prior, its gradient with respect to theta) of the row ``theta`` under ``priors`` (a list as ``per_parameter``
    returns), Jacobians included, summed in csrc/hyper_prior.h's order -- numpy's log / expm1, so equal to the device's
    value to the libraries' rounding, not bit for bit."""
    theta = np.asarray(theta, dtype=np.float64)
    lp, grad = 0.0, np.zeros(theta.size)
    for k, (prior, t) in enumerate(zip(priors, theta)):
        if prior is None:
            continue
        lp = lp + float(prior.lnpdf(t))
        lp = lp + float(log_jacobian(t))
        grad[k] = float(prior.lnpdf_grad(t)) + float(log_jacobian_grad(t))
    return lp, grad
