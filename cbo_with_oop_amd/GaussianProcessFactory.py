"""Host-side mirror of the reference's GP factory for the MI355X path.

Same names, argument meaning and error behaviour as /root/reference/src/GaussianProcessFactory.py:9-73;
the object ``create`` returns answers the calls the reference makes on a GPy ``GPRegression`` and on
emukit's ``GPyModelWrapper`` around it, but every number comes from the HIP kernels
behind libcbo_hip.so (include/cbo_hip.h).  There is no CPU implementation in this package.
"""
from __future__ import annotations

import ctypes
import os
import warnings
from enum import IntEnum

import numpy as np

from . import _lib


class GaussianProcessType(IntEnum):
    """src/GaussianProcessFactory.py:9-15."""
    GRAPH_GP = 0
    CAUSAL_GP = 1
    NON_CAUSAL_GP = 2


# paramz ``transformations.Logexp`` (paramz~=0.9.5, requirements.txt:9), the constraint GPy puts on every positive parameter
# of these models (``RBF.variance`` / ``.lengthscale``, ``Gaussian.variance``): the optimiser works on x, the model sees
# theta = log(1 + exp(x)).  Restated here because GPy's ``model.optimize()`` (src/CBO.py:173, src/utils_functions/utils.py:44)
# runs scipy's L-BFGS-B in THAT space, from x0 = finv(theta0): same routine + same space + same start = its trajectory.
_LOGEXP_LIM = 36.0
_LOGEXP_LOG_LIM = float(np.log(np.finfo(np.float64).max))


def logexp_f(x):
    """Logexp.f: theta(x)."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > _LOGEXP_LIM, x, np.log1p(np.exp(np.clip(x, -_LOGEXP_LOG_LIM, _LOGEXP_LIM))))


def logexp_finv(theta):
    """Logexp.finv: x(theta)."""
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.where(theta > _LOGEXP_LIM, theta, np.log(np.expm1(theta)))


def logexp_gradfactor(theta):
    """Logexp.gradfactor without the df factor: d theta / d x = 1 - exp(-theta)."""
    theta = np.asarray(theta, dtype=np.float64)
    return np.where(theta > _LOGEXP_LIM, 1.0, -np.expm1(-theta))


def _column(values, n, what):
    """A reference closure returns (k,1) (DoCalculus.py:66); accept (k,), (k,1) or a scalar."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(n, float(v))
    v = np.ascontiguousarray(v.reshape(-1))
    if v.shape[0] != n:
        raise ValueError(f"{what} returned {v.shape[0]} values for {n} points")
    return v


def standard_normals(size, m):
    """The (size, M) standard normals ``np.random.multivariate_normal(mean, cov, size)`` draws for an M-dimensional
    mean, from numpy's global legacy stream and in the same order: a seeded run stays aligned with GPy's."""
    return np.random.standard_normal((int(size), int(m)))


def gaussian_likelihood_samples(f, variance):
    """GPy ``Gaussian.samples``: one ``np.random.normal(f_j, sqrt(variance), size=1)`` per element of ``f`` in flattened
    order, reshaped to ``f``'s shape."""
    f = np.asarray(f, dtype=np.float64)
    scale = np.sqrt(variance)
    return np.array([np.random.normal(fj, scale=scale, size=1) for fj in f.flatten()]).reshape(f.shape)


class HipGaussianProcess:
    """GP posterior resident on one MI355X.  Duck-types the two objects the reference uses:

    * GPy ``GPRegression``: ``predict(Xnew)`` -> (mean (M,1), var (M,1)) with the Gaussian likelihood
      noise included (used by src/DoCalculus.py:77), ``predict(Xnew, full_cov=True)``,
      ``posterior_covariance_between_points``, ``posterior_samples_f``, ``posterior_samples``, ``X``, ``Y``,
      ``set_XY``, ``optimize``.
    * emukit ``GPyModelWrapper``: ``predict``, ``set_data`` (src/Monitor.py:160), ``optimize``
      (src/CBO.py:173), ``predict_with_full_covariance``, ``predict_covariance``, ``get_covariance_between_points``,
      ``calculate_variance_reduction``, ``X``, ``Y``, ``model``.
    """

    def __init__(self, x, y, *, variance=1.0, lengthscale=1.0, ard=False, noise_var=1e-10, mean_function=None,
                 variance_adjustment=None, zero_diag=None, context=None, fix_noise=False, fit=True, dtype=None):
        if (mean_function is None) != (variance_adjustment is None):
            raise ValueError("mean_function and variance_adjustment must be given together")
        self._lib = _lib.load()
        self._ctx = context if context is not None else _lib.Context.get()
        # "f64" (default) or "f32": the fit is fp64 either way; "f32" runs every sweep / predict of this model on the
        # f32 MFMA from a once-per-fit fp32 copy of the factor (BASELINE.json configs[4]; include/cbo_hip.h)
        self.dtype = dtype if dtype is not None else os.environ.get("CBO_HIP_DTYPE", "f64")
        if self.dtype not in _lib.DTYPE_CODE:
            raise ValueError(f"dtype must be one of {sorted(_lib.DTYPE_CODE)}")
        self.mean_function = mean_function
        self.variance_adjustment = variance_adjustment
        self.causal = mean_function is not None
        self.variance = float(variance)
        self.noise_var = float(noise_var)
        self.ard = bool(ard)
        self.fix_noise = bool(fix_noise)
        x = _lib.as_f64(x)
        if x.ndim != 2:
            raise ValueError("x must be (N, d)")
        self.input_dim = x.shape[1]
        ls = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64))
        if self.ard and ls.size == 1:
            ls = np.full(self.input_dim, ls[0])
        self.lengthscale = np.ascontiguousarray(ls)
        # GPy's plain RBF takes the X2=None shortcut (zero diagonal distance); CausalRBF passes X2
        # explicitly (causal_kernels.py:53-55)
        self.zero_diag = (not self.causal) if zero_diag is None else bool(zero_diag)
        self._handle = ctypes.c_void_p()
        self._priors = {}          # name -> utils_functions.priors.Prior (set_prior); the device handle holds the descriptors
        self._set_arrays(x, y)
        pm, pv = self._prior(self.X)
        _lib.check(self._lib.cbo_gp_create(
            self._ctx.handle, _lib.DTYPE_CODE[self.dtype], self.X.shape[0], self.input_dim, _lib.dptr(self.X), _lib.dptr(self._y_flat),
            _lib.dptr(pm), _lib.dptr(pv), self.variance, _lib.dptr(self.lengthscale), int(self.ard), self.noise_var,
            int(self.zero_diag), ctypes.byref(self._handle)))
        self._initial_hyper = (self.variance, self.lengthscale.copy(), self.noise_var)
        self._hyper_initial = True
        if fit:
            self._fit()
        else:
            self.stale = True      # the first acquisition sweep refits, overlapped (see set_data(fit=False))

    # -- construction helpers ------------------------------------------------------------------
    def _set_arrays(self, x, y):
        x = _lib.as_f64(x)
        y = _lib.as_f64(y)
        if y.ndim == 1:
            y = y[:, None]
        if x.ndim != 2 or y.shape != (x.shape[0], 1):
            raise ValueError(f"expected x (N,d) and y (N,1), got {x.shape} and {y.shape}")
        if x.shape[1] != self.input_dim:
            raise ValueError("input dimension changed")
        self.X, self.Y = x, y
        self._y_flat = np.ascontiguousarray(y[:, 0])

    def _prior(self, pts):
        if not self.causal:
            return None, None
        n = pts.shape[0]
        return (_column(self.mean_function(pts), n, "mean_function"),
                _column(self.variance_adjustment(pts), n, "variance_adjustment"))

    def _fit(self):
        tries = ctypes.c_int(0)
        jitter = ctypes.c_double(0.0)
        _lib.check(self._lib.cbo_gp_fit(self._handle, ctypes.byref(tries), ctypes.byref(jitter)))
        self._note_jitter(tries.value, jitter.value)

    def fit_level(self, level):
        """ONE level of jitchol's ladder (``cbo_gp_fit_level``; sharding.fit_over_ranks walks the ladder with one level
        per rank): ``(outcome, jitter)``, outcome 1 = factored (the model is fitted with ``jitter_tries = level``), 0 =
        not positive definite at this level, -1 = non-positive diagonal entries."""
        status = ctypes.c_int(0)
        jitter = ctypes.c_double(0.0)
        _lib.check(self._lib.cbo_gp_fit_level(self._handle, int(level), ctypes.byref(status), ctypes.byref(jitter)))
        if status.value == 1:
            self._note_jitter(int(level), jitter.value)
        return status.value, jitter.value

    def adopted_factor(self, level):
        """The factor at ``level`` has arrived from another rank (``cbo_comm_share_factor``): the host-side state follows."""
        tries = ctypes.c_int(0)
        jitter = ctypes.c_double(0.0)
        _lib.check(self._lib.cbo_gp_jitter(self._handle, ctypes.byref(tries), ctypes.byref(jitter)))
        self._note_jitter(tries.value, jitter.value)

    def take_factor_slices(self, source, level, n_owners):
        """The receiving side of ``cbo_comm_share_factor`` with device copies in the place of the transfers
        (``cbo_gp_take_factor_slices``): this model takes ``source``'s factor at ``level`` in the ``n_owners`` row slices
        the owners would send, and adopts it.  For tests on one GPU."""
        _lib.check(self._lib.cbo_gp_take_factor_slices(self._handle, source._handle, int(level), int(n_owners)))
        self.adopted_factor(level)
        self.stale = False

    stale = False      # data uploaded, posterior not yet refitted (set_data(..., fit=False))

    @property
    def small(self):
        """At most 128 observations on the fp64 path: the multi-set sweep (``cbo_acq_sweep_sets``) factors and sweeps
        such a model inside one launch, from its resident data, whether it is fitted or not."""
        return self.dtype == "f64" and self.X.shape[0] <= 128

    def _note_jitter(self, tries, jitter):
        self.stale = False
        self.jitter_tries, self.jitter = tries, jitter
        if tries:
            # GPy logs a warning when jitchol needed jitter
            warnings.warn(f"Added jitter of {jitter:.10e}", RuntimeWarning, stacklevel=4)

    # -- reference-facing API -------------------------------------------------------------------
    @property
    def model(self):
        """emukit's wrapper exposes the GPy model as ``.model``; here they are the same object."""
        return self

    def _points(self, x):
        x = _lib.as_f64(x)
        if x.ndim != 2 or x.shape[1] != self.input_dim:
            raise ValueError(f"x must be (M, {self.input_dim})")
        return x

    def predict(self, x, include_likelihood=True, full_cov=False):
        """(mean (M,1), var (M,1)); GP.predict / GPyModelWrapper.predict.  ``full_cov=True``: (mean (M,1), cov (M,M)),
        GPy's full_cov branch (``cbo_gp_predict_cov``): not clipped, the likelihood noise on the diagonal only, and for
        the causal kernel a diagonal of variance * exp(-r2_ii / 2) + v(x) rather than Kdiag (include/cbo_hip.h)."""
        x = self._points(x)
        m = x.shape[0]
        pm, pv = self._prior(x)
        mean = np.empty(m)
        if full_cov:
            cov = np.empty((m, m))
            self.ensure_fitted()
            _lib.check(self._lib.cbo_gp_predict_cov(self._handle, m, _lib.dptr(x), _lib.dptr(pm), _lib.dptr(pv),
                                                    int(include_likelihood), _lib.dptr(mean), _lib.dptr(cov)))
            return mean[:, None], cov
        var = np.empty(m)
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_predict(self._handle, m, _lib.dptr(x), _lib.dptr(pm), _lib.dptr(pv),
                                            int(include_likelihood), _lib.dptr(mean), _lib.dptr(var)))
        return mean[:, None], var[:, None]

    def predict_grouped(self, x, group, include_likelihood=True):
        """Predict at ``x`` ((M*group, d)) and average mean and variance over each consecutive run of ``group``
        rows on the device: (mean (M,1), var (M,1)).  This is the do-calculus reduction of
        src/DoCalculus.py:59-60 (np.mean over the observed rows of one intervention)."""
        x = _lib.as_f64(x)
        if x.ndim != 2 or x.shape[1] != self.input_dim or x.shape[0] % group:
            raise ValueError(f"x must be (M*group, {self.input_dim})")
        m = x.shape[0] // group
        pm, pv = self._prior(x)
        mean = np.empty(m)
        var = np.empty(m)
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_predict_grouped(self._handle, m, group, _lib.dptr(x), _lib.dptr(pm), _lib.dptr(pv),
                                                    int(include_likelihood), _lib.dptr(mean), _lib.dptr(var)))
        return mean[:, None], var[:, None]

    def predict_do(self, observed, intervened_index, values, include_likelihood=True):
        """The do-calculus reduction with the inputs built on the device (``cbo_gp_predict_do``): for every row of
        ``values`` ((M, n_iv)) predict at the rows of ``observed`` ((N_obs, d)) with column j replaced by
        ``values[:, intervened_index[j]]`` where ``intervened_index[j] >= 0``, and average over the rows
        (src/DoCalculus.py:59-60, 74-89).  Returns (mean (M,1), var (M,1)); nothing of size M * N_obs exists on the host."""
        observed = _lib.as_f64(observed)
        values = _lib.as_f64(values)
        if values.ndim == 1:
            values = values[None, :]
        if observed.ndim != 2 or observed.shape[1] != self.input_dim:
            raise ValueError(f"observed must be (N_obs, {self.input_dim})")
        idx = np.ascontiguousarray(intervened_index, dtype=np.int32)
        if idx.shape != (self.input_dim,):
            raise ValueError("intervened_index needs one entry per input column")
        m = values.shape[0]
        mean, var = np.empty(m), np.empty(m)
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_predict_do(self._handle, m, observed.shape[0], _lib.dptr(observed), values.shape[1],
                                               _lib.dptr(values), idx.ctypes.data_as(_lib.c_int_p), int(include_likelihood),
                                               _lib.dptr(mean), _lib.dptr(var)))
        return mean[:, None], var[:, None]

    def predict_noiseless(self, x):
        return self.predict(x, include_likelihood=False)

    def posterior_covariance_between_points(self, X1, X2):
        """GPy ``posterior_covariance_between_points`` without the likelihood: K(X1,X2) - (L^-1 K(X,X1))^T L^-1 K(X,X2),
        (M1, M2) (``cbo_gp_cov_between``).  GPy is not installed here: parity unpinned."""
        X1, X2 = self._points(X1), self._points(X2)
        m1, m2 = X1.shape[0], X2.shape[0]
        pv1 = self._prior(X1)[1]
        pv2 = self._prior(X2)[1]
        cov = np.empty((m1, m2))
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_cov_between(self._handle, m1, _lib.dptr(X1), _lib.dptr(pv1), m2, _lib.dptr(X2),
                                                _lib.dptr(pv2), _lib.dptr(cov)))
        return cov

    # emukit GPyModelWrapper's covariance interface.  Emukit is not installed here: the bodies restate emukit 0.4's
    # gpy_model_wrappers.py from memory, and parity is unpinned for every one of them.
    def predict_with_full_covariance(self, X):
        """emukit ``predict_with_full_covariance``: ``model.predict(X, full_cov=True)`` -> (mean (M,1), cov (M,M)), noise
        included.  Restated from memory, parity unpinned."""
        return self.predict(X, full_cov=True)

    def predict_covariance(self, X, with_noise=True):
        """emukit ``predict_covariance``: the (M,M) covariance of ``model.predict(X, full_cov=True,
        include_likelihood=with_noise)``, clipped elementwise at 1e-10 as recalled of emukit 0.4 (not checked against its
        source).  Restated from memory, parity unpinned."""
        _, cov = self.predict(X, include_likelihood=with_noise, full_cov=True)
        return np.clip(cov, 1e-10, np.inf)

    def get_covariance_between_points(self, X1, X2):
        """emukit ``get_covariance_between_points``: ``model.posterior_covariance_between_points(X1, X2)``.  Restated from
        memory, parity unpinned."""
        return self.posterior_covariance_between_points(X1, X2)

    def calculate_variance_reduction(self, x_train_new, x_test):
        """emukit ``calculate_variance_reduction``: cov(x_train_new, x_test)^2 / predict(x_train_new)[1], the drop in
        variance at ``x_test`` from observing ``x_train_new``.  Restated from memory, parity unpinned."""
        covariance = self.posterior_covariance_between_points(x_train_new, x_test)
        variance_prediction = self.predict(x_train_new)[1]
        return covariance ** 2 / variance_prediction

    # GPy GP's joint posterior samples.  GPy is not installed here: the bodies restate GPy 1.10's core/gp.py and
    # likelihoods/gaussian.py from memory, parity unpinned.
    last_sample_jitter = (0, 0.0)      # (retries, jitter) of the last posterior_samples_f call's factor of Sigma

    def posterior_samples_f(self, X, size=10, normals=None, **predict_kwargs):
        """GPy ``posterior_samples_f``: ``size`` joint draws of f at ``X`` from the noise-free posterior, shape (M, 1, size)
        (``cbo_gp_posterior_samples``).  The normals default to ``standard_normals(size, M)`` -- exactly the draws, in the
        same order, that ``np.random.multivariate_normal(mean, cov, size)`` takes inside GPy, so numpy's global stream is
        left where GPy would leave it; ``normals=`` passes a (size, M) block of one's own.  GPy factors the covariance by
        SVD, the device by Cholesky (with a jitter ladder, ``last_sample_jitter``): the draws have the same distribution
        but are not GPy's draw for draw.  Parity unpinned: GPy not importable here."""
        if predict_kwargs.get("kern") is not None:
            raise NotImplementedError("posterior_samples_f: a kernel other than the model's (kern=) is not supported")
        x = self._points(X)
        m, size = x.shape[0], int(size)
        if normals is None:
            normals = standard_normals(size, m)
        normals = _lib.as_f64(normals)
        if normals.shape != (size, m):
            raise ValueError(f"normals must be (size, M) = ({size}, {m}), got {normals.shape}")
        pm, pv = self._prior(x)
        out = np.empty((m, size))
        tries = ctypes.c_int(0)
        jitter = ctypes.c_double(0.0)
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_posterior_samples(self._handle, m, _lib.dptr(x), _lib.dptr(pm), _lib.dptr(pv), size,
                                                      _lib.dptr(normals), _lib.dptr(out), ctypes.byref(tries),
                                                      ctypes.byref(jitter)))
        self.last_sample_jitter = (tries.value, jitter.value)
        return out[:, None, :]

    def posterior_samples(self, X, size=10, Y_metadata=None, likelihood=None, **predict_kwargs):
        """GPy ``posterior_samples``: ``posterior_samples_f`` with the likelihood's noise added on the host,
        (M, 1, size).  The Gaussian likelihood draws one ``np.random.normal(f, sqrt(noise_var), size=1)`` per element
        in flattened order (``gaussian_likelihood_samples``), as GPy's ``Gaussian.samples``.  Parity unpinned: GPy not
        importable here."""
        fsim = self.posterior_samples_f(X, size, **predict_kwargs)
        for d in range(fsim.shape[1]):
            if likelihood is None:
                fsim[:, d] = gaussian_likelihood_samples(fsim[:, d], self.noise_var)
            else:
                fsim[:, d] = likelihood.samples(fsim[:, d], Y_metadata=Y_metadata)
        return fsim

    def set_data(self, X, Y, fit=True):
        """GPyModelWrapper.set_data -> GP.set_XY: replace the data and refit (src/Monitor.py:160).  When the new data
        are the resident ones plus one observation -- what that call site passes every trial -- the factor grows by
        one column on the device (``append``) instead of being rebuilt; same posterior up to rounding.

        ``fit=False`` uploads only and leaves the refit to the next use: an acquisition sweep then runs the
        refit and the sweep overlapped (``cbo_gp_fit_sweep``); any other consumer (predict, log_likelihood, ...)
        fits first.  A not-positive-definite error then surfaces at that use instead of here."""
        # (a model of at most 128 observations is refactored inside every multi-set sweep anyway: no append there)
        if not (self.dtype == "f64" and np.shape(X)[0] <= 128 and not fit) and self._grew_by_one_row(X, Y) \
                and self.append(np.asarray(X)[-1], np.asarray(Y).reshape(-1)[-1]):
            return                                   # the factor grew by one column instead of being rebuilt
        self._set_arrays(X, Y)
        pm, pv = self._prior(self.X)
        if not fit:
            _lib.check(self._lib.cbo_gp_upload_data(self._handle, self.X.shape[0], _lib.dptr(self.X),
                                                    _lib.dptr(self._y_flat), _lib.dptr(pm), _lib.dptr(pv)))
            self.stale = True
            return
        _lib.check(self._lib.cbo_gp_set_data(self._handle, self.X.shape[0], _lib.dptr(self.X),
                                             _lib.dptr(self._y_flat), _lib.dptr(pm), _lib.dptr(pv)))
        self.stale = False
        tries = ctypes.c_int(0)
        jitter = ctypes.c_double(0.0)
        _lib.check(self._lib.cbo_gp_jitter(self._handle, ctypes.byref(tries), ctypes.byref(jitter)))
        self.jitter_tries, self.jitter = tries.value, jitter.value

    def append(self, x_new, y_new):
        """One more observation (what every CBO trial adds to the set it intervened on): the factor grows by one
        column on the device instead of being rebuilt (``cbo_gp_append``).  Returns False -- and changes nothing --
        when the shortcut does not apply (model not fitted yet, jitter in the factor, padded size exhausted,
        non-positive pivot); the caller then uses ``set_data``."""
        if self.stale:
            return False
        x_new = _lib.as_f64(x_new).reshape(1, self.input_dim)
        y_val = float(np.asarray(y_new, dtype=np.float64).reshape(-1)[0])
        pm, pv = self._prior(x_new)
        done = ctypes.c_int(0)
        _lib.check(self._lib.cbo_gp_append(self._handle, _lib.dptr(x_new), y_val, float(pm[0]) if pm is not None else 0.0,
                                           float(pv[0]) if pv is not None else 0.0, ctypes.byref(done)))
        if not done.value:
            return False
        self.X = np.vstack([self.X, x_new])
        self.Y = np.vstack([self.Y, [[y_val]]])
        self._y_flat = np.ascontiguousarray(self.Y[:, 0])
        return True

    def append_block(self, X_new, Y_new):
        """``k`` more observations in one device step (the results of a batch coming back together): the factor grows
        by ``k`` columns instead of being rebuilt (``cbo_gp_append_block``, at most ``_lib.MAX_APPEND`` points per call).
        Returns False -- and changes nothing -- when the shortcut does not apply (model not fitted yet, jitter in the
        factor, padded size exhausted, fp32 model, non-positive pivot); the caller then uses ``set_data``."""
        if self.stale:
            return False
        X_new = _lib.as_f64(X_new).reshape(-1, self.input_dim)
        y_new = _lib.as_f64(Y_new).reshape(-1)
        if y_new.shape[0] != X_new.shape[0]:
            raise ValueError(f"X_new has {X_new.shape[0]} rows, Y_new {y_new.shape[0]}")
        pm, pv = self._prior(X_new)
        done = ctypes.c_int(0)
        _lib.check(self._lib.cbo_gp_append_block(self._handle, X_new.shape[0], _lib.dptr(X_new), _lib.dptr(y_new),
                                                 _lib.dptr(pm), _lib.dptr(pv), ctypes.byref(done)))
        if not done.value:
            return False
        self.X = np.vstack([self.X, X_new])
        self.Y = np.vstack([self.Y, y_new[:, None]])
        self._y_flat = np.ascontiguousarray(self.Y[:, 0])
        return True

    def _grew_by_one_row(self, X, Y):
        """The new data are the resident ones plus one observation (what src/Monitor.py:148-160 produces every
        trial) and the model is fitted: the append shortcut applies."""
        if self.stale:
            return False
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64).reshape(-1, 1)
        return (X.ndim == 2 and X.shape[0] == self.X.shape[0] + 1 and X.shape[1] == self.X.shape[1]
                and Y.shape[0] == X.shape[0] and np.array_equal(X[:-1], self.X) and np.array_equal(Y[:-1], self.Y))

    def ensure_fitted(self):
        """Fit now if the data were replaced with ``set_data(..., fit=False)`` and nothing has refitted since."""
        if self.stale:
            self._fit()

    set_XY = set_data

    def log_likelihood(self):
        """GPy ``model.log_likelihood()``: log marginal likelihood of the fitted model (device reduction over
        the factor's diagonal and z = L^-1 (y - m))."""
        out = ctypes.c_double(0.0)
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_log_marginal(self._handle, ctypes.byref(out)))
        return out.value

    def set_hyperparameters(self, variance, lengthscale, noise_var, fit=True):
        """Replace kernel variance, lengthscale(s) and Gaussian noise variance and refit (``fit=False``: the next
        use refits, as with ``set_data``)."""
        ls = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64))
        if self.ard and ls.size == 1:
            ls = np.full(self.input_dim, ls[0])
        ls = np.ascontiguousarray(ls)
        _lib.check(self._lib.cbo_gp_set_hyper(self._handle, float(variance), _lib.dptr(ls), float(noise_var)))
        self.variance, self.lengthscale, self.noise_var = float(variance), ls, float(noise_var)
        v0, ls0, nv0 = self._initial_hyper
        self._hyper_initial = (self.variance, self.noise_var) == (v0, nv0) and np.array_equal(ls, ls0)
        self.stale = True            # the device model is unfitted from here on; _fit clears the flag when it succeeds
        if fit:
            self._fit()

    def hyper_is_initial(self):
        """The hyper-parameters are the ones the constructor was given (what a model rebuilt by the reference starts
        from); they only change through ``set_hyperparameters``, which keeps the answer."""
        return self._hyper_initial

    def rebuild(self, X, Y, fit=True):
        """What the reference obtains by constructing a NEW model on new data (src/CBO.py:224-235 builds one each
        trial): the hyper-parameters the constructor was given, the new data.  Same device handle and buffers, so
        nothing is allocated when the padded size does not change."""
        if not self.hyper_is_initial():
            v0, ls0, nv0 = self._initial_hyper
            self.set_hyperparameters(v0, ls0, nv0, fit=False)
        self.set_data(X, Y, fit=fit)                 # appends when the data merely grew by one row

    def log_likelihood_gradients(self):
        """(d log p(y)/d variance, d/d lengthscale (array), d/d noise_var) of the fitted model: the gradients GPy's
        inference hands its optimiser, computed on the device (``cbo_gp_lml_gradients``).  A model of at most 128
        observations is not fitted for this: one launch goes from the data and the current hyper-parameters to the
        likelihood and its gradients (the general path, jitchol ladder included, takes over when that fails)."""
        if not self.small:
            self.ensure_fitted()
        lml, dv, dn = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        dls = np.zeros(self.lengthscale.size)
        _lib.check(self._lib.cbo_gp_lml_gradients(self._handle, ctypes.byref(lml), ctypes.byref(dv), _lib.dptr(dls),
                                                  ctypes.byref(dn)))
        self._last_lml = lml.value
        return dv.value, dls, dn.value

    # -- priors on the hyper-parameters (GPy set_prior) ---------------------------------
    @property
    def priors(self):
        """The priors as a dict name -> prior (``"variance"``, ``"lengthscale"``, ``"noise_var"``), a copy."""
        return dict(self._priors)

    def _upload_priors(self, priors):
        from .utils_functions.priors import checked_priors, per_parameter
        priors = checked_priors(priors, self.fix_noise)
        row = per_parameter(priors, self.lengthscale.size)
        desc = (_lib.CboHyperPrior * len(row))(*[p.descriptor() if p is not None else _lib.CboHyperPrior() for p in row])
        _lib.check(self._lib.cbo_gp_set_priors(self._handle, len(row), desc))
        self._priors = priors

    def set_prior(self, name, prior):
        """GPy ``model.<parameter>.set_prior(prior)``: ``name`` is ``"variance"``, ``"lengthscale"`` (one prior covers every
        ARD lengthscale) or ``"noise_var"`` (ValueError for a model whose noise is fixed); ``prior`` a ``Gaussian``,
        ``LogGaussian``, ``Gamma`` or ``InverseGamma`` of ``utils_functions.priors``.  The priors are state of the model:
        ``set_data``, ``rebuild``, ``append``, ``set_hyperparameters`` and fits keep them.  From here on ``optimize`` (host
        and device), ``optimize_restarts`` and the HMC work on the log posterior (``objective_function``)."""
        self._upload_priors({**self._priors, name: prior})

    def unset_priors(self, name=None):
        """GPy ``unset_priors``: drop the prior on ``name``, or every prior.  A model without priors takes the code paths
        and gives the bits of one that never had any."""
        from .utils_functions.priors import PARAMETER_NAMES
        if name is not None and name not in PARAMETER_NAMES:
            raise ValueError(f"a prior goes on one of {PARAMETER_NAMES}, not {name!r}")
        self._upload_priors({} if name is None else {k: v for k, v in self._priors.items() if k != name})

    def log_prior(self):
        """GPy ``model.log_prior()``: the sum of the priors' log densities at the current parameters plus the Logexp
        log-Jacobian of every parameter that has a prior, evaluated on the device (``cbo_gp_log_prior_batch``); 0.0
        without priors."""
        return log_prior_batch([self])[0][0]

    def log_prior_gradients(self):
        """Its gradient with respect to (variance, lengthscale(s), noise variance) -- without the noise entry for a model
        whose noise is fixed; zeros without priors."""
        return log_prior_batch([self])[0][1]

    def objective_function(self):
        """GPy ``model.objective_function()``: ``-log_likelihood() - log_prior()``."""
        return -self.log_likelihood() - self.log_prior()

    def _loo(self, want_mean=False, want_var=False, want_lpd=False):
        """``cbo_gp_loo`` of the fitted model: (mean, var, lpd, sum of lpd), None where not asked for."""
        self.ensure_fitted()
        n = self.X.shape[0]
        mean, var, lpd = (np.zeros(n) if want else None for want in (want_mean, want_var, want_lpd))
        total = ctypes.c_double(0.0)
        _lib.check(self._lib.cbo_gp_loo(self._handle, _lib.dptr(mean), _lib.dptr(var), _lib.dptr(lpd), ctypes.byref(total)))
        return mean, var, lpd, total.value

    def loo(self):
        """GPy ``model.inference_method.LOO(kern, X, Y, likelihood, posterior)``: the leave-one-out log predictive
        density of every observation, (n, 1), GPy's shape and sign -- computed on the device from the resident factor
        (``cbo_gp_loo``; Rasmussen & Williams 5.4.2).  A factor that carries jitchol jitter gives the LOO of the
        jittered Ky (``jitter_tries`` tells)."""
        return self._loo(want_lpd=True)[2][:, None]

    def loo_predict(self):
        """(mean (n, 1), var (n, 1)) of every observation predicted from the other n - 1; the variance is that of the
        observation, noise included."""
        mean, var, _, _ = self._loo(want_mean=True, want_var=True)
        return mean[:, None], var[:, None]

    def loo_score(self):
        """The LOO pseudo-likelihood, the sum of ``loo()``, summed on the device in a fixed order."""
        return self._loo()[3]

    def _objective(self, x, transform="log"):
        """(negative log marginal likelihood, its gradient with respect to x) at theta(x) = [variance, lengthscale(s),
        (noise)]: ``transform="logexp"``: theta = log(1 + exp(x)), paramz's ``Model._objective_grads`` with
        ``_transform_gradients`` (gradient times 1 - exp(-theta)); ``"log"``: theta = exp(x).  A model with priors: the
        negative log POSTERIOR -- the log prior and its gradient (one more device call) are added to the likelihood's before
        the sign and the transform, as the device kernels add them; ``"logexp"`` only (ValueError otherwise)."""
        _check_prior_transform(self, transform)
        x = np.asarray(x, dtype=np.float64)
        theta = logexp_f(x) if transform == "logexp" else np.exp(x)
        try:
            _objective_set(self, theta)
            dv, dls, dn = self.log_likelihood_gradients()
        except np.linalg.LinAlgError:
            # paramz hands the optimiser inf and the clipped gradient of the last good point (and gives up after ten such
            # evaluations in a row); a large finite value keeps scipy's line search defined and is rejected the same way
            return 1e25, np.zeros_like(x)
        prior = log_prior_batch([self])[0] if _has_priors(self) else None
        return _objective_value(self, theta, self._last_lml, dv, dls, dn, transform, prior)

    def optimize(self, max_iters=1000, transform="logexp", optimizer="host", device_rows=128, **kwargs):
        """Hyper-parameter MLE (emukit ``GPyModelWrapper.optimize`` -> GPy ``optimize_restarts(1, robust=True)`` -- one run from
        the current parameters, nothing drawn --, src/CBO.py:173; ``gp.optimize()`` in src/utils_functions/utils.py:44):
        maximise the log marginal likelihood over kernel variance, lengthscale(s) and -- unless fixed, as for graph-level
        GPs -- the noise variance.  Host logic, as paramz has it (``Model.optimize`` -> ``opt_lbfgsb.opt``):
        ``scipy.optimize.fmin_l_bfgs_b(f_fp, x0, maxfun=max_iters, maxiter=max_iters)`` on the Logexp-transformed
        parameters from ``x0 = finv(theta0)``, the model left at the routine's ``x_opt``.  Every evaluation is a device
        refit plus the device likelihood and its analytic gradients.  ``transform="log"`` is rounds 1-4's parametrisation
        (theta = exp(x), same stationary point, another path to it).  GPy is not installed here: the trajectory is GPy's
        by construction, not by comparison (parity unpinned).
        ``optimizer="device"``: the whole search inside one device launch (``optimize_together([self], ...,
        optimizer="device")``, DESIGN.md §4v: ``lockstep_lbfgs``' iteration, not scipy's); ``"host"`` is the run described
        above, unchanged.  ``device_rows=256`` lets the launch take a model of 129..256 observations."""
        from scipy.optimize import fmin_l_bfgs_b
        checked_mle_device_rows(device_rows, checked_mle_optimizer(optimizer))
        if optimizer == "device":
            return optimize_together([self], max_iters, transform, optimizer="device", device_rows=device_rows)[0]
        theta0, x0 = _optimizer_start(self, transform)
        x_opt, f_opt, info = fmin_l_bfgs_b(lambda x: self._objective(x, transform), x0, maxfun=int(max_iters),
                                           maxiter=int(max_iters))
        f_opt = self._objective(x_opt, transform)[0]          # opt_lbfgsb: f_opt = f_fp(x_opt)[0]; the model sits at x_opt
        return _optimizer_finish(self, theta0, x_opt, f_opt, info, transform)

    def optimize_restarts(self, num_restarts=10, max_iters=1000, optimizer="device", device_rows=128, **kwargs):
        """GPy ``model.optimize_restarts(num_restarts)``: the MLE from the current parameters and from ``num_restarts - 1``
        randomised starts (``mle_restart_starts``: paramz ``randomize()``, a standard normal in the Logexp space, numpy's
        global generator), the model left at the best end point.  Every start is one workgroup of ONE device launch
        (DESIGN.md §4v); ``optimizer="host"`` would be ``num_restarts`` optimiser runs one after another and is not offered
        (ValueError for more than one start).  Returns the ``optimization_result``; its ``runs`` hold every start's record.
        A model with priors (``set_prior``): a parameter that has one is drawn from it, as paramz does, and the best end point
        is the one with the highest log posterior (every run's ``lml`` then includes the log prior).
        ``device_rows=256``: a model of 129..256 observations has its restarts inside the launch too."""
        return optimize_together([self], max_iters, "logexp", optimizer=optimizer, num_restarts=num_restarts,
                                 device_rows=device_rows)[0]

    def generate_hyperparameters_samples(self, n_samples=20, n_burnin=100, subsample_interval=10, step_size=1e-1,
                                         leapfrog_steps=20, sampler="host"):
        """emukit ``GPyModelWrapper.generate_hyperparameters_samples``: ``optimize()``, a multiplicative 1 % perturbation of
        the parameters (``theta * (1 + 0.01 * np.random.randn(P))``, numpy's global generator), GPy's HMC over the
        Logexp-transformed parameters (``integrated_hyper.hmc_sample`` on this model's ``_objective``) for
        ``n_burnin + n_samples * subsample_interval`` samples, and ``samples[n_burnin::subsample_interval]``: an
        (n_samples, P) array of (variance, lengthscale(s), noise variance) rows -- without the noise column for a model whose
        noise is fixed.  The model is LEFT AT THE CHAIN'S LAST STATE, unfitted (``stale``): the next use refits it there.
        ``sampler="device"``: the same draws from the generator, the chain inside one device launch
        (``generate_hyperparameters_samples_together([self], ...)``); ``"host"`` is the chain described above.
        emukit and GPy are not installed here: restated from memory, parity unpinned."""
        from .utils_functions.integrated_hyper import hmc_sample
        if sampler not in ("host", "device"):
            raise ValueError(f"sampler must be 'host' or 'device', not {sampler!r}")
        if sampler == "device":
            return generate_hyperparameters_samples_together([self], n_samples, n_burnin, subsample_interval, step_size,
                                                             leapfrog_steps)[0]
        self.optimize()
        theta0, _ = _optimizer_start(self, "logexp")
        theta0 = theta0 * (1.0 + 0.01 * np.random.randn(theta0.size))
        num = int(n_burnin) + int(n_samples) * int(subsample_interval)
        samples = hmc_sample(lambda x: self._objective(x, "logexp"), theta0, num, int(leapfrog_steps), float(step_size))
        _objective_set(self, samples[-1], fit=False)         # (the last evaluation may have been a rejected proposal)
        return samples[int(n_burnin)::int(subsample_interval)]

    def get_prediction_gradients(self, x):
        """emukit ``GPyModelWrapper.get_prediction_gradients`` -> GPy ``predictive_gradients``:
        (d mean / d x (M,d), d var / d x (M,d)).  As in GPy, the mean function's and the causal rank-1 term's own
        gradients are not included.  Any number of points (a whole grid included): forward and
        backward substitution of the batch on the device."""
        x = _lib.as_f64(x)
        if x.ndim != 2 or x.shape[1] != self.input_dim:
            raise ValueError(f"x must be (M, {self.input_dim})")
        m = x.shape[0]
        pv = _column(self.variance_adjustment(x), m, "variance_adjustment") if self.causal else None
        dmean = np.empty((m, self.input_dim))
        dvar = np.empty((m, self.input_dim))
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_predict_gradients(self._handle, m, _lib.dptr(x), _lib.dptr(pv), _lib.dptr(dmean),
                                                      _lib.dptr(dvar)))
        return dmean, dvar

    # -- posterior state (GPy: model.posterior.woodbury_chol / woodbury_vector) -------------------
    def posterior_state(self):
        n = self.X.shape[0]
        L = np.empty((n, n))
        alpha = np.empty(n)
        self.ensure_fitted()
        _lib.check(self._lib.cbo_gp_get_posterior(self._handle, _lib.dptr(L), _lib.dptr(alpha)))
        return L, alpha[:, None]

    def assembled_Ky(self):
        n = self.X.shape[0]
        K = np.empty((n, n))
        _lib.check(self._lib.cbo_gp_assemble_kxx(self._handle, _lib.dptr(K)))
        return K

    # -- lifetime ------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            if not self._ctx.closed:               # after cbo_shutdown the device memory is gone with the context
                self._lib.cbo_gp_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the pieces of HipGaussianProcess._objective / optimize that the lockstep form shares with them

def _objective_set(model, theta, fit=None):
    """The model at theta (a small model is not fitted for its likelihood; a larger one is, and may raise
    LinAlgError; ``fit`` overrides)."""
    nl = model.lengthscale.size
    noise = model.noise_var if model.fix_noise else theta[1 + nl]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model.set_hyperparameters(theta[0], theta[1:1 + nl], noise, fit=(not model.small) if fit is None else fit)


def _batched(model):
    """The batched likelihood launch answers this model without a fit: fp64, at most 256 observations (above 128 in
    the kernel's two-block form)."""
    return model.dtype == "f64" and model.X.shape[0] <= 256


def _has_priors(model):
    """The model carries at least one prior (a stand-in without the attribute carries none)."""
    return bool(getattr(model, "_priors", None))


def _check_prior_transform(model, transform):
    if transform != "logexp" and _has_priors(model):
        raise ValueError("a model with priors is optimised over the Logexp-transformed parameters (the log prior carries "
                         "that constraint's Jacobian): transform must be 'logexp'")


def log_prior_batch(models, thetas=None):
    """``(log_prior, its gradient with respect to theta)`` of many models in one device call (``cbo_gp_log_prior_batch``:
    one lane per model evaluates csrc/hyper_prior.h).  ``thetas[k]``: the row (variance, lengthscale(s), and the noise
    variance unless the model's noise is fixed) to evaluate model k at, None -- or ``thetas=None`` for all -- for its own
    parameters.  The gradient has the row's entries.  A model without priors answers (0.0, zeros)."""
    k = len(models)
    lib = _lib.load()
    handles = (ctypes.c_void_p * k)(*[m._handle for m in models])
    rows, ptrs = [], (_lib.c_double_p * k)()
    for j, m in enumerate(models):
        t = None if thetas is None or thetas[j] is None else np.asarray(thetas[j], dtype=np.float64).reshape(-1)
        if t is not None:
            t = np.ascontiguousarray(np.append(t, m.noise_var) if m.fix_noise else t)
            if t.size != 2 + m.lengthscale.size:
                raise ValueError(f"theta of model {j} must have {2 + m.lengthscale.size - int(m.fix_noise)} entries")
            ptrs[j] = ctypes.cast(_lib.dptr(t), _lib.c_double_p)
        rows.append(t)
    lp, grad = np.zeros(k), np.zeros((k, _lib.HMC_MAX_PARAMS))
    status = np.zeros(k, dtype=np.int32)
    _lib.check(lib.cbo_gp_log_prior_batch(k, handles, ptrs, _lib.dptr(lp), _lib.dptr(grad),
                                          status.ctypes.data_as(_lib.c_int_p)))
    return [(float(lp[j]), grad[j, :1 + m.lengthscale.size + (0 if m.fix_noise else 1)].copy())
            for j, m in enumerate(models)]


def _objective_value(model, theta, lml, dv, dls, dn, transform, prior=None):
    """(-lml, -gradient with respect to x) from the likelihood and its gradients at theta(x); ``prior`` = (log prior, its
    gradient with respect to theta): added first, so the pair is the negative log posterior's."""
    g = np.asarray([dv, *dls] + ([] if model.fix_noise else [dn]), dtype=np.float64)
    if prior is not None:
        lml, g = lml + prior[0], g + prior[1]
    g = g * (logexp_gradfactor(theta) if transform == "logexp" else theta)
    return -lml, -g


def _optimizer_start(model, transform):
    """(theta0, x0) of ``optimize``."""
    if transform not in ("logexp", "log"):
        raise ValueError("transform must be 'logexp' (GPy / paramz) or 'log'")
    _check_prior_transform(model, transform)
    theta0 = [model.variance, *model.lengthscale]
    if not model.fix_noise:
        theta0.append(model.noise_var)
    theta0 = np.asarray(theta0, dtype=np.float64)
    return theta0, (logexp_finv(theta0) if transform == "logexp" else np.log(theta0))


def _optimizer_finish(model, theta0, x_opt, f_opt, info, transform):
    """What ``optimize`` does once the routine has returned and ``f_fp(x_opt)`` has been re-evaluated."""
    from scipy.optimize import OptimizeResult
    if f_opt >= 1e25:                     # the factorisation failed at the point the optimiser settled on
        nl = model.lengthscale.size       # (GPy restores the previous parameters after a failed step): back to the
        model.set_hyperparameters(theta0[0], theta0[1:1 + nl],     # starting point, which was fitted before
                                  model.noise_var if model.fix_noise else theta0[1 + nl])
    res = OptimizeResult(x=x_opt, fun=f_opt, jac=info["grad"], nfev=info["funcalls"], nit=info["nit"],
                         status=info["warnflag"], message=info["task"], success=info["warnflag"] == 0,
                         transform=transform)
    model.optimization_result = res
    return res


def lml_gradients_batch(models):
    """``log_likelihood_gradients`` of many models in one device call (``cbo_gp_lml_gradients_batch``: one launch for
    every fp64 model of at most 256 observations -- for n <= 128 the same bits as one model alone, above in the
    kernel's two-block form -- none of them fitted for it; larger models are fitted first).  Returns, per model, (lml,
    d/d variance, d/d lengthscale (array), d/d noise_var), or None where Ky is not positive definite even with the
    jitchol ladder's jitter (the model alone raises LinAlgError)."""
    if not models:
        return []
    lib = _lib.load()
    for m in models:
        if not _batched(m):
            m.ensure_fitted()
    k = len(models)
    handles = (ctypes.c_void_p * k)(*[m._handle for m in models])
    lml, dv, dn = np.zeros(k), np.zeros(k), np.zeros(k)
    dls = np.zeros(k * _lib.MAX_DIM)
    status = np.zeros(k, dtype=np.int32)
    _lib.check(lib.cbo_gp_lml_gradients_batch(k, handles, _lib.dptr(lml), _lib.dptr(dv), _lib.dptr(dls), _lib.dptr(dn),
                                              status.ctypes.data_as(_lib.c_int_p)))
    out = []
    for i, m in enumerate(models):
        rc = int(status[i])
        if rc in (_lib.CBO_ERR_NOT_PD, _lib.CBO_ERR_NONPOS_DIAG):
            out.append(None)
            continue
        _lib.check(rc)
        m._last_lml = float(lml[i])
        base = i * _lib.MAX_DIM
        out.append((float(lml[i]), float(dv[i]), dls[base:base + m.lengthscale.size].copy(), float(dn[i])))
    return out


def checked_mle_optimizer(optimizer, num_restarts=1):
    """``optimizer`` (``"host"``: scipy's L-BFGS-B with one device call per evaluation; ``"device"``: the one-launch search,
    DESIGN.md §4v) and ``num_restarts`` (1..``_lib.MLE_MAX_STARTS``; more than one start on the device alone) checked on
    the host, before any device call.  Returns ``optimizer``."""
    if optimizer not in ("host", "device"):
        raise ValueError(f"optimizer must be 'host' or 'device', not {optimizer!r}")
    if isinstance(num_restarts, bool) or not isinstance(num_restarts, (int, np.integer)) \
            or not 1 <= num_restarts <= _lib.MLE_MAX_STARTS:
        raise ValueError(f"num_restarts must be an int in 1..{_lib.MLE_MAX_STARTS}, not {num_restarts!r}")
    if optimizer == "host" and num_restarts > 1:
        raise ValueError("restarts are run by the device launch: num_restarts > 1 needs optimizer='device'")
    return optimizer


def checked_mle_device_rows(device_rows, optimizer="device"):
    """``device_rows``: the largest model the one-launch search takes -- 128 (``cbo_gp_mle_sets``) or 256 (the
    two-block form beside it, ``cbo_gp_mle_sets_rows``; ``optimizer="device"`` alone) -- checked on the host,
    before any device call.  Returns ``device_rows``."""
    if isinstance(device_rows, bool) or not isinstance(device_rows, (int, np.integer)) or device_rows not in (128, 256):
        raise ValueError(f"device_rows must be 128 or 256, not {device_rows!r}")
    if device_rows == 256 and optimizer != "device":
        raise ValueError("device_rows=256 chooses the models the device launch takes: it needs optimizer='device'")
    return int(device_rows)


def mle_restart_starts(P, num_restarts, priors=None, fit_noise=True):
    """The randomised starts of ``optimize_restarts``: ``num_restarts - 1`` rows ``x = np.random.randn(P)`` in the Logexp
    space (paramz ``randomize()``: a standard normal for every transformed parameter), one ``randn(P)`` call per row from
    numpy's global generator; (num_restarts - 1, P).  One start draws nothing.
    ``priors`` (a dict name -> prior, as ``HipGaussianProcess.priors``): paramz draws a parameter that has a prior FROM the
    prior.  Per row, after its ``randn(P)``: in the order variance, lengthscale, noise variance, one ``prior.rvs(size)`` per
    parameter that has a prior (size = the number of lengthscales, P - 1 - ``fit_noise``, for that one, else 1; the noise
    only when ``fit_noise``: the row's last entry) replaces those entries of theta = ``logexp_f(x)`` -- the row keeps
    ``x = logexp_finv(drawn)`` there.  A drawn value that is not positive and finite -- possible under a Gaussian prior --
    keeps the ``randn`` entry: ``cbo_gp_mle_sets`` refuses such starts (a deviation from paramz, which would hand it to
    the model).  Without priors nothing changes, the generator's consumption included."""
    rows = []
    n_ls = int(P) - 1 - int(bool(fit_noise))
    slots = (("variance", 0, 1), ("lengthscale", 1, n_ls)) + ((("noise_var", 1 + n_ls, 1),) if fit_noise else ())
    for _ in range(int(num_restarts) - 1):
        x = np.random.randn(P)
        for name, lo, size in slots if priors else ():
            if name not in priors:
                continue
            drawn = np.asarray(priors[name].rvs(size), dtype=np.float64).reshape(-1)
            ok = np.isfinite(drawn) & (drawn > 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                x[lo:lo + size] = np.where(ok, logexp_finv(np.where(ok, drawn, 1.0)), x[lo:lo + size])
        rows.append(x)
    return np.array(rows, dtype=np.float64).reshape(-1, P)


def mle_best_run(lmls, statuses):
    """The run GPy's ``argmin(f_opt)`` keeps: the highest final ``lml`` among the runs that have one (neither ``NAN_START``
    nor ``NOT_PD``, and not NaN), the lowest index on ties; None when no run has."""
    best = None
    for j, (v, st) in enumerate(zip(lmls, statuses)):
        if st in (_lib.REFINE_NAN_START, _lib.MLE_NOT_PD, _lib.MLE_DECLINED) or v != v:
            continue
        if best is None or v > lmls[best]:
            best = j
    return best


def mle_runs_device(models, theta0s, max_rounds, device_rows=128):
    """One ``cbo_gp_mle_sets`` call -- with ``device_rows=256`` one ``cbo_gp_mle_sets_rows`` call, which also takes the fp64
    models of 129..256 observations --: model k's searches from the rows of ``theta0s[k]`` ((n_starts, P)
    parameters).  Returns per model dict(declined, status (n_starts,), rounds, theta (n_starts, P), lml, grad): every run's reason for stopping
    (``_lib.REFINE_*`` or ``_lib.MLE_NOT_PD``), rounds and end point with the likelihood and its gradients there --
    meaningless for a ``NOT_PD`` run and for a declined model.  The models are only read."""
    device_rows = checked_mle_device_rows(device_rows)
    k = len(models)
    lib = _lib.load()
    handles = (ctypes.c_void_p * k)(*[m._handle for m in models])
    runs = (_lib.CboMleRun * k)()
    model_status = np.full(k, -1, dtype=np.int32)
    out, keep = [], []
    for j, (m, theta0) in enumerate(zip(models, theta0s)):
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
        if theta0.ndim == 1:
            theta0 = theta0[None]
        starts, size = theta0.shape
        o = dict(declined=False, status=np.full(starts, -1, dtype=np.int32), rounds=np.zeros(starts, dtype=np.int32),
                 theta=np.full((starts, size), np.nan), lml=np.full(starts, np.nan), grad=np.full((starts, size), np.nan))
        r = runs[j]
        r.n_params, r.fit_noise, r.n_starts, r.max_rounds = size, 0 if m.fix_noise else 1, starts, int(max_rounds)
        r.theta0 = _lib.dptr(theta0)
        r.theta_out, r.lml_out, r.grad_out = _lib.dptr(o["theta"]), _lib.dptr(o["lml"]), _lib.dptr(o["grad"])
        r.status_out, r.rounds_out = o["status"].ctypes.data_as(_lib.c_int_p), o["rounds"].ctypes.data_as(_lib.c_int_p)
        out.append(o)
        keep.append(theta0)
    if device_rows == 128:
        _lib.check(lib.cbo_gp_mle_sets(k, handles, runs, model_status.ctypes.data_as(_lib.c_int_p)))
    else:
        _lib.check(lib.cbo_gp_mle_sets_rows(k, handles, runs, device_rows, model_status.ctypes.data_as(_lib.c_int_p)))
    for o, st in zip(out, model_status):
        o["declined"] = int(st) == _lib.MLE_DECLINED
    return out


def _optimize_on_device(models, max_iters, num_restarts, host_fallback, device_rows=128):
    """``optimize_together``'s device route: the results, None where the model has to take the host route."""
    from scipy.optimize import OptimizeResult
    max_rounds = min(int(max_iters), _lib.MLE_MAX_ROUNDS)
    theta0s = []
    for m in models:                                           # (the draws: per model, in model order, before the call)
        theta0, _ = _optimizer_start(m, "logexp")
        extra = mle_restart_starts(theta0.size, num_restarts, getattr(m, "_priors", None) or None, not m.fix_noise)
        theta0s.append(np.vstack([theta0[None], logexp_f(extra)]) if extra.size else theta0[None])
    answers = mle_runs_device(models, theta0s, max_rounds, device_rows)
    results = [None] * len(models)
    for j, (m, a) in enumerate(zip(models, answers)):
        back = a["declined"] or int(a["status"][0]) == _lib.MLE_NOT_PD
        if back:
            if not host_fallback:
                why = "was declined" if a["declined"] else "starts at a Ky that is not positive definite as assembled"
                raise RuntimeError(f"the device search of model {j} {why} and host_fallback is off")
            continue
        status = [int(v) for v in a["status"]]
        runs = [dict(theta0=theta0s[j][i].copy(), theta=a["theta"][i].copy(), lml=float(a["lml"][i]), grad=a["grad"][i].copy(),
                     rounds=int(a["rounds"][i]), status=status[i], message=_lib.MLE_STATUS_NAME.get(status[i], "?"))
                for i in range(len(status))]
        best = mle_best_run(a["lml"], status)
        won = runs[0 if best is None else best]
        if best is not None:                                   # (every run failed: the model keeps its parameters)
            _objective_set(m, won["theta"], fit=False)
            m._last_lml = won["lml"]
        theta = won["theta"]
        res = OptimizeResult(x=logexp_finv(theta), fun=-won["lml"], jac=-(won["grad"] * logexp_gradfactor(theta)),
                             nit=won["rounds"], nfev=1 + won["rounds"], status=won["status"], message=won["message"],
                             success=best is not None and won["status"] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL),
                             transform="logexp", optimizer="device", best_run=best, runs=runs)
        m.optimization_result = res
        results[j] = res
    return results


def optimize_together(models, max_iters=1000, transform="logexp", optimizer="host", num_restarts=1, host_fallback=True,
                      device_rows=128):
    """``[m.optimize(max_iters, transform) for m in models]`` with the models' L-BFGS-B runs in lockstep: every round
    evaluates the likelihood and gradients of all models that asked for a value in ONE device call
    (``lml_gradients_batch``).  A model of at most 128 observations follows the trajectory ``optimize`` gives it alone,
    bit for bit, and ends with the same result record; one of 128 < n <= 256 is evaluated by the two-block form without
    a fit (``optimize`` alone refits it and takes the general path): the same likelihood and gradients to rounding.
    Returns the results (``optimization_result`` of each model).
    ``optimizer="device"``: ONE ``cbo_gp_mle_sets`` call runs every model's whole search -- and, with
    ``num_restarts`` > 1, its searches from ``num_restarts - 1`` randomised starts beside the current parameters
    (``mle_restart_starts``, drawn per model in model order before the call) -- at most ``min(max_iters, 4096)`` rounds
    each.  The iteration is ``causal_optimizer.lockstep_lbfgs``', not scipy's: the same stationary points, another
    trajectory.  Per model the best run wins (highest final likelihood, lowest index on ties, a NaN never wins: GPy's
    ``argmin(f_opt)``); the model is set to its parameters, unfitted (``stale``), and its ``optimization_result`` carries
    ``x``, ``fun``, ``jac``, ``nit``, ``status`` / ``message`` (why the winner's search ended, ``_lib.REFINE_*``),
    ``transform="logexp"``, ``optimizer="device"`` and every start's record under ``runs``.  A model whose every run ended
    at a non-finite start keeps its parameters.  A model the call declined (more than 128 observations, fp32,
    ``CBO_HIP_SMALL_SETS=0``) or whose own start has a Ky that is not positive definite as assembled goes through the
    lockstep route described above inside the same call (``host_fallback=False``: RuntimeError instead).
    ``transform="log"`` with ``"device"``, and ``num_restarts`` > 1 with ``"host"``, raise ValueError.
    ``device_rows=256`` (with ``"device"``): the call is ``cbo_gp_mle_sets_rows`` and also takes the fp64 models
    of 129..256 observations -- the same search around the two-block likelihood, restarts included -- so only larger models
    are declined; 128, the default, is the call described above.  Any other value, and 256 with ``"host"``, raise ValueError.
    Models with priors (``set_prior``): both routes minimise ``-log_likelihood - log_prior`` -- the device
    launch adds the prior inside the kernel, the host route through one ``log_prior_batch`` call per round for all models --
    ``fun`` is that objective, the restarts draw such parameters from their priors, and ``transform="log"`` raises
    ValueError."""
    from .utils_functions.lockstep_lbfgsb import lockstep_fmin_l_bfgs_b
    models = list(models)
    checked_mle_optimizer(optimizer, num_restarts)
    checked_mle_device_rows(device_rows, optimizer)
    if optimizer == "device":
        if transform != "logexp":
            raise ValueError("optimizer='device' searches the Logexp-transformed parameters: transform must be 'logexp'")
        if not models:
            return []
        results = _optimize_on_device(models, max_iters, int(num_restarts), host_fallback, int(device_rows))
        rest = [j for j, r in enumerate(results) if r is None]
        for j, r in zip(rest, optimize_together([models[j] for j in rest], max_iters, transform) if rest else []):
            results[j] = r
        return results
    starts = [_optimizer_start(m, transform) for m in models]

    def evaluate(ks, xs):
        values = [None] * len(ks)
        batch = []
        for j, (k, x) in enumerate(zip(ks, xs)):
            m = models[k]
            x = np.asarray(x, dtype=np.float64)
            theta = logexp_f(x) if transform == "logexp" else np.exp(x)
            try:
                _objective_set(m, theta, fit=not _batched(m))
            except np.linalg.LinAlgError:
                values[j] = (1e25, np.zeros_like(x))
                continue
            batch.append((j, k, x, theta))
        answers = lml_gradients_batch([models[k] for _, k, _, _ in batch])
        # the models sit at their thetas: one more call for every model's log prior (none without priors)
        priors = log_prior_batch([models[k] for _, k, _, _ in batch]) if any(_has_priors(models[k]) for _, k, _, _ in batch) \
            else [None] * len(batch)
        for (j, k, x, theta), a, pr in zip(batch, answers, priors):
            pr = pr if _has_priors(models[k]) else None
            values[j] = (1e25, np.zeros_like(x)) if a is None else _objective_value(models[k], theta, *a, transform, pr)
        return values

    runs = lockstep_fmin_l_bfgs_b(evaluate, [x0 for _, x0 in starts], maxfun=int(max_iters), maxiter=int(max_iters))
    # opt_lbfgsb: f_opt = f_fp(x_opt)[0], every model re-evaluated at its x_opt -- one more batched call
    finals = evaluate(list(range(len(models))), [x for x, _, _ in runs])
    return [_optimizer_finish(m, theta0, x_opt, f_final[0], info, transform)
            for m, (theta0, _), (x_opt, _, info), f_final in zip(models, starts, runs, finals)]


def hmc_chains_device(models, theta0s, draws, hmc_iters, stepsize):
    """One ``cbo_gp_hmc_sets`` call: model k's chain from ``theta0s[k]`` with the handed-in ``draws[k]`` = (momenta,
    uniforms).  Returns per model dict(status, rows, accept, theta, lml, grad): rows (num_samples, P), the accept flags, and
    the chain's last state -- everything but ``status`` is meaningless unless it is ``_lib.HMC_OK``.  The models are only
    read."""
    k = len(models)
    lib = _lib.load()
    handles = (ctypes.c_void_p * k)(*[m._handle for m in models])
    chains = (_lib.CboHmcChain * k)()
    status = np.full(k, -1, dtype=np.int32)
    out = []
    for j, (m, theta0, (momenta, uniforms)) in enumerate(zip(models, theta0s, draws)):
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64).reshape(-1)
        momenta = np.ascontiguousarray(momenta, dtype=np.float64)
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
        num, size = uniforms.size, theta0.size
        if momenta.shape != (num, size):
            raise ValueError(f"momenta of model {j} must be ({num}, {size}), not {momenta.shape}")
        o = dict(status=-1, rows=np.zeros((num, size)), accept=np.zeros(num, dtype=np.int32), theta=np.zeros(size),
                 lml=np.zeros(1), grad=np.zeros(size), _keep=(theta0, momenta, uniforms))
        ch = chains[j]
        ch.n_params, ch.sample_noise, ch.num_samples, ch.hmc_iters = size, 0 if m.fix_noise else 1, num, int(hmc_iters)
        ch.stepsize = float(stepsize)
        ch.theta0, ch.momenta, ch.uniforms = _lib.dptr(theta0), _lib.dptr(momenta), _lib.dptr(uniforms)
        ch.rows_out, ch.accept_out = _lib.dptr(o["rows"]), o["accept"].ctypes.data_as(_lib.c_int_p)
        ch.final_theta, ch.final_lml, ch.final_grad = _lib.dptr(o["theta"]), _lib.dptr(o["lml"]), _lib.dptr(o["grad"])
        out.append(o)
    _lib.check(lib.cbo_gp_hmc_sets(k, handles, chains, status.ctypes.data_as(_lib.c_int_p)))
    for o, st in zip(out, status):
        o["status"] = int(st)
        o["lml"] = float(o["lml"][0])
        o["accept"] = o["accept"].astype(bool)
        del o["_keep"]
    return out


def generate_hyperparameters_samples_together(models, n_samples=20, n_burnin=100, subsample_interval=10, step_size=1e-1,
                                              leapfrog_steps=20, host_fallback=True, optimizer="host", num_restarts=1):
    """``[m.generate_hyperparameters_samples(...) for m in models]`` with every model's HMC chain inside ONE device launch
    (``cbo_gp_hmc_sets``): ``optimize_together(models)``; then per model, in order, the 1 % perturbation
    (``randn(P)``) and the chain's draws (``hmc_draws``) -- the generator is consumed exactly as by the per-model sequence,
    ``optimize`` draws nothing --; then the one call.  A model the call declined (more than 128 observations, fp32), or
    whose chain met a Ky that is not positive definite as assembled, is repeated on the host by ``hmc_sample_from_draws``
    on its ``_objective`` with the same draws (``host_fallback=False``: RuntimeError instead).  Returns per model
    ``samples[n_burnin::subsample_interval]``; every model is left at its chain's last state, unfitted (``stale``).
    ``optimizer`` / ``num_restarts`` go to ``optimize_together`` (``"device"``: the MLE in one launch too; its
    restarts are drawn before the chains' numbers)."""
    from .utils_functions.integrated_hyper import hmc_draws, hmc_sample_from_draws
    models = list(models)
    if not models:
        return []
    checked_mle_optimizer(optimizer, num_restarts)
    if optimizer == "device":
        optimize_together(models, optimizer=optimizer, num_restarts=num_restarts, host_fallback=host_fallback)
    else:
        optimize_together(models)
    num = int(n_burnin) + int(n_samples) * int(subsample_interval)
    theta0s, draws = [], []
    for m in models:
        theta0, _ = _optimizer_start(m, "logexp")
        theta0s.append(theta0 * (1.0 + 0.01 * np.random.randn(theta0.size)))
        draws.append(hmc_draws(theta0.size, num))
    answers = hmc_chains_device(models, theta0s, draws, int(leapfrog_steps), float(step_size))
    if not host_fallback:
        for j, a in enumerate(answers):
            if a["status"] != _lib.HMC_OK:
                why = "was declined" if a["status"] == _lib.HMC_DECLINED else \
                    "met a Ky that is not positive definite as assembled"
                raise RuntimeError(f"the device chain of model {j} {why} and host_fallback is off")
    results = []
    for m, theta0, (momenta, uniforms), a in zip(models, theta0s, draws, answers):
        if a["status"] == _lib.HMC_OK:
            samples = a["rows"]
        else:
            samples, _, _ = hmc_sample_from_draws(lambda x, m=m: m._objective(x, "logexp"), theta0, momenta, uniforms,
                                                  int(leapfrog_steps), float(step_size))
        _objective_set(m, samples[-1], fit=False)            # (the chain's last state: the last row, accepted or not)
        results.append(samples[int(n_burnin)::int(subsample_interval)])
    return results


class GaussianProcessFactory:
    """src/GaussianProcessFactory.py:18-73, same static methods."""

    @staticmethod
    def create(gp_type, x, y, parameters=None, emukit_wrapper=False, fit=True, dtype=None, priors=None):
        """``fit=False`` (not in the reference) builds the model without fitting it; the first acquisition sweep
        then refits and sweeps in one overlapped call.  ``dtype="f32"`` (not in the reference either; default from
        ``CBO_HIP_DTYPE``, else "f64") selects the fp32 sweep.  ``priors`` (a dict name -> prior, not in the reference:
        its models have none) are set on the new model (``HipGaussianProcess.set_prior``)."""
        gp_functions = {
            GaussianProcessType.GRAPH_GP: GaussianProcessFactory.create_graph_gp,
            GaussianProcessType.CAUSAL_GP: GaussianProcessFactory.create_causal_gp,
            GaussianProcessType.NON_CAUSAL_GP: GaussianProcessFactory.create_non_causal_gp,
        }
        # emukit_wrapper only selected the wrapper class in the reference; HipGaussianProcess answers
        # both interfaces, so the flag changes nothing here.
        model = gp_functions[gp_type](x, y, parameters, fit=fit, dtype=dtype)
        for name, prior in (priors or {}).items():
            model.set_prior(name, prior)
        return model

    @staticmethod
    def create_graph_gp(x, y, parameters, fit=True, dtype=None):
        """:49-54  RBF(lengthscale=p[0], variance=p[1], ARD=p[3]), noise fixed to 1e-2 after construction."""
        return HipGaussianProcess(x, y, variance=parameters[1], lengthscale=parameters[0], ard=parameters[3],
                                  noise_var=1e-2, fix_noise=True, fit=fit, dtype=dtype)

    @staticmethod
    def create_non_causal_gp(x, y, _, fit=True, dtype=None):
        """:57-60  RBF(lengthscale=1, variance=1), noise 1e-10."""
        return HipGaussianProcess(x, y, variance=1.0, lengthscale=1.0, noise_var=1e-10, fit=fit, dtype=dtype)

    @staticmethod
    def create_causal_gp(x, y, parameters, fit=True, dtype=None):
        """:63-73  CausalRBF(variance_adjustment=var_function) + mean function, noise 1e-10."""
        mean_function, var_function = parameters
        return HipGaussianProcess(x, y, variance=1.0, lengthscale=1.0, noise_var=1e-10,
                                  mean_function=mean_function, variance_adjustment=var_function, fit=fit, dtype=dtype)
