"""Do-calculus prior on the MI355X path: the mean / variance closures the reference
feeds to ``create_causal_gp`` (/root/reference/src/DoCalculus.py:14-89).

For every candidate intervention value the reference builds the observed inputs of a graph-level GP with
the intervened columns overwritten (``get_intervened_inputs``, :80-89), predicts with that GP (:77) and
averages over the observed rows (:59-60) -- a Python loop over candidates with a dict cache.  Here all
candidates go through ONE batched device predict whose per-candidate row means are reduced on the GPU
(``cbo_gp_predict_do``: the intervened inputs are expanded on the device too).  The shipped reference indexes a dict with a list and passes the raw
interventions record instead of the variable names, so this restates the
intended computation, with the exploration-set variable names as the "intervention".
"""
from __future__ import annotations

from functools import partial

import numpy as np


def intervened_inputs(observed, intervened_index, values):
    """(M*N_obs, d_in) inputs: ``observed`` (N_obs, d_in) tiled per candidate, column j replaced by
    ``values[m, intervened_index[j]]`` where ``intervened_index[j] >= 0`` (DoCalculus.py:74-76, 80-89)."""
    observed = np.asarray(observed, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    m, n_obs = values.shape[0], observed.shape[0]
    out = np.broadcast_to(observed[None, :, :], (m, n_obs, observed.shape[1])).copy()
    for j, idx in enumerate(intervened_index):
        if idx >= 0:
            out[:, :, j] = values[:, idx][:, None]
    return out.reshape(m * n_obs, observed.shape[1])


def do_function(gp, observed, intervened_index, index, values):
    """``update_do_function`` for all rows of ``values`` at once: (M,1) mean (index 0) or variance (index 1)
    of the graph GP's predictive distribution averaged over the observed rows."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1:
        values = values[None, :]
    # the (M * N_obs, d) intervened inputs are built on the device from `observed` and `values`
    mean, var = gp.predict_do(observed, intervened_index, values)
    return np.float64(mean if index == 0 else var)


def do_prior_functions(gp, observed, intervened_index):
    """(mean_function, variance_function) for ``GaussianProcessFactory.create_causal_gp``."""
    return (partial(do_function, gp, observed, intervened_index, 0),
            partial(do_function, gp, observed, intervened_index, 1))


def do_prior_clip_ratio(n_g, variance, noise_var):
    """``sn / (n_g sigma^2 + sn)``, ``sn = sigma_n^2 + 1e-8``: the least latent variance of an RBF GP of ``n_g`` rows over
    ``sigma^2`` (all rows placed at the point itself).  ``cbo_do_prior_create`` declines a model below ``DO_PRIOR_CLIP_BOUND``
    (DESIGN.md §4u): the factored form has no per-row clip at 1e-15 as GPy's has."""
    sn = float(noise_var) + 1e-8
    return sn / (float(n_g) * float(variance) + sn)


DO_PRIOR_CLIP_BOUND = 2.0 ** -26        # sqrt(eps): half the digits of a difference of sigma^2-sized terms as margin


class DoPrior:
    """The do-calculus prior of a fitted RBF graph GP as a device-resident handle (``cbo_do_prior``):
    ``evaluate(values)`` is ``gp.predict_do(observed, intervened_index, values)`` at O(n_g^2) per point, and the handle is
    what ``refine_sets(device_prior=True)`` gives the launch for a causal set.  It snapshots the model: rebuild it when the
    graph GP changes.  Raises ``_lib.CboHipError`` (``CBO_ERR_UNSUPPORTED``, the reason in the message) for an fp32 or
    causal graph GP, more than ``_lib.DO_PRIOR_MAX_N`` rows, a model that needed jitter, or the clip rule."""

    def __init__(self, gp, observed, intervened_index):
        import ctypes
        from . import _lib
        observed = _lib.as_f64(observed)
        if observed.ndim != 2 or observed.shape[1] != gp.input_dim or observed.shape[0] < 1:
            raise ValueError(f"observed must be (N_obs, {gp.input_dim}) with N_obs >= 1")
        idx = np.ascontiguousarray(intervened_index, dtype=np.int32)
        if idx.shape != (gp.input_dim,):
            raise ValueError("intervened_index needs one entry per input column")
        if not np.any(idx >= 0):
            raise ValueError("intervened_index marks no column as intervened")
        self.n_iv = int(idx.max()) + 1
        self._lib, self._ctx, self._handle = _lib, gp._ctx, None
        gp.ensure_fitted()
        h = ctypes.c_void_p()
        _lib.check(_lib.load().cbo_do_prior_create(gp._handle, observed.shape[0], _lib.dptr(observed), self.n_iv,
                                                   idx.ctypes.data_as(_lib.c_int_p), ctypes.byref(h)))
        self._handle = h

    def evaluate(self, values):
        """(mean (M,1), var (M,1)) at the rows of ``values`` ((M, n_iv))."""
        if self._handle is None:
            raise ValueError("the prior is closed")
        values = self._lib.as_f64(values)
        if values.ndim == 1:
            values = values[None, :]
        if values.ndim != 2 or values.shape[1] != self.n_iv or values.shape[0] < 1:
            raise ValueError(f"values must be (M, {self.n_iv}) with M >= 1")
        m = values.shape[0]
        mean, var = np.empty(m), np.empty(m)
        self._lib.check(self._lib.load().cbo_do_prior_eval(self._handle, m, self._lib.dptr(values), self._lib.dptr(mean),
                                                           self._lib.dptr(var)))
        return mean[:, None], var[:, None]

    def close(self):
        if self._handle is not None and not self._ctx.closed:
            self._lib.load().cbo_do_prior_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _spec_of_partial(f):
    """(gp, observed, intervened_index, index) of one prior closure, or None."""
    if not isinstance(f, partial) or f.keywords:
        return None
    if f.func is do_function and len(f.args) == 4:
        gp, observed, idx, index = f.args
        return gp, observed, idx, index
    bound = getattr(f.func, "__self__", None)
    if isinstance(bound, DoCalculus) and getattr(f.func, "__func__", None) is DoCalculus.update_do_function \
            and len(f.args) == 3:
        gaussian_processes, intervention, index = f.args
        cbo = bound.cbo
        try:                                   # (what update_do_function itself would look up, and fail on)
            gp = gaussian_processes[cbo.graph.get_gp_name(intervention)]
            input_vars = next(filter(lambda dep: dep[0] == intervention[0], cbo.graph.fit_dependencies))
            observed = np.hstack([np.asarray(cbo.measurements[v], dtype=np.float64).reshape(-1, 1) for v in input_vars])
            idx = [intervention.index(v) if v in intervention else -1 for v in input_vars]
        except (StopIteration, LookupError, TypeError, ValueError, AttributeError):
            return None
        return gp, observed, idx, index
    return None


def prior_spec(model):
    """``(gp, observed, intervened_index)`` of a causal model whose ``mean_function`` / ``variance_adjustment`` are the
    do-calculus closures -- ``functools.partial(do_function, gp, observed, idx, 0 | 1)`` as ``do_prior_functions`` builds them
    (the same first three arguments in both), or the bound partials of ``DoCalculus.update_do_functions`` -- and ``None``
    for anything else (a lambda, another callable, keyword arguments): such a prior can only be evaluated in Python.
    Recognised the way ``cost_structure`` recognises ``graphs.cost``."""
    a = _spec_of_partial(getattr(model, "mean_function", None))
    b = _spec_of_partial(getattr(model, "variance_adjustment", None))
    if a is None or b is None or a[3] != 0 or b[3] != 1:
        return None
    if a[0] is not b[0]:
        return None
    try:
        oa, ob = np.asarray(a[1], dtype=np.float64), np.asarray(b[1], dtype=np.float64)
        ia, ib = [int(v) for v in a[2]], [int(v) for v in b[2]]
    except (TypeError, ValueError):
        return None
    if oa.shape != ob.shape or not np.array_equal(oa, ob) or ia != ib:
        return None
    return a[0], oa, ia


class DoCalculus:
    """Same method names as the reference class.  ``cbo`` must expose ``exploration_set``, ``es_size``,
    ``measurements`` (mapping variable name -> column) and ``graph`` with ``get_gp_name`` and
    ``fit_dependencies`` (as src/graphs/GraphInterface.py and the graph classes provide)."""

    def __init__(self, cbo):
        self.cbo = cbo

    def update_all_do_functions(self, gaussian_processes):
        return [self.update_do_functions(index, gaussian_processes) for index in [0, 1]]

    def update_do_functions(self, index, gaussian_processes):
        return [
            partial(self.update_do_function, gaussian_processes, self.cbo.exploration_set[i], index)
            for i in range(self.cbo.es_size)
        ]

    def update_do_function(self, gaussian_processes, intervention, index, values):
        name = self.cbo.graph.get_gp_name(intervention)
        gp = gaussian_processes[name]
        input_vars = next(filter(lambda dep: dep[0] == intervention[0], self.cbo.graph.fit_dependencies))
        observed = np.hstack([np.asarray(self.cbo.measurements[v], dtype=np.float64).reshape(-1, 1)
                              for v in input_vars])
        intervened_index = [intervention.index(v) if v in intervention else -1 for v in input_vars]
        return do_function(gp, observed, intervened_index, index, values)

    def compute_do(self, measurements, gp, value, input_vars, intervention_vars):
        """DoCalculus.py:68-77 for one value: (mean (N_obs,1), var (N_obs,1)) before the row average."""
        observed = np.hstack([np.asarray(measurements[v], dtype=np.float64).reshape(-1, 1) for v in input_vars])
        idx = [intervention_vars.index(v) if v in intervention_vars else -1 for v in input_vars]
        return gp.predict(intervened_inputs(observed, idx, np.asarray(value, dtype=np.float64)[None, :]))
