"""``find_current_global`` and ``find_next_y_point`` of /root/reference/src/utils_functions/utils.py:8-37
for the MI355X path.  ``find_next_y_point`` keeps the reference signature; the acquisition optimiser
behind it is a dense candidate-grid sweep on the GPU instead of 100 random anchors + L-BFGS
(BASELINE.json configs).
"""
from __future__ import annotations

import os

import numpy as np

from ..graphs import meshgrid_candidates
from .causal_acquisition_functions import CandidateGrid, CausalExpectedImprovement
from .cost_functions import Cost


def find_current_global(current_y, dict_interventions, task):
    """utils.py:8-26: best value observed so far over all exploration sets."""
    dict_values = {}
    for j in range(len(dict_interventions)):
        dict_values[dict_interventions[j]] = []
    for variable, value in current_y.items():
        if len(value) > 0:
            if task == 'min':
                dict_values[variable] = np.min(current_y[variable])
            else:
                dict_values[variable] = np.max(current_y[variable])
    if task == 'min':
        opt_variable = min(dict_values, key=dict_values.get)
    else:
        opt_variable = max(dict_values, key=dict_values.get)
    return dict_values[opt_variable]


def fit_gaussian_process(x, y, parameter_list, optimizer="host", num_restarts=1, device_rows=128):
    """utils.py:40-45: graph-level GP, RBF(lengthscale=p[0], variance=p[1], ARD=p[3]), noise fixed 1e-2.
    ``gp.optimize()`` (hyper-parameter MLE) is called as in the reference.  ``optimizer="device"`` (with
    ``num_restarts`` starts): the one-launch search of DESIGN.md §4v instead; ``device_rows=256`` lets it take a model of
    129..256 rows."""
    from ..GaussianProcessFactory import (GaussianProcessFactory, GaussianProcessType, checked_mle_device_rows,
                                          checked_mle_optimizer, optimize_together)
    checked_mle_device_rows(device_rows, checked_mle_optimizer(optimizer, num_restarts))
    gp = GaussianProcessFactory.create(GaussianProcessType.GRAPH_GP, x, y, parameter_list)
    if optimizer == "device":
        optimize_together([gp], optimizer=optimizer, num_restarts=num_restarts, device_rows=device_rows)
    else:
        gp.optimize()
    return gp


def fit_gaussian_processes(xs, ys, parameter_lists, lockstep=True, optimizer="host", num_restarts=1, device_rows=128):
    """``[fit_gaussian_process(x, y, p) for ...]`` -- the graph-level GPs of an observe step -- with the hyper-parameter
    MLEs run together: every round of the models' L-BFGS-B runs is ONE device call for all of them
    (``GaussianProcessFactory.optimize_together``).  Models of at most 128 rows get the trajectories and results of
    fitting them one by one, bit for bit; those of 128 < n <= 256 are evaluated by the device's two-block form without
    refits (the same values to rounding).  ``lockstep=False`` fits them one by one.  ``optimizer="device"`` (with
    ``num_restarts`` starts per model): every model's whole search in ONE device launch, whatever
    ``lockstep`` says; ``device_rows=256``: models of 129..256 rows inside that launch too."""
    from ..GaussianProcessFactory import (GaussianProcessFactory, GaussianProcessType, checked_mle_device_rows,
                                          checked_mle_optimizer, optimize_together)
    checked_mle_device_rows(device_rows, checked_mle_optimizer(optimizer, num_restarts))
    if optimizer == "device":
        models = [GaussianProcessFactory.create(GaussianProcessType.GRAPH_GP, x, y, p)
                  for x, y, p in zip(xs, ys, parameter_lists)]
        optimize_together(models, optimizer=optimizer, num_restarts=num_restarts, device_rows=device_rows)
        return models
    if not lockstep:
        return [fit_gaussian_process(x, y, p) for x, y, p in zip(xs, ys, parameter_lists)]
    models = [GaussianProcessFactory.create(GaussianProcessType.GRAPH_GP, x, y, p)
              for x, y, p in zip(xs, ys, parameter_lists)]
    optimize_together(models)
    return models


def update_hull(observational_samples, manipulative_variables):
    """src/utils_functions/cbo_functions.py:7-17: volume of the convex hull of the observations of the manipulative
    variables (``observational_samples[v]`` a column per variable)."""
    from scipy.spatial import ConvexHull
    stack = np.column_stack([np.asarray(observational_samples[v], dtype=np.float64).reshape(-1)
                             for v in manipulative_variables])
    return ConvexHull(stack).volume


def compute_coverage(observational_samples, manipulative_variables, dict_ranges):
    """src/utils_functions/cbo_functions.py:26-41: (coverage of the observations' hull over the box of the interventional
    ranges, the observations' hull, the box's volume)."""
    import itertools
    from scipy.spatial import ConvexHull
    vertices = list(itertools.product(*[dict_ranges[v] for v in manipulative_variables]))
    coverage_total = ConvexHull(vertices).volume
    stack = np.column_stack([np.asarray(observational_samples[v], dtype=np.float64).reshape(-1)
                             for v in manipulative_variables])
    hull_obs = ConvexHull(stack)
    return hull_obs.volume / coverage_total, hull_obs, coverage_total


def space_bounds(space):
    """[(lo, hi)] from an emukit ParameterSpace (``get_bounds()``), from objects with ``.parameters``
    carrying ``.min/.max`` (graph_functions.py:80-93 builds ContinuousParameter(name, min, max)), or
    from a plain list of pairs."""
    if hasattr(space, "get_bounds"):
        return [tuple(b) for b in space.get_bounds()]
    if hasattr(space, "parameters"):
        return [(p.min, p.max) for p in space.parameters]
    return [tuple(b) for b in space]


def default_grid_shape(d, budget=None):
    """Points per dimension for a d-dimensional sweep.  BASELINE.json: 200 per 1-D toy set, and the
    16k grid 32x32x16 for d=3; other d get the largest equal split within the same 16k budget."""
    if budget is None:
        budget = int(os.environ.get("CBO_HIP_GRID_BUDGET", "16384"))
    if d == 1:
        return [min(budget, 200)]
    if d == 3 and budget == 16384:
        return [32, 32, 16]
    n = max(2, int(np.floor(budget ** (1.0 / d))))
    return [n] * d


def find_next_y_point(space, model, current_global_best, evaluated_set, costs_functions, task='min',
                      grid_shape=None, candidates=None, anchors="grid", num_anchor_points=None, acquisition="EI",
                      batch_size=None, hyper_samples=None, cost_mode="batch", constraints=None):
    """utils.py:29-37.  Returns (y_acquisition (1,1), x_new (1,d)).

    ``candidates`` (optional (M,d) array or CandidateGrid) overrides the regular grid over ``space``.
    ``anchors="uniform"``: the reference's own optimiser instead of the grid -- 100 uniform anchors from numpy's global
    generator, one batched device sweep over them, L-BFGS from the best (causal_optimizer.py:26-65), then the
    acquisition re-evaluated at the point found (utils.py:36) -- the four lines of the reference's function.
    ``acquisition="MES"``: emukit's ``MaxValueEntropySearch(model, space) / Cost`` over the same grid in the place of the
    causal EI (its Gumbel fit draws from numpy's global generator; ``current_global_best`` is not used).  MES minimises and
    has no gradients: ``task="max"`` and ``anchors="uniform"`` raise ``ValueError``.
    ``constraints`` (a list of ``ProbabilityOfFeasibility``, each over the model of a node that must stay in range): the
    grid is scored with ``EI * prod PoF / Cost`` in one device call (constrained.py); together with
    ``acquisition="MES"`` or ``anchors="uniform"`` it raises ``ValueError``.  ``None``: nothing changes.
    ``batch_size`` (a positive int): greedy batch selection over the grid (greedy_batch.py, one ``cbo_acq_sweep_batch``
    call): returns (y (B,1), x (B,d)), row 0 being the single-point result; together with ``acquisition="MES"``,
    ``constraints`` or ``anchors="uniform"`` it raises ``ValueError``.  ``None``: nothing changes.
    ``acquisition="LCB" | "PI" | "MPEI" | "VAR"``: the point-wise acquisitions of pointwise_acquisitions.py -- emukit's
    ``NegativeLowerConfidenceBound`` (beta 1), ``ProbabilityOfImprovement``, ``MeanPluginExpectedImprovement`` and
    ``ModelVariance`` -- over the cost, on the grid or with ``anchors="uniform"`` (they have gradients).  ``"MPEI"`` and
    ``"VAR"`` do not use ``current_global_best``, ``"VAR"`` does not use ``task``.  Together with ``constraints``,
    ``batch_size`` or ``hyper_samples`` they raise those branches' ``ValueError``.
    ``acquisition="LOGEI"``: the logarithm of the causal EI, computed without underflow, minus the logarithm of the cost
    (``CausalLogExpectedImprovement / Cost``), on the grid or with ``anchors="uniform"``; together with
    ``constraints``, ``batch_size`` or ``hyper_samples`` it raises those branches' ``ValueError``.
    ``hyper_samples`` (an (H, P) array of hyper-parameter samples, or an int: that many drawn by the model's HMC with the
    defaults): the grid is scored with the EI marginalised over the samples, over the cost, in one device call
    (integrated_hyper.py, ``cbo_acq_sweep_hyper``); together with ``acquisition="MES"``, ``constraints``, ``batch_size`` or
    ``anchors="uniform"`` it raises ``ValueError``.  ``None``: nothing changes.
    ``cost_mode="pointwise"``: every candidate is scored over its OWN cost, ``EI(x) / c(x)`` or, with
    ``acquisition="LOGEI"``, ``log EI(x) - log c(x)`` (``acquisition / PointwiseCost``, ``cbo_acq_sweep_pointcost``); the value
    returned is the winner's own, with no re-pricing step.  Another acquisition, ``constraints``, ``hyper_samples``,
    ``batch_size`` and a cost table ``cost_structure`` does not recognise raise ``ValueError`` before any device call.
    ``"batch"`` (default) is the reference's one scalar per batch: nothing changes.
    ``acquisition="LOGCEI"`` with ``constraints``: the constrained acquisition in log space, ``log EI + sum
    log PoF - log cost`` (``ConstrainedLogExpectedImprovement / Cost``, ``cbo_acq_sweep_constrained_log``) -- finite and
    ordered where ``EI * prod PoF`` is an exact 0.  An empty list scores ``"LOGEI"``'s bits; ``constraints=None``,
    ``hyper_samples``, ``batch_size``, ``cost_mode="pointwise"`` and ``anchors="uniform"`` raise ``ValueError`` before any
    device call.
    ``acquisition="LOGMEI"`` with ``hyper_samples``: the marginalised EI in log space, ``log((1 / H) sum_h
    EI_h) - log cost`` (``IntegratedHyperParameterAcquisition`` over a ``CausalLogExpectedImprovement`` generator,
    ``cbo_acq_sweep_hyper_log``) -- the logarithm of the average ``hyper_samples`` with ``"EI"`` scores, not the average of the
    logarithms; finite and ordered where that average is an exact 0.  Without ``hyper_samples``, or with ``constraints``,
    ``batch_size``, ``cost_mode="pointwise"`` or ``anchors="uniform"``, it raises ``ValueError`` before any device call.
    ``acquisition="LOGBEI"`` with ``batch_size``: the greedy batch scored in log space -- the same believer,
    every pick's score ``log EI - log cost`` (``CausalLogExpectedImprovement.sweep_batch``, ``cbo_acq_sweep_batch_logei``):
    finite and ordered where the EI of every pick is an exact 0 and ``"EI"`` returns candidate 0 ``batch_size`` times.
    Without ``batch_size`` (the acquisition is then ``"LOGEI"``), or with ``constraints``, ``hyper_samples``,
    ``cost_mode="pointwise"`` or ``anchors="uniform"``, it raises ``ValueError`` before any device call.
    """
    checked_log_bei((acquisition, None), batch_size, constraints, hyper_samples, cost_mode=cost_mode, anchors=anchors)
    checked_log_mei((acquisition, None), hyper_samples, constraints, batch_size, cost_mode=cost_mode, anchors=anchors)
    checked_log_cei((acquisition, None), constraints, hyper_samples, batch_size, cost_mode=cost_mode, anchors=anchors)
    if checked_pointwise_cost(cost_mode, (acquisition, None), constraints, hyper_samples, batch_size):
        from .cost_functions import PointwiseCost
        quotient = _acquisition_for(acquisition, model, current_global_best, task, space) / \
            PointwiseCost(costs_functions, evaluated_set)
        if anchors == "uniform":
            from .causal_optimizer import CausalGradientAcquisitionOptimizer
            optimizer = CausalGradientAcquisitionOptimizer(space, num_anchor_points=num_anchor_points, anchors="uniform")
            x_new, _ = optimizer.optimize(quotient)
            return quotient.evaluate(x_new), x_new
        own = not isinstance(candidates, CandidateGrid)
        if candidates is None:
            bounds = space_bounds(space)
            candidates = meshgrid_candidates(bounds, grid_shape or default_grid_shape(len(bounds)))
        grid = CandidateGrid(candidates, model) if own else candidates
        try:
            res = quotient.sweep(grid)
            x_new = grid.points[res["best_idx"] - grid.index_offset][None, :].copy()
        finally:
            if own:
                grid.close()
        return np.array([[res["best_val"]]]), x_new
    if hyper_samples is not None:
        if acquisition not in ("EI", LOG_MEI):
            raise ValueError("hyper-parameter samples marginalise the causal EI: acquisition must be 'EI' (or 'LOGMEI', the "
                             "logarithm of the average)")
        if constraints is not None:
            raise ValueError("the marginalised EI is not defined with constraints: constraints must be None")
        if batch_size is not None:
            raise ValueError("the marginalised EI picks one point: batch_size must be None")
        if anchors != "grid":
            raise ValueError("the marginalised EI is scored over the grid: anchors must be 'grid'")
        if isinstance(hyper_samples, bool) or (isinstance(hyper_samples, (int, np.integer)) and hyper_samples < 1):
            raise ValueError(f"hyper_samples must be an (H, P) array or a positive int, not {hyper_samples!r}")
    if batch_size is not None:
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f"batch_size must be a positive int, not {batch_size!r}")
        if acquisition not in ("EI", LOG_BEI):
            raise ValueError("batch selection believes the causal EI's model: acquisition must be 'EI' (or 'LOGBEI', the "
                             "same batch scored in log space)")
        if constraints is not None:
            raise ValueError("batch selection is not defined for constrained acquisitions: constraints must be None")
        if anchors != "grid":
            raise ValueError("batch selection picks from the grid: anchors must be 'grid'")
    if acquisition not in ("EI", "MES", LOG_EI, LOG_CEI, LOG_MEI, LOG_BEI) + POINTWISE_ACQUISITIONS:
        raise ValueError(f"acquisition must be 'EI', 'MES', 'LCB', 'PI', 'MPEI' or 'VAR', not {acquisition!r}")
    if acquisition == "MES":
        if task != "min":
            raise ValueError("acquisition='MES' minimises: task must be 'min'")
        if anchors != "grid":
            raise ValueError("acquisition='MES' has no gradients: anchors must be 'grid'")
    if constraints is not None:
        if acquisition not in ("EI", LOG_CEI):
            raise ValueError("constraints multiply the causal EI: acquisition must be 'EI' (or 'LOGCEI', the sum of the "
                             "logarithms)")
        if anchors != "grid":
            raise ValueError("constraints are scored over the grid: anchors must be 'grid'")
    cost_acquisition = Cost(costs_functions, evaluated_set)
    if anchors == "uniform":
        from .causal_optimizer import CausalGradientAcquisitionOptimizer
        optimizer = CausalGradientAcquisitionOptimizer(space, num_anchor_points=num_anchor_points, anchors="uniform")
        acquisition = _acquisition_for(acquisition, model, current_global_best, task, space) / cost_acquisition
        x_new, _ = optimizer.optimize(acquisition)
        return acquisition.evaluate(x_new), x_new
    ei = _acquisition_for(acquisition, model, current_global_best, task, space)
    if constraints:
        from .constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement
        # the sets of the constraints' models follow the grid's
        ei = (ConstrainedLogExpectedImprovement(ei, constraints) if acquisition == LOG_CEI
              else AcquisitionProduct([ei] + list(constraints)))
    if hyper_samples is not None:
        from .integrated_hyper import IntegratedHyperParameterAcquisition
        if acquisition == LOG_MEI:
            generator = lambda mdl: _acquisition_for(LOG_EI, mdl, current_global_best, task, space)      # noqa: E731
        else:
            generator = lambda mdl: CausalExpectedImprovement(current_global_best, task, mdl)      # noqa: E731
        if isinstance(hyper_samples, (int, np.integer)):
            ei = IntegratedHyperParameterAcquisition(model, generator, n_samples=int(hyper_samples))
        else:
            ei = IntegratedHyperParameterAcquisition(model, generator, samples=hyper_samples)
    own = False
    if candidates is None:
        bounds = space_bounds(space)
        pts = meshgrid_candidates(bounds, grid_shape or default_grid_shape(len(bounds)))
        grid, own = CandidateGrid(pts, model), True
    elif isinstance(candidates, CandidateGrid):
        grid = candidates
    else:
        grid, own = CandidateGrid(candidates, model), True
    try:
        batch_cost = float(cost_acquisition.evaluate(grid.points))      # ONE scalar for the batch (Quotient)
        if batch_size is not None:
            return _next_y_points_batch(ei, grid, cost_acquisition, batch_cost, int(batch_size), acquisition == LOG_BEI)
        res = ei.sweep(grid, cost=batch_cost)
        x_new = grid.points[res["best_idx"] - grid.index_offset][None, :].copy()
        # utils.py:36 re-evaluates the acquisition at x_new alone; only variable costs change the value
        point_cost = float(cost_acquisition.evaluate(x_new))
        if point_cost == batch_cost:
            y = np.array([[res["best_val"]]])
        else:
            y = ei.sweep(x_new, cost=point_cost, want_acq=True)["acq"]
    finally:
        if constraints:
            ei.close()
        if own:
            grid.close()
    return y, x_new


POINTWISE_ACQUISITIONS = ("LCB", "PI", "MPEI", "VAR")
LOG_EI = "LOGEI"      # the log Expected Improvement: a name of its own, routed to the cbo_acq_*_logei calls
LOG_CEI = "LOGCEI"    # log EI + sum log PoF - log cost: routed by name to the cbo_acq_*_constrained_log calls
LOG_MEI = "LOGMEI"    # log((1 / H) sum_h EI_h) - log cost: routed by name to the cbo_acq_sweep*_hyper_log calls
LOG_BEI = "LOGBEI"    # the Kriging-believer batch on log EI - log cost: routed by name to cbo_acq_sweep*_batch_logei


def _acquisition_for(name, model, current_global_best, task, space, param=None):
    """The acquisition object ``find_next_y_point(acquisition=name)`` scores with (defaults: beta 1, jitter 0; ``param``
    replaces the default of a point-wise kind that has one)."""
    if name == "MES":
        from .max_value_entropy import MaxValueEntropySearch
        return MaxValueEntropySearch(model, space)
    if name in (LOG_EI, LOG_CEI, LOG_BEI):         # (LOGCEI's objective; its constraints are the caller's to add.  LOGBEI's picks)
        from .pointwise_acquisitions import CausalLogExpectedImprovement
        return CausalLogExpectedImprovement(current_global_best, task, model, 0.0 if param is None else param)
    if name in POINTWISE_ACQUISITIONS:
        from . import pointwise_acquisitions as pw
        extra = () if param is None else (param,)
        if name == "LCB":
            return pw.CausalNegativeLowerConfidenceBound(task, model, *extra)
        if name == "PI":
            return pw.CausalProbabilityOfImprovement(current_global_best, task, model, *extra)
        if name == "MPEI":
            return pw.CausalMeanPluginExpectedImprovement(task, model, *extra)
        return pw.ModelVariance(model)
    return CausalExpectedImprovement(current_global_best, task, model)


def sets_acquisition(acquisition="EI", acquisition_param=None):
    """(name, parameter) of the acquisition a multi-set sweep scores with, checked on the host before any device call:
    ``"EI"`` (no parameter: today's call, ``None``), ``"LCB"`` (beta, default 1, finite and not negative), ``"PI"`` and
    ``"MPEI"`` (the jitter, default 0, finite), ``"LOGEI"`` (the log Expected Improvement of DESIGN.md §4x: the jitter, as
    PI's), ``"LOGCEI"`` (its constrained form, DESIGN.md §4aa: the log EI's jitter, checked as LOGEI's), ``"LOGMEI"`` (its
    hyper-marginalised form, DESIGN.md §4ac: the log EI's jitter, checked as LOGEI's), ``"LOGBEI"`` (its greedy batch, DESIGN.md
    §4ad: the log EI's jitter, checked as LOGEI's; the callers require a ``batch_size`` with it), ``"VAR"`` (no
    parameter: 0 travels), ``"MES"`` with a pair of ints ``(num_samples, grid_size)``, ``num_samples`` in 1..64,
    ``grid_size`` at least 1 (the parameter returned is that pair).
    Anything else raises ``ValueError`` -- a bare ``"MES"`` too: this function never answered for it and has no default for
    it; ``sets_acquisition_or_default`` -- what ``find_next_y_points``, ``CBOAcquisitionPath`` and ``CBO`` call -- puts
    emukit's defaults (10 samples, a Gumbel grid of 5000) in the place of a ``None`` first.
    An answer of this function is accepted in the place of the name (and returned as it is)."""
    import math
    if type(acquisition) is tuple and acquisition_param is None and len(acquisition) == 2:
        name, param = acquisition                 # an earlier answer of this function (a path keeps its own): checked again
        sets_acquisition(name, None if name in ("EI", "VAR") else param)
        return acquisition
    if not isinstance(acquisition, str) \
            or acquisition not in ("EI", "MES", LOG_EI, LOG_CEI, LOG_MEI, LOG_BEI) + POINTWISE_ACQUISITIONS:
        raise ValueError("acquisition must be 'EI', 'MES', 'LCB', 'PI', 'MPEI' or 'VAR' in a multi-set sweep, "
                         f"not {acquisition!r}")
    if acquisition == "MES":
        if acquisition_param is None:
            raise ValueError("acquisition must be 'EI', 'LCB', 'PI', 'MPEI' or 'VAR' -- or 'MES' with acquisition_param = "
                             "(num_samples, grid_size) -- in a multi-set sweep")
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))      # noqa: E731
        if not isinstance(acquisition_param, (tuple, list)) or len(acquisition_param) != 2 \
                or not all(is_int(v) for v in acquisition_param):
            raise ValueError("acquisition_param (num_samples, grid_size) must be a pair of ints, "
                             f"not {acquisition_param!r}")
        num_samples, grid_size = int(acquisition_param[0]), int(acquisition_param[1])
        if not 1 <= num_samples <= 64:
            raise ValueError(f"acquisition_param: num_samples must be in 1..64, not {num_samples}")
        if grid_size < 1:
            raise ValueError(f"acquisition_param: grid_size must be at least 1, not {grid_size}")
        return "MES", (num_samples, grid_size)
    if acquisition == "EI":
        if acquisition_param is not None:
            raise ValueError("acquisition_param: the multi-set EI takes none (its jitter is the reference's 0)")
        return "EI", None
    what = "acquisition_param (beta)" if acquisition == "LCB" else "acquisition_param (jitter)"
    if acquisition_param is None:
        return acquisition, (1.0 if acquisition == "LCB" else 0.0)
    if acquisition == "VAR":
        raise ValueError("acquisition_param: the model variance takes none")
    try:
        param = float(np.asarray(acquisition_param, dtype=np.float64).reshape(-1)[0])
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"{what} must be a finite number, not {acquisition_param!r}") from None
    if not math.isfinite(param):
        raise ValueError(f"{what} must be a finite number, not {acquisition_param!r}")
    if acquisition == "LCB" and param < 0.0:
        raise ValueError(f"{what} must not be negative, not {acquisition_param!r}")
    return acquisition, param


MES_DEFAULTS = (10, 5000)          # emukit's MaxValueEntropySearch: num_samples, grid_size


def sets_acquisition_or_default(acquisition="EI", acquisition_param=None):
    """``sets_acquisition`` with emukit's defaults for ``"MES"`` where no parameter was given: what the callers that take
    ``acquisition`` / ``acquisition_param`` from a user (``find_next_y_points``, ``CBOAcquisitionPath``, ``CBO``) call."""
    if isinstance(acquisition, str) and acquisition == "MES" and acquisition_param is None:
        acquisition_param = MES_DEFAULTS
    return sets_acquisition(acquisition, acquisition_param)


def _repriced(value, batch_cost, point_cost, log_form):
    """A later pick's value moved from the batch's cost to the point's own: the quotient rescaled, or -- the log form,
    ``log EI - log cost`` -- the two logarithms exchanged."""
    if log_form:
        return (value + np.log(batch_cost)) - np.log(point_cost)
    return value * batch_cost / point_cost


def _next_y_points_batch(ei, grid, cost_acquisition, batch_cost, batch_size, log_form=False):
    """``find_next_y_point(batch_size=B)``: (y (B,1), x (B,d)) of one ``sweep_batch``.  y[t] is the pick's acquisition over
    the point's own cost where variable costs make that differ from the batch's (utils.py:36): pick 0 by the single-point
    path's re-evaluation, the later picks -- whose believed model exists on the device only -- by rescaling (``_repriced``)."""
    res = ei.sweep_batch(grid, batch_size, cost=batch_cost)
    x_new = grid.points[res["best_idx"] - grid.index_offset].copy()
    y = np.asarray(res["best_val"], dtype=np.float64).reshape(-1, 1).copy()
    for t in range(batch_size):
        point_cost = float(cost_acquisition.evaluate(x_new[t:t + 1]))
        if point_cost != batch_cost:
            y[t, 0] = (ei.sweep(x_new[t:t + 1], cost=point_cost, want_acq=True)["acq"][0, 0] if t == 0
                       else _repriced(y[t, 0], batch_cost, point_cost, log_form))
    return y, x_new


def find_next_y_points(models, current_global_best, evaluated_sets, costs_functions, task, grids, cache=None, raw=False,
                       acquisition="EI", acquisition_param=None, hyper_samples=None, spaces=None, batch_size=None,
                       update_incumbent=False, refine=False, device_prior=False, cost_mode="batch", refine_constrained=False,
                       constraints=None):
    """``find_next_y_point`` for every exploration set of a trial in ONE device call (``cbo_acq_sweep_sets``): the loop
    of src/CBO.py:249-257.  ``grids[s]`` is the CandidateGrid of set s.  Models with at most 128 observations -- all
    the reference builds -- are factored and swept inside one launch and need not be fitted; the others go through
    the general path inside the same call.  ``cache`` (a dict the caller keeps between trials) holds what does not
    change while models, grids and cost functions stay the same objects: the handle arrays and the batch costs.
    Returns (xs, ys): lists of (1,d) points and (1,1) acquisition values.  ``raw=True`` (the multi-GPU caller): the
    batch costs are given (``costs_functions.values``, those of the whole grid) and ys are (value, global index)
    pairs for the arg-max exchange, xs is None.
    ``acquisition="LCB" | "PI" | "MPEI" | "VAR"`` with ``acquisition_param`` (beta, default 1; the jitter of PI and MPEI,
    default 0): the point-wise acquisitions of ``find_next_y_point`` in the same one call (``cbo_acq_sweep_sets_kind``,
    DESIGN.md §4l) -- per set what ``find_next_y_point(acquisition=...)`` returns.  ``"EI"`` is today's call, untouched.  The
    cache entry records the kind: a changed kind rebuilds nothing but the call.  Unknown names, a negative beta and a
    non-finite parameter raise ``ValueError`` before any device call.
    ``constraints`` (one entry per set, each a possibly empty list of ``ProbabilityOfFeasibility``): every set is scored with
    ``EI * prod PoF / cost`` in the same one call (``cbo_acq_sweep_sets_constrained``) -- per set what
    ``find_next_y_point(constraints=[...])`` returns.  Each constraint model gets a ``CandidateGrid`` over the set's own grid
    points with the set's ``index_offset``, built once and kept in the cache entry while the model object stays the same.
    Non-empty constraints with another ``acquisition`` than ``"EI"`` or with ``raw=True``, a wrong length, more than 8
    constraints in a set and a non-finite ``max_value`` or ``jitter`` raise ``ValueError`` before any device call.  ``None``,
    or every list empty, takes exactly today's calls.
    ``hyper_samples`` (one entry per set, each an (H_s, P_s) array of hyper-parameter samples in GPy's parameter order -- a
    model whose noise is fixed has no noise column -- or a positive int: every model then draws that many with
    ``generate_hyperparameters_samples``): every set is scored with the causal EI marginalised over its own samples, over
    the cost, in the same one call (``cbo_acq_sweep_sets_hyper``) -- per set what
    ``find_next_y_point(hyper_samples=rows_s)`` returns.  A wrong length, a bad shape, more than 256 rows, non-finite or
    non-positive entries, another ``acquisition`` than ``"EI"``, non-empty ``constraints`` and ``raw=True`` raise
    ``ValueError`` before any device call.  ``None`` takes exactly today's calls.
    ``acquisition="MES"`` with ``acquisition_param`` (``None``: 10 samples, a Gumbel grid of 5000; or ``(num_samples,
    grid_size)``) and ``spaces`` (one entry per set, as ``space_bounds`` accepts): emukit's ``MaxValueEntropySearch(model,
    space) / Cost`` for every set in two device calls -- ``max_value_entropy.mes_sets_parameters`` (every
    set's Gumbel fit, ``cbo_gp_mes_gumbel_sets``; it draws from numpy's global generator in the order documented there),
    then ``cbo_acq_sweep_sets_mes``.  ``task`` other than ``"min"``, missing ``spaces``, ``raw=True``, non-empty
    ``constraints`` and ``hyper_samples`` raise ``ValueError`` before any device call.
    ``batch_size`` (a positive int B, at most 64 and at most every grid's size) with ``update_incumbent``: greedy batch
    selection for every set in ONE device call (``cbo_acq_sweep_sets_batch``) -- per set what
    ``find_next_y_point(batch_size=B)`` returns: ``xs[s]`` is (B, d), ``ys[s]`` (B, 1), row 0 the single-point result.  Under
    variable costs ``ys[s][0]`` is today's re-evaluation and the later picks are rescaled from the batch cost to the point's
    own.  Another ``acquisition`` than ``"EI"``, non-empty ``constraints``, ``hyper_samples`` and ``raw=True`` raise
    ``ValueError`` before any device call.  ``None`` takes exactly today's calls.
    ``refine=True`` with ``spaces`` (one entry per set): the reference's second stage (causal_optimizer.py:59-65) -- every
    set's winner is the start of an L-BFGS ascent inside the set's box, all of them in one further device call
    (``causal_optimizer.refine_sets``; sets the launch does not take go through ``refine_batched``).  The
    refined point replaces the winner only if its value, priced at its own cost, is not lower.  ``refine=True`` with
    ``"MES"``, non-empty ``constraints``, ``hyper_samples``, ``batch_size`` or ``raw=True``, or without ``spaces``, raises
    ``ValueError`` before any device call.  ``False`` takes exactly today's calls.
    ``device_prior=True`` (with ``refine=True``; ``ValueError`` without): a causal set whose prior closures are the do-calculus
    closures joins the refinement's device launch through a device-resident prior (``refine_sets(device_prior=True)``,
    DESIGN.md §4u) instead of ``refine_batched``.  ``False`` takes exactly today's calls.
    ``acquisition="LOGEI"`` with ``acquisition_param`` (the jitter, default 0): the log Expected Improvement minus the
    logarithm of the cost for every set in the same one call (``cbo_acq_sweep_sets_logei``) -- per set what
    ``find_next_y_point(acquisition="LOGEI")`` returns -- and, with ``refine=True``, refined by ``cbo_acq_refine_sets_logei``
    (causal sets through the host route).  Together with non-empty ``constraints``, ``hyper_samples``, ``batch_size``,
    ``device_prior=True`` or ``raw=True`` it raises ``ValueError`` before any device call.
    ``cost_mode="pointwise"`` with ``"EI"`` or ``"LOGEI"``: every candidate over its own cost for every set in
    one call (``cbo_acq_sweep_sets_pointcost``) -- per set what ``find_next_y_point(cost_mode="pointwise")`` returns, the
    winner's value being its own ``EI / c(x)`` with no re-pricing -- and, with ``refine=True``, refined with the cost's own
    gradient (``refine_sets(cost_mode="pointwise")``).  Another acquisition, non-empty ``constraints``, ``hyper_samples``,
    ``batch_size``, ``device_prior=True``, ``raw=True`` and a cost ``cost_structure`` does not recognise raise ``ValueError``
    before any device call.  ``"batch"`` (default) takes exactly today's calls.
    ``acquisition="LOGCEI"`` with ``acquisition_param`` (the log EI's jitter, default 0) and ``constraints``:
    every set is scored with ``log EI + sum log PoF - log cost`` in the same one call
    (``cbo_acq_sweep_sets_constrained_log``) -- per set what ``find_next_y_point(acquisition="LOGCEI", constraints=[...])``
    returns; a set with an empty list scores ``"LOGEI"``'s bits.  ``constraints=None``, ``hyper_samples``, ``batch_size``,
    ``refine=True``, ``device_prior=True``, ``cost_mode="pointwise"`` and ``raw=True`` raise ``ValueError`` before any device
    call.
    ``refine_constrained=True`` with ``acquisition`` ``"EI"`` or ``"LOGCEI"``, non-empty ``constraints`` and
    ``spaces``: every set's constrained winner is the start of an L-BFGS ascent of the constrained acquisition inside the set's
    box, all of them in one further device call (``refine_sets(constraints=...)``, ``cbo_acq_refine_sets_constrained``; sets the
    launch does not take go through ``refine_batched``).  The refined point replaces the winner only if its value at its own
    cost is not lower.  Another acquisition, ``constraints`` that are ``None`` or all empty, missing ``spaces``, ``raw=True``,
    ``hyper_samples``, ``batch_size``, ``device_prior=True`` and ``cost_mode="pointwise"`` raise ``ValueError`` before any device
    call.  ``False`` takes exactly today's calls; ``refine=True`` with constraints keeps raising.
    ``acquisition="LOGMEI"`` with ``acquisition_param`` (the log EI's jitter, default 0) and ``hyper_samples`` (DESIGN.md
    §4ac): every set's score is the LOGARITHM of the EI marginalised over its samples, ``log((1 / H) sum_h EI_h) - log cost``
    -- not the average of the logarithms -- in the same one call (``cbo_acq_sweep_sets_hyper_log``): per set what
    ``find_next_y_point(acquisition="LOGMEI", hyper_samples=rows_s)`` returns, finite and ordered where the marginalised EI
    is an exact 0.  Without ``hyper_samples``, or with non-empty ``constraints``, ``batch_size``, ``refine``,
    ``refine_constrained``, ``device_prior``, ``cost_mode="pointwise"`` or ``raw=True``, it raises ``ValueError`` before any
    device call.
    ``acquisition="LOGBEI"`` with ``acquisition_param`` (the log EI's jitter, default 0), ``batch_size`` and
    ``update_incumbent``: every set's greedy batch scored in log space in ONE device call
    (``cbo_acq_sweep_sets_batch_logei``) -- per set what ``find_next_y_point(acquisition="LOGBEI", batch_size=B)`` returns,
    distinct and ordered picks where ``"EI"`` with a ``batch_size`` returns candidate 0 B times.  Without ``batch_size``, or
    with non-empty ``constraints``, ``hyper_samples``, ``refine``, ``refine_constrained``, ``device_prior``,
    ``cost_mode="pointwise"`` or ``raw=True``, it raises ``ValueError`` before any device call."""
    import ctypes
    from .. import _lib
    kind = sets_acquisition_or_default(acquisition, acquisition_param)
    checked_log_bei(kind, batch_size, constraints, hyper_samples, refine, refine_constrained, device_prior, raw, cost_mode)
    checked_log_mei(kind, hyper_samples, constraints, batch_size, refine, refine_constrained, device_prior, raw, cost_mode)
    checked_refine_constrained(refine_constrained, kind, constraints, hyper_samples, batch_size, raw, spaces, len(models),
                               device_prior, cost_mode)
    checked_log_cei(kind, constraints, hyper_samples, batch_size, refine, device_prior, raw, cost_mode)
    if checked_pointwise_cost(cost_mode, kind, constraints, hyper_samples, batch_size, device_prior, raw):
        checked_refine(refine, kind, None, None, None, False, spaces, len(models))
        return _next_y_points_pointwise(models, current_global_best, evaluated_sets, costs_functions, task, grids, kind,
                                        refine, spaces)
    checked_device_prior(device_prior, refine)
    checked_log_ei(kind, device_prior, raw)
    checked_refine(refine, kind, constraints, hyper_samples, batch_size, raw, spaces, len(models))
    batch_size = checked_batch_size(batch_size, kind, constraints, hyper_samples, raw)
    if batch_size is not None and task not in _lib.TASK_CODE:
        raise ValueError(f"task must be 'min' or 'max', not {task!r}")
    if kind[0] == "MES":
        if task != "min":
            raise ValueError("acquisition='MES' minimises: task must be 'min'")
        if spaces is None or not hasattr(spaces, "__len__") or len(spaces) != len(models):
            raise ValueError(f"acquisition='MES' draws its Gumbel grids from the sets' spaces: spaces must have one entry per "
                             f"exploration set ({len(models)})")
        if raw:
            raise ValueError("acquisition='MES' is not defined across several ranks (raw=True)")
    constraints = checked_set_constraints(constraints, len(models), kind, raw)
    hyper_rows = checked_set_hyper_samples(hyper_samples, models, kind, constraints, raw)
    if kind[0] != "EI" and task not in _lib.TASK_CODE:
        raise ValueError(f"task must be 'min' or 'max', not {task!r}")
    s = len(models)
    # The cache entry holds the models, grids and cost table themselves (strong references, compared with ``is``)
    # next to their device handles: an ``id()`` alone comes back as soon as CPython reuses a freed address, and the
    # handle array would then name destroyed cbo_gp / cbo_cands objects.
    handles = tuple(int(o._handle.value or 0) for o in list(models) + list(grids))      # ctypes.c_void_p handles
    st = cache.get("sweep_sets") if cache is not None else None
    same = (st is not None and not raw and st["cost_table"] is costs_functions and st["handles"] == handles
            and len(st["models"]) == s and all(a is b for a, b in zip(st["models"], models))
            and all(a is b for a, b in zip(st["grids"], grids)))
    if not same:
        if 0 in handles:
            raise ValueError("find_next_y_points: a model or candidate grid has been closed")
        costs = None if raw else [Cost(costs_functions, evaluated_sets[i]) for i in range(s)]
        st = {"cost_table": costs_functions, "models": list(models), "grids": list(grids), "handles": handles,
              "costs": costs,
              "batch_cost": np.array(costs_functions.values if raw else
                                     [float(costs[i].evaluate(grids[i].points)) for i in range(s)], dtype=np.float64),
              "gps": (ctypes.c_void_p * s)(*[m._handle for m in models]),
              "cds": (ctypes.c_void_p * s)(*[g._handle for g in grids]),
              "y_best": np.empty(s), "vals": np.empty(s), "idxs": np.empty(s, dtype=np.int64)}
        if cache is not None:
            cache["sweep_sets"] = st
    costs, batch_cost, vals, idxs = st["costs"], st["batch_cost"], st["vals"], st["idxs"]
    if st.get("kind") != kind:
        st.pop("trial_args", None)               # (CBOAcquisitionPath.trial_step's fixed arguments name the kind's call)
        st["kind"] = kind
    st["y_best"][:] = float(np.asarray(current_global_best, dtype=np.float64).reshape(-1)[0])
    if st.get("constraints") is not None or constraints is not None:
        st.pop("trial_args", None)               # (the one-call trial step names the unconstrained call)
    st["constraints"] = constraints
    if st.get("hyper_rows") is not None or hyper_rows is not None:
        st.pop("trial_args", None)               # (likewise: the one-call trial step names the plug-in call)
    st["hyper_rows"] = hyper_rows
    if st.get("batch_size") != batch_size:
        st.pop("trial_args", None)               # (a batch takes the three-call route; back at None the call is made anew)
    st["batch_size"] = batch_size
    if batch_size is not None:
        return _sweep_sets_batch(st, models, grids, current_global_best, task, batch_size, bool(update_incumbent), kind)
    if hyper_rows is not None:
        # (the entry keeps the row arrays and the pointer array alive; the rows change from trial to trial)
        st["hyper_args"] = ((ctypes.c_int * s)(*[r.shape[0] for r in hyper_rows]),
                            (ctypes.c_void_p * s)(*[r.ctypes.data for r in hyper_rows]))
        log_form = kind[0] == LOG_MEI            # (the same list, the log EI's jitter in the jitter's place)
        call = _lib.load().cbo_acq_sweep_sets_hyper_log if log_form else _lib.load().cbo_acq_sweep_sets_hyper
        _lib.check(call(s, st["gps"], st["cds"], st["hyper_args"][0], st["hyper_args"][1], _lib.dptr(st["y_best"]),
                        _lib.TASK_CODE[task], float(kind[1]) if log_form else 0.0, _lib.dptr(batch_cost), _lib.dptr(vals),
                        idxs.ctypes.data_as(_lib.c_int64_p)))
    elif constraints is not None:
        _sweep_sets_constrained(st, models, grids, constraints, task, kind)
    elif kind[0] == "MES":
        from .max_value_entropy import mes_sets_parameters
        st.pop("trial_args", None)               # (a trial step with MES takes the three-call route)
        _, mins = mes_sets_parameters(models, spaces, kind[1][0], kind[1][1])
        # (the entry keeps the sample arrays and the pointer array alive; winners_to_points re-evaluates against them)
        st["mes_mins"] = [_lib.as_f64(m) for m in mins]
        st["mes_args"] = ((ctypes.c_int * s)(*[m.shape[0] for m in st["mes_mins"]]),
                          (ctypes.c_void_p * s)(*[m.ctypes.data for m in st["mes_mins"]]))
        _lib.check(_lib.load().cbo_acq_sweep_sets_mes(s, st["gps"], st["cds"], st["mes_args"][0], st["mes_args"][1],
                                                      _lib.dptr(batch_cost), _lib.dptr(vals),
                                                      idxs.ctypes.data_as(_lib.c_int64_p)))
    elif kind[0] in (LOG_EI, LOG_CEI):           # (LOGCEI whose every list is empty: LOGEI's call, LOGEI's bits)
        st.pop("trial_args", None)               # (a trial step with the log EI takes the three-call route)
        _lib.check(_lib.load().cbo_acq_sweep_sets_logei(s, st["gps"], st["cds"], _lib.dptr(st["y_best"]), _lib.TASK_CODE[task],
                                                        kind[1], _lib.dptr(batch_cost), _lib.dptr(vals),
                                                        idxs.ctypes.data_as(_lib.c_int64_p)))
    elif kind[0] == "EI":
        _lib.check(_lib.load().cbo_acq_sweep_sets(s, st["gps"], st["cds"], _lib.dptr(st["y_best"]), _lib.TASK_CODE[task], 0.0,
                                                  _lib.dptr(batch_cost), _lib.dptr(vals),
                                                  idxs.ctypes.data_as(_lib.c_int64_p)))
    else:
        _lib.check(_lib.load().cbo_acq_sweep_sets_kind(s, st["gps"], st["cds"], _lib.ACQ_KIND_CODE[kind[0]],
                                                       _lib.dptr(st["y_best"]), _lib.TASK_CODE[task], kind[1],
                                                       _lib.dptr(batch_cost), _lib.dptr(vals),
                                                       idxs.ctypes.data_as(_lib.c_int64_p)))
    for i in range(s):
        # the general path fitted it on the way (deferred refit) -- the marginalised one restores a model instead: fitted
        # again if it was, unfitted if it was not
        if not models[i].small and hyper_rows is None:
            models[i].stale = False
    if constraints is not None:
        for i in range(s):                       # (a set with a larger model anywhere took the general path: all fitted)
            mine = [models[i]] + [c.model for c in constraints[i]]
            if any(not m.small for m in mine):
                for m in mine:
                    m.stale = False
    if raw:
        return None, [(float(vals[i]), int(idxs[i])) for i in range(s)]
    xs, ys = winners_to_points(st, models, grids, current_global_best, task)
    if refine:
        xs, ys = refine_winners(xs, ys, models, spaces, current_global_best, task, costs, kind, device_prior)
    if refine_constrained:
        xs, ys = refine_winners(xs, ys, models, spaces, current_global_best, task, costs, kind, constraints=constraints)
    return xs, ys


def checked_pointwise_cost(cost_mode, kind=("EI", None), constraints=None, hyper_samples=None, batch_size=None,
                           device_prior=False, raw=False):
    """``cost_mode`` of a sweep, a path or an agent, checked on the host before any device call: True for ``"pointwise"``
    (DESIGN.md §4y), which prices the causal EI or its logarithm alone -- no constraints, hyper-parameter samples, batches,
    device-resident priors or several ranks; False for ``"batch"``, today's behaviour."""
    from .cost_functions import checked_cost_mode
    if checked_cost_mode(cost_mode) == "batch":
        return False
    if kind[0] not in ("EI", LOG_EI):
        raise ValueError(f"cost_mode='pointwise' prices the causal EI or its logarithm: acquisition must be 'EI' or 'LOGEI', "
                         f"not {kind[0]!r}")
    if constraints is not None and any(constraints):
        raise ValueError("cost_mode='pointwise' is not defined for constrained acquisitions: constraints must be None or empty")
    if hyper_samples is not None:
        raise ValueError("cost_mode='pointwise' is not defined for the marginalised EI: hyper_samples must be None")
    if batch_size is not None:
        raise ValueError("cost_mode='pointwise' is not defined for batches: batch_size must be None")
    if device_prior:
        raise ValueError("cost_mode='pointwise' refines causal sets through the host route: device_prior must be False")
    if raw:
        raise ValueError("cost_mode='pointwise' is not defined across several ranks (raw=True)")
    return True


def _next_y_points_pointwise(models, current_global_best, evaluated_sets, costs_functions, task, grids, kind, refine, spaces):
    """``find_next_y_points(cost_mode="pointwise")``: one ``cbo_acq_sweep_sets_pointcost`` call over grids that carry their
    cost vectors, then -- ``refine=True`` -- ``refine_sets(cost_mode="pointwise")`` from the winners."""
    import ctypes
    from .. import _lib
    from .cost_functions import PointwiseCost
    s = len(models)
    if task not in _lib.TASK_CODE:
        raise ValueError(f"task must be 'min' or 'max', not {task!r}")
    costs = [PointwiseCost(costs_functions, evaluated_sets[i]) for i in range(s)]
    jitter = 0.0 if kind[1] is None else float(kind[1])
    y_best = float(np.asarray(current_global_best, dtype=np.float64).reshape(-1)[0])
    if any(not (o._handle.value or 0) for o in list(models) + list(grids)):
        raise ValueError("find_next_y_points: a model or candidate grid has been closed")
    for i in range(s):
        (_acquisition_for(kind[0], models[i], current_global_best, task, None, kind[1]) / costs[i]).set_grid_cost(grids[i])
    vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
    _lib.check(_lib.load().cbo_acq_sweep_sets_pointcost(
        s, (ctypes.c_void_p * s)(*[m._handle for m in models]), (ctypes.c_void_p * s)(*[g._handle for g in grids]),
        int(kind[0] == LOG_EI), _lib.dptr(np.full(s, y_best)), _lib.TASK_CODE[task], jitter, _lib.dptr(vals),
        idxs.ctypes.data_as(_lib.c_int64_p)))
    for m in models:
        if not m.small:                          # (the general path fitted it on the way)
            m.stale = False
    xs = [grids[i].points[int(idxs[i]) - grids[i].index_offset][None, :].copy() for i in range(s)]
    ys = [np.array([[float(vals[i])]]) for i in range(s)]
    if refine:
        from .causal_optimizer import refine_sets
        res = refine_sets(models, xs, [space_bounds(sp) for sp in spaces], current_global_best, task, costs, kind=kind,
                          cost_mode="pointwise")
        for i, (pts, fs, _) in enumerate(res):
            best = int(np.argmax(fs))
            if fs[best] >= ys[i][0, 0]:
                xs[i], ys[i] = pts[best][None, :].copy(), np.array([[fs[best]]])
    return xs, ys


def checked_log_cei(kind, constraints, hyper_samples=None, batch_size=None, refine=False, device_prior=False, raw=False,
                    cost_mode="batch", anchors="grid"):
    """What the constrained acquisition in log space (``"LOGCEI"``) does not combine with, checked on the
    host before any device call: it needs ``constraints`` (possibly empty lists) and is scored over the grid, once, with
    one cost per set, by a single process."""
    if kind[0] != LOG_CEI:
        return
    what = "acquisition='LOGCEI'"
    if constraints is None:
        raise ValueError(f"{what} sums the logarithms of the constraints' probabilities: constraints must be given "
                         "(without constraints the acquisition is 'LOGEI')")
    if hyper_samples is not None:
        raise ValueError(f"{what} is not defined for the marginalised EI: hyper_samples must be None")
    if batch_size is not None:
        raise ValueError(f"{what} is not defined for batches: batch_size must be None")
    if refine:
        raise ValueError(f"{what} has no refinement kernel: refine must be False")
    if device_prior:
        raise ValueError(f"{what} has no refinement kernel: device_prior must be False")
    if cost_mode != "batch":
        raise ValueError(f"{what} takes one cost per set: cost_mode must be 'batch', not {cost_mode!r}")
    if anchors != "grid":
        raise ValueError(f"{what} is scored over the grid: anchors must be 'grid'")
    if raw:
        raise ValueError(f"{what} is not defined across several ranks (raw=True)")


def checked_log_mei(kind, hyper_samples, constraints=None, batch_size=None, refine=False, refine_constrained=False,
                    device_prior=False, raw=False, cost_mode="batch", anchors="grid"):
    """What the hyper-marginalised EI in log space (``"LOGMEI"``) needs and does not combine with, checked on
    the host before any device call: it needs ``hyper_samples`` and is scored over the grid, once, with one cost per set,
    without constraints, by a single process."""
    if kind[0] != LOG_MEI:
        return
    what = "acquisition='LOGMEI'"
    if hyper_samples is None:
        raise ValueError(f"{what} is the logarithm of the EI averaged over hyper-parameter samples: hyper_samples must be "
                         "given (without samples the acquisition is 'LOGEI')")
    if constraints is not None and (not hasattr(constraints, "__len__") or any(constraints)):
        raise ValueError(f"{what} is not defined with constraints: constraints must be None or empty")
    if batch_size is not None:
        raise ValueError(f"{what} picks one point: batch_size must be None")
    if refine:
        raise ValueError(f"{what} has no refinement kernel: refine must be False")
    if refine_constrained:
        raise ValueError(f"{what} has no refinement kernel: refine_constrained must be False")
    if device_prior:
        raise ValueError(f"{what} has no refinement kernel: device_prior must be False")
    if cost_mode != "batch":
        raise ValueError(f"{what} takes one cost per set: cost_mode must be 'batch', not {cost_mode!r}")
    if anchors != "grid":
        raise ValueError(f"{what} is scored over the grid: anchors must be 'grid'")
    if raw:
        raise ValueError(f"{what} is not defined across several ranks (raw=True)")


def checked_log_bei(kind, batch_size, constraints=None, hyper_samples=None, refine=False, refine_constrained=False,
                    device_prior=False, raw=False, cost_mode="batch", anchors="grid"):
    """What the greedy batch in log space (``"LOGBEI"``) needs and does not combine with, checked on the host
    before any device call: it needs a ``batch_size`` and picks from the grid, with one cost per set, without constraints or
    hyper-parameter samples, unrefined, by a single process."""
    if kind[0] != LOG_BEI:
        return
    what = "acquisition='LOGBEI'"
    if batch_size is None:
        raise ValueError(f"{what} is the greedy batch scored in log space: batch_size must be given (without a batch the "
                         "acquisition is 'LOGEI')")
    if constraints is not None and (not hasattr(constraints, "__len__") or any(constraints)):
        raise ValueError(f"{what} is not defined with constraints: constraints must be None or empty")
    if hyper_samples is not None:
        raise ValueError(f"{what} is not defined for the marginalised EI: hyper_samples must be None")
    if refine:
        raise ValueError(f"{what} has no refinement between picks: refine must be False")
    if refine_constrained:
        raise ValueError(f"{what} has no refinement between picks: refine_constrained must be False")
    if device_prior:
        raise ValueError(f"{what} has no refinement between picks: device_prior must be False")
    if cost_mode != "batch":
        raise ValueError(f"{what} takes one cost per set: cost_mode must be 'batch', not {cost_mode!r}")
    if anchors != "grid":
        raise ValueError(f"{what} picks from the grid: anchors must be 'grid'")
    if raw:
        raise ValueError(f"{what} is not defined across several ranks (raw=True)")


def checked_device_prior(device_prior, refine):
    """``device_prior`` of a multi-set sweep, a path or an agent: it selects how causal sets are REFINED."""
    if device_prior and not refine:
        raise ValueError("device_prior=True puts causal sets into the refinement's device launch: refine must be True")
    return bool(device_prior)


def checked_log_ei(kind, device_prior=False, raw=False):
    """What the log Expected Improvement does not combine with beyond what the other checks refuse for every kind but the
    EI (constraints, hyper-parameter samples, batches): a device-resident prior in the refinement (the kernel's causal
    instantiation of this kind is not built) and several ranks (their exchange rescales values by a cost ratio)."""
    if kind[0] != LOG_EI:
        return
    if device_prior:
        raise ValueError("acquisition='LOGEI' refines causal sets through the host route: device_prior must be False")
    if raw:
        raise ValueError("acquisition='LOGEI' is not defined across several ranks (raw=True)")


def checked_refine(refine, kind, constraints=None, hyper_samples=None, batch_size=None, raw=False, spaces=None, n_sets=None):
    """``refine`` of a multi-set sweep, a path or an agent, checked on the host before any device call: gradient refinement
    is defined for the causal EI and the point-wise kinds alone, one winner per set, on a single rank, and needs the sets'
    boxes."""
    if not refine:
        return False
    if kind[0] == "MES":
        raise ValueError("refine=True: max-value entropy search has no gradients")
    if constraints is not None and any(constraints):
        raise ValueError("refine=True is not defined for constrained acquisitions: constraints must be None or empty")
    if hyper_samples is not None:
        raise ValueError("refine=True is not defined for the marginalised EI: hyper_samples must be None")
    if batch_size is not None:
        raise ValueError("refine=True is not defined for batches: batch_size must be None")
    if raw:
        raise ValueError("refine=True is not defined across several ranks (raw=True)")
    if spaces is None or not hasattr(spaces, "__len__") or (n_sets is not None and len(spaces) != n_sets):
        raise ValueError("refine=True searches inside the sets' boxes: spaces must have one entry per exploration set"
                         + ("" if n_sets is None else f" ({n_sets})"))
    return True


def checked_refine_constrained(refine_constrained, kind, constraints=None, hyper_samples=None, batch_size=None, raw=False,
                               spaces=None, n_sets=None, device_prior=False, cost_mode="batch"):
    """``refine_constrained`` of a multi-set sweep, a path or an agent, checked on the host before any device
    call: the constrained winners are refined under the product form (``"EI"``) or the log form (``"LOGCEI"``) alone, with
    constraints to refine under, inside the sets' boxes, one winner per set, on a single rank, with one cost per point from
    the sets' tables and no device-resident prior."""
    if not refine_constrained:
        return False
    what = "refine_constrained=True"
    if kind[0] not in ("EI", LOG_CEI):
        raise ValueError(f"{what} refines the constrained causal EI: acquisition must be 'EI' or 'LOGCEI', not {kind[0]!r}")
    if constraints is None or not hasattr(constraints, "__len__") or not any(constraints):
        raise ValueError(f"{what} refines under constraints: constraints must be given and not all empty (without "
                         "constraints the keyword is refine)")
    if raw:
        raise ValueError(f"{what} is not defined across several ranks (raw=True)")
    if hyper_samples is not None:
        raise ValueError(f"{what} is not defined for the marginalised EI: hyper_samples must be None")
    if batch_size is not None:
        raise ValueError(f"{what} is not defined for batches: batch_size must be None")
    if device_prior:
        raise ValueError(f"{what} has no causal instantiation: device_prior must be False")
    if cost_mode != "batch":
        raise ValueError(f"{what} climbs with the reference's zero cost gradient: cost_mode must be 'batch', not {cost_mode!r}")
    if spaces is None or not hasattr(spaces, "__len__") or (n_sets is not None and len(spaces) != n_sets):
        raise ValueError(f"{what} searches inside the sets' boxes: spaces must have one entry per exploration set"
                         + ("" if n_sets is None else f" ({n_sets})"))
    return True


def refine_winners(xs, ys, models, spaces, current_global_best, task, costs, kind, device_prior=False, constraints=None):
    """``find_next_y_points(refine=True)``'s second stage: every set's winner refined by ``refine_sets``; the refined point
    replaces it only if its value -- over the point's own cost, as ``winners_to_points`` prices the winner -- is not lower.
    ``constraints`` (``refine_constrained=True``): the same rule with the constrained value."""
    from .causal_optimizer import refine_sets
    res = refine_sets(models, xs, [space_bounds(sp) for sp in spaces], current_global_best, task, costs, kind=kind,
                      device_prior=device_prior, constraints=constraints)
    xs, ys = list(xs), list(ys)
    for i, (pts, vals, _) in enumerate(res):
        best = int(np.argmax(vals))
        if vals[best] >= ys[i][0, 0]:
            xs[i], ys[i] = pts[best][None, :].copy(), np.array([[vals[best]]])
    return xs, ys


def checked_batch_size(batch_size, kind=("EI", None), constraints=None, hyper_samples=None, raw=False):
    """``batch_size`` of a multi-set sweep, a path or an agent, checked on the host before any device call: ``None``, or
    an int in 1..64 -- with the causal EI (``"EI"``, or ``"LOGBEI"``: the same batch scored in log space), no (non-empty)
    constraints, no hyper-parameter samples and a single rank."""
    if batch_size is None:
        return None
    from .. import _lib
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive int, not {batch_size!r}")
    if batch_size > _lib.MAX_BATCH:
        raise ValueError(f"batch_size must be at most {_lib.MAX_BATCH}, not {batch_size}")
    if kind[0] not in ("EI", LOG_BEI):
        raise ValueError("batch selection believes the causal EI's model: acquisition must be 'EI' (or 'LOGBEI', the same "
                         "batch scored in log space)")
    if constraints is not None and any(constraints):
        raise ValueError("batch selection is not defined for constrained acquisitions: constraints must be None or empty")
    if hyper_samples is not None:
        raise ValueError("batch selection is not defined for the marginalised EI: hyper_samples must be None")
    if raw:
        raise ValueError("batch selection is not defined across several ranks (raw=True)")
    return int(batch_size)


def _sweep_sets_batch(st, models, grids, current_global_best, task, batch_size, update_incumbent, kind=("EI", None)):
    """The batch form of ``find_next_y_points``' device call: one ``cbo_acq_sweep_sets_batch`` -- for ``kind``
    ``("LOGBEI", jitter)`` one ``cbo_acq_sweep_sets_batch_logei`` -- its set-major winners as (B, d) points and (B, 1) values
    per set (``_next_y_points_batch``'s treatment of variable costs)."""
    from .. import _lib
    s = len(models)
    log_form = kind[0] == LOG_BEI
    for i in range(s):
        if batch_size > grids[i].points.shape[0]:
            raise ValueError(f"batch_size {batch_size} exceeds the {grids[i].points.shape[0]} candidates of set {i}")
    vals, idxs = np.empty(s * batch_size), np.empty(s * batch_size, dtype=np.int64)
    call = _lib.load().cbo_acq_sweep_sets_batch_logei if log_form else _lib.load().cbo_acq_sweep_sets_batch
    _lib.check(call(s, st["gps"], st["cds"], _lib.dptr(st["y_best"]), _lib.TASK_CODE[task], float(kind[1]) if log_form else 0.0,
                    _lib.dptr(st["batch_cost"]), batch_size, int(update_incumbent), _lib.dptr(vals),
                    idxs.ctypes.data_as(_lib.c_int64_p)))
    vals, idxs = vals.reshape(s, batch_size), idxs.reshape(s, batch_size)
    st["vals"][:], st["idxs"][:] = vals[:, 0], idxs[:, 0]
    xs, ys = [], []
    for i in range(s):
        # The library's static routing, mirrored: a set the one launch does not take was fitted by the general path inside
        # the call -- a larger or fp32 model always; a grid above the cap only when batch_size > 1 (a batch of one is
        # cbo_acq_sweep_sets' route, which takes a small model whatever its grid and does not fit it).  The library has no
        # query for "fitted": a small set that fell to the general path at run time (a non-positive pivot in the launch,
        # CBO_HIP_SMALL_SETS=0) is fitted too but stays ``stale`` here, which costs one redundant refit later, never a
        # wrong answer.
        if not models[i].small or (batch_size > 1 and grids[i].points.shape[0] > _lib.SMALL_BATCH_MAX_CANDS):
            models[i].stale = False
        x_new = grids[i].points[idxs[i] - grids[i].index_offset].copy()
        y = vals[i].reshape(-1, 1).copy()
        batch_cost = float(st["batch_cost"][i])
        for t in range(batch_size):
            point_cost = float(st["costs"][i].evaluate(x_new[t:t + 1]))
            if point_cost != batch_cost:
                y[t, 0] = (_acquisition_for(kind[0], models[i], current_global_best, task, None, kind[1]).sweep(
                    x_new[t:t + 1], cost=point_cost, want_acq=True)["acq"][0, 0] if t == 0
                           else _repriced(y[t, 0], batch_cost, point_cost, log_form))
        xs.append(x_new)
        ys.append(y)
    return xs, ys


def checked_set_hyper_samples(hyper_samples, models, kind=("EI", None), constraints=None, raw=False):
    """``find_next_y_points``' ``hyper_samples`` checked on the host: ``None``, or per set the contiguous (H_s, 2 + L_s) rows
    of ``cbo_acq_sweep_sets_hyper`` (``integrated_hyper._hyper_rows``: a fixed noise fills its own column).  Everything that
    can be refused is refused before a model draws (an int) and before any device call."""
    if hyper_samples is None:
        return None
    if kind[0] not in ("EI", LOG_MEI):
        raise ValueError("hyper-parameter samples marginalise the causal EI: acquisition must be 'EI' (or 'LOGMEI', the "
                         "logarithm of the average)")
    if constraints is not None:
        raise ValueError("the marginalised EI is not defined with constraints: constraints must be None or empty")
    if raw:
        raise ValueError("the marginalised EI is not defined across several ranks (raw=True)")
    from .. import _lib
    from .integrated_hyper import _hyper_rows
    if isinstance(hyper_samples, bool) or (isinstance(hyper_samples, (int, np.integer)) and hyper_samples < 1):
        raise ValueError(f"hyper_samples must be a list of (H, P) arrays or a positive int, not {hyper_samples!r}")
    if isinstance(hyper_samples, (int, np.integer)):
        if hyper_samples > _lib.MAX_HYPER_SAMPLES:
            raise ValueError(f"at most {_lib.MAX_HYPER_SAMPLES} samples, not {hyper_samples}")
        hyper_samples = [m.generate_hyperparameters_samples(int(hyper_samples)) for m in models]
    elif isinstance(hyper_samples, np.ndarray) or not hasattr(hyper_samples, "__len__"):
        raise ValueError("hyper_samples must be a list with one (H, P) array per exploration set, or a positive int")
    if len(hyper_samples) != len(models):
        raise ValueError(f"hyper_samples must have one entry per exploration set ({len(models)}), not {len(hyper_samples)}")
    rows = []
    for i, (model, samples) in enumerate(zip(models, hyper_samples)):
        try:
            r = _hyper_rows(model, samples)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"hyper_samples of set {i}: {exc}") from None
        if not np.all(np.isfinite(r)) or not np.all(r[:, :-1] > 0.0) or not np.all(r[:, -1] >= 0.0):
            raise ValueError(f"hyper_samples of set {i}: variances and lengthscales must be finite and positive, the noise "
                             "variance finite and not negative")
        rows.append(r)
    return rows


def checked_set_constraints(constraints, n_sets, kind=("EI", None), raw=False):
    """``find_next_y_points``' ``constraints`` checked on the host, before any device call: ``None`` when there is nothing
    to constrain (``None`` given, or every set's list empty), else a list of ``n_sets`` lists of ``ProbabilityOfFeasibility``."""
    import math
    if constraints is None:
        return None
    from .constrained import MAX_CONSTRAINTS, ProbabilityOfFeasibility
    constraints = [list(c) if c is not None else [] for c in constraints]
    if len(constraints) != n_sets:
        raise ValueError(f"constraints must have one entry per exploration set ({n_sets}), not {len(constraints)}")
    if not any(constraints):
        return None
    if kind[0] not in ("EI", LOG_CEI):
        raise ValueError("constraints multiply the causal EI: acquisition must be 'EI' (or 'LOGCEI', the sum of the "
                         "logarithms)")
    if raw:
        raise ValueError("constraints are not defined across several ranks (raw=True)")
    for i, cons in enumerate(constraints):
        if len(cons) > MAX_CONSTRAINTS:
            raise ValueError(f"set {i}: at most {MAX_CONSTRAINTS} constraints, not {len(cons)}")
        for c in cons:
            if not isinstance(c, ProbabilityOfFeasibility):
                raise ValueError(f"set {i}: a constraint must be a ProbabilityOfFeasibility, not {type(c).__name__}")
            for what, v in (("max_value", c.max_value), ("jitter", c.jitter)):
                try:
                    ok = math.isfinite(float(v))
                except (TypeError, ValueError):
                    ok = False
                if not ok:
                    raise ValueError(f"set {i}: a constraint's {what} must be a finite number, not {v!r}")
    return constraints


def _sweep_sets_constrained(st, models, grids, constraints, task, kind=("EI", None)):
    """The constrained form of ``find_next_y_points``' device call: the constraint models' candidate grids from the cache
    entry ``st`` (rebuilt where a model object changed), then ``cbo_acq_sweep_sets_constrained`` -- for ``kind``
    ``("LOGCEI", jitter)`` ``cbo_acq_sweep_sets_constrained_log`` -- into ``st``'s winners."""
    import ctypes
    from .. import _lib
    from .causal_acquisition_functions import CandidateGrid
    from .constrained import SENSE_CODE
    kept = st.setdefault("con_grids", {})            # (set, position) -> (model, CandidateGrid or None when it is grids[i])
    wanted = {(i, k): c.model for i, cons in enumerate(constraints) for k, c in enumerate(cons)}
    for key in [k for k, (m, _) in kept.items() if wanted.get(k) is not m]:
        grid = kept.pop(key)[1]
        if grid is not None:
            grid.close()
    con_gps, con_cds, values, jitters, senses = [], [], [], [], []
    for i, cons in enumerate(constraints):
        by_model = {id(models[i]): grids[i]}         # one candidate set serves one model (and that model everywhere in the set)
        for k, c in enumerate(cons):
            if (i, k) not in kept:
                grid = by_model.get(id(c.model))
                own = grid is None
                if own:
                    grid = CandidateGrid(grids[i].points, c.model, index_offset=grids[i].index_offset)
                kept[(i, k)] = (c.model, grid if own else None)
                by_model[id(c.model)] = grid
            else:
                grid = kept[(i, k)][1]
                if grid is None:
                    grid = by_model[id(c.model)]
                by_model.setdefault(id(c.model), grid)
            if not (c.model._handle.value and grid._handle.value):
                raise ValueError("find_next_y_points: a constraint's model or candidate grid has been closed")
            con_gps.append(c.model._handle); con_cds.append(grid._handle)
            values.append(float(c.max_value)); jitters.append(float(c.jitter)); senses.append(SENSE_CODE[c.sense])
    n = len(con_gps)
    n_con = (ctypes.c_int * len(models))(*[len(cons) for cons in constraints])
    log_form = kind[0] == LOG_CEI
    call = _lib.load().cbo_acq_sweep_sets_constrained_log if log_form else _lib.load().cbo_acq_sweep_sets_constrained
    _lib.check(call(
        len(models), st["gps"], st["cds"], _lib.dptr(st["y_best"]), _lib.TASK_CODE[task],
        float(kind[1]) if log_form else 0.0, _lib.dptr(st["batch_cost"]),
        n_con, (ctypes.c_void_p * n)(*con_gps), (ctypes.c_void_p * n)(*con_cds), _lib.dptr(np.array(values)),
        _lib.dptr(np.array(jitters)), (ctypes.c_int * n)(*senses), _lib.dptr(st["vals"]),
        st["idxs"].ctypes.data_as(_lib.c_int64_p)))


def winners_to_points(st, models, grids, current_global_best, task):
    """(xs, ys) of utils.py:36 from the winners a multi-set sweep left in ``st`` (the cache entry of
    ``find_next_y_points``): the grid point of every set and its acquisition value re-evaluated at that point alone --
    only variable costs change the value -- through the acquisition class of the kind the entry records."""
    costs, batch_cost, vals, idxs = st["costs"], st["batch_cost"], st["vals"], st["idxs"]
    name, param = st.get("kind", ("EI", None))
    constraints = st.get("constraints")
    hyper_rows = st.get("hyper_rows")
    xs, ys = [], []
    winners, values, batch = idxs.tolist(), vals.tolist(), batch_cost.tolist()
    for i in range(len(models)):
        j = winners[i] - grids[i].index_offset
        x_new = grids[i].points[j:j + 1].copy()
        point_cost = float(costs[i].evaluate(x_new))
        if point_cost == batch[i]:
            y = np.array(((values[i],),))
        elif hyper_rows is not None:
            from .integrated_hyper import IntegratedHyperParameterAcquisition
            if name == LOG_MEI:                  # (the log generator: re-priced by cbo_acq_sweep_hyper_log)
                generator = lambda mdl, c=costs[i]: _acquisition_for(LOG_EI, mdl, current_global_best, task, None,   # noqa: E731
                                                                     param) / c
            else:
                generator = lambda mdl, c=costs[i]: CausalExpectedImprovement(current_global_best, task, mdl) / c   # noqa: E731
            y = IntegratedHyperParameterAcquisition(models[i], generator, samples=hyper_rows[i]).evaluate(x_new)
        elif constraints is not None and constraints[i]:
            from .constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement
            if name == LOG_CEI:
                log_ei = _acquisition_for(name, models[i], current_global_best, task, None, param)
                y = (ConstrainedLogExpectedImprovement(log_ei, constraints[i]) / costs[i]).evaluate(x_new)
            else:
                ei = CausalExpectedImprovement(current_global_best, task, models[i])
                y = (AcquisitionProduct([ei] + list(constraints[i])) / costs[i]).evaluate(x_new)
        elif name == "MES":
            # the set's own draw: a fresh MaxValueEntropySearch would refit the Gumbel and draw again
            from .max_value_entropy import MaxValueEntropySearch
            mes = MaxValueEntropySearch(models[i], [(0.0, 1.0)] * x_new.shape[1], param[0], param[1])
            mes.mins = st["mes_mins"][i]
            y = mes.sweep(x_new, cost=point_cost, want_acq=True)["acq"]
        else:
            y = _acquisition_for(name, models[i], current_global_best, task, None, param).sweep(x_new, cost=point_cost,
                                                                                                want_acq=True)["acq"]
        xs.append(x_new)
        ys.append(y)
    return xs, ys
