"""The four methods of the reference's agent that drive the hot path, as a mixin/standalone class
(/root/reference/src/CBO.py:209-277; INTEGRATION.md shows the two-line change that makes ``src/CBO.py`` use it), and
``CBO``, the whole agent on top of them (src/CBO.py:11-291: ``run``, ``observe``, ``intervene``, ``epsilon``).
"""
from __future__ import annotations

import numpy as np

from .GaussianProcessFactory import GaussianProcessFactory as GPFactory
from .graphs import meshgrid_candidates
from .utils_functions.causal_acquisition_functions import CandidateGrid
from .utils_functions.utils import (checked_batch_size, default_grid_shape, find_current_global, find_next_y_point,  # noqa: F401
                                    find_next_y_points, space_bounds)


class _FixedCosts:
    """Batch costs decided by the caller (the whole grid's, when a rank only holds a block of it)."""

    def __init__(self, by_set, order):
        self.values = [by_set[s] for s in order]


def checked_path_constraints(constraints, kind=("EI", None)):
    """``CBOAcquisitionPath``'s ``constraints`` checked on the host: a list of ``(name, sense, value, jitter)`` (jitter 0
    where it was left out), empty for ``None``."""
    import math
    from .utils_functions.constrained import MAX_CONSTRAINTS, SENSE_CODE
    if not constraints:
        return []
    if kind[0] not in ("EI", "LOGCEI"):
        raise ValueError("constraints multiply the causal EI: acquisition must be 'EI' (or 'LOGCEI', the sum of the "
                         "logarithms)")
    if len(constraints) > MAX_CONSTRAINTS:
        raise ValueError(f"at most {MAX_CONSTRAINTS} constraints, not {len(constraints)}")
    out = []
    for entry in constraints:
        if not isinstance(entry, (tuple, list)) or len(entry) not in (3, 4):
            raise ValueError(f"a constraint is (name, sense, value[, jitter]), not {entry!r}")
        name, sense, value = entry[:3]
        jitter = entry[3] if len(entry) == 4 else 0.0
        if sense not in SENSE_CODE:
            raise ValueError(f"constraint {name!r}: sense must be '<=' or '>=', not {sense!r}")
        try:
            value, jitter = float(value), float(jitter)
        except (TypeError, ValueError):
            raise ValueError(f"constraint {name!r}: value and jitter must be finite numbers") from None
        if not (math.isfinite(value) and math.isfinite(jitter)):
            raise ValueError(f"constraint {name!r}: value and jitter must be finite numbers")
        out.append((name, sense, value, jitter))
    return out


def checked_path_hyper_samples(hyper_samples, kind=("EI", None), constraints=()):
    """``CBOAcquisitionPath``'s ``hyper_samples`` checked on the host: ``None``, a positive int (at most 256) or a callable."""
    from . import _lib
    if hyper_samples is None:
        return None
    if kind[0] not in ("EI", "LOGMEI"):
        raise ValueError("hyper-parameter samples marginalise the causal EI: acquisition must be 'EI' (or 'LOGMEI', the "
                         "logarithm of the average)")
    if constraints:
        raise ValueError("the marginalised EI is not defined with constraints: constraints must be None")
    if callable(hyper_samples):
        return hyper_samples
    if isinstance(hyper_samples, bool) or not isinstance(hyper_samples, (int, np.integer)) \
            or not 1 <= hyper_samples <= _lib.MAX_HYPER_SAMPLES:
        raise ValueError(f"hyper_samples must be an int in 1..{_lib.MAX_HYPER_SAMPLES} or a callable sampler(model, set_index), "
                         f"not {hyper_samples!r}")
    return int(hyper_samples)


def checked_hyper_sampler(hyper_sampler, hyper_samples):
    """``hyper_sampler`` checked on the host: ``"host"`` (the per-model host chain) or ``"device"`` (every chain in one
    launch); a callable ``hyper_samples`` is its own sampler and takes ``"host"`` alone."""
    if hyper_sampler not in ("host", "device"):
        raise ValueError(f"hyper_sampler must be 'host' or 'device', not {hyper_sampler!r}")
    if hyper_sampler == "device" and callable(hyper_samples):
        raise ValueError("hyper_sampler='device' draws the samples itself: hyper_samples must be an int, not a callable")
    return hyper_sampler


class CBOAcquisitionPath:
    """Holds exactly the state those methods read on the reference's ``CBO`` object: ``gp_type``,
    ``exploration_set``, ``costs``, ``task``, per-set data, spaces, prior closures and models.  ``acquisition`` (``"EI"``,
    the reference's, or ``"LCB" | "PI" | "MPEI" | "VAR"``) and ``acquisition_param`` (beta, default 1; the jitter of PI and
    MPEI, default 0) name what every exploration set is scored with (``find_next_y_points``); they are fixed
    at construction.  ``acquisition="MES"`` (``acquisition_param``: ``None`` or ``(num_samples, grid_size)``) scores every set
    with emukit's max-value entropy search over the cost: two device calls per trial for all sets, the
    Gumbel grids drawn from ``space_list``; it needs ``task="min"``, no constraints, no hyper-parameter samples and a single
    process, and its ``trial_step`` takes the three-call route.  ``acquisition="LOGEI"`` (``acquisition_param``: the jitter,
    default 0) scores every set with the logarithm of the causal EI minus the logarithm of the cost, computed without
    underflow: where the EI of every candidate is an exact 0.0 the sets still rank; no constraints, no
    hyper-parameter samples, no batch, no ``device_prior``, a single process, and ``trial_step`` takes the three-call route.
    ``cost_mode="pointwise"`` (with ``"EI"`` or ``"LOGEI"``) scores every candidate over its OWN cost,
    ``EI(x) / c(x)``, where the default ``"batch"`` divides a whole grid by one scalar (the reference's quirk): the value
    reported for a set is the winner's own, ``refine=True`` climbs with the cost's own gradient, and ``trial_step`` takes the
    three-call route; no constraints, hyper-parameter samples, batch or ``device_prior``, a single process, and a cost table
    ``cost_structure`` recognises.
    ``constraints`` (a list of ``(name, sense, value[, jitter])``, at most 8, shared by all sets; ``sense`` ``"<="`` or
    ``">="``) with ``constraint_data_y`` (``constraint_data_y[s][c]`` is (n_s, 1): the values of node ``c`` at ``data_x[s]``)
    make every set's score ``EI * prod PoF / cost``: the path keeps ``constraint_models[s][c]`` --
    non-causal models from the factory on ``data_x[s]`` -- rebuilds them with the objectives and passes them on.  They need
    ``acquisition="EI"`` and a single process -- or ``acquisition="LOGCEI"`` (``acquisition_param``: the log EI's jitter,
    default 0), which scores every set with ``log EI + sum log PoF - log cost``: finite and ordered where
    every product is an exact 0.0 and set 0 would win the tie.  ``"LOGCEI"`` needs constraints, no hyper-parameter samples,
    no batch, no ``refine``, no ``device_prior``, ``cost_mode="batch"`` and a single process.
    ``hyper_samples`` (a positive int H, or a callable ``sampler(model, set_index) -> (H, P)`` samples in GPy's parameter
    order) makes every set's score the causal EI marginalised over hyper-parameter samples of its own model:
    an int draws ``model.generate_hyperparameters_samples(H)`` with emukit's defaults.  The path keeps ``hyper_rows[s]`` and
    redraws them whenever it rebuilds the set's model.  It needs ``acquisition="EI"``, no constraints and a single process.
    ``hyper_sampler="device"`` (with an int ``hyper_samples``) draws them by the one-launch HMC: every set's
    rows in one ``cbo_gp_hmc_sets`` call after ``update_all_gaussian_processes``, the rebuilt set's in a one-model call;
    ``"host"`` (default) is the per-model host chain.
    ``acquisition="LOGMEI"`` (``acquisition_param``: the log EI's jitter, default 0) with ``hyper_samples``
    scores every set with the LOGARITHM of that marginalised EI, ``log((1 / H) sum_h EI_h) - log cost`` -- not the average of
    the logarithms -- which stays finite and ordered where the average itself is an exact 0.0 on every grid (small models with
    noise 1e-10, early in a run) and set 0 would win the tie.  It needs ``hyper_samples`` (either ``hyper_sampler``), no
    constraints, no batch, no ``refine`` / ``refine_constrained`` / ``device_prior``, ``cost_mode="batch"`` and a single process.
    ``batch_size`` (an int B in 1..64) with ``update_incumbent`` makes every set's answer a greedy batch of B Kriging-believer
    picks in one device call (``find_next_y_points(batch_size=B)``): ``xs[s]`` is (B, d), ``ys[s]`` (B, 1); the
    set is chosen by pick 0, as before.  It needs ``acquisition="EI"``, no constraints, no hyper-parameter samples and a
    single process, and its ``trial_step`` takes the three-call route.
    ``acquisition="LOGBEI"`` (``acquisition_param``: the log EI's jitter, default 0) with ``batch_size`` scores
    every pick of that batch with ``log EI - log cost`` (``cbo_acq_sweep_sets_batch_logei``): where the incumbent lies below a
    set's own data -- every set but the best one -- the EI of every pick is an exact 0.0 and ``"EI"`` returns the grid's first
    point B times; the log form returns B distinct, ordered picks.  It needs ``batch_size``, no constraints, no
    hyper-parameter samples, no ``refine`` / ``refine_constrained`` / ``device_prior``, ``cost_mode="batch"`` and a single
    process, and its ``trial_step`` takes the multi-call route.
    ``refine_constrained=True`` (with ``constraints`` and ``acquisition`` ``"EI"`` or ``"LOGCEI"``): every set's
    constrained winner is refined by L-BFGS on the constrained acquisition inside the set's box from ``space_list``
    (``find_next_y_points(refine_constrained=True)``), all sets in one further device call, single process; ``trial_step``
    takes the multi-call route, as it does under constraints anyway.  ``refine=True`` with constraints keeps raising.
    ``refine=True`` adds the reference's second stage (``find_next_y_points(refine=True)``): every set's
    winner is refined by L-BFGS inside the set's box from ``space_list``, all sets in one further device call, and kept only
    if it is not lower.  It needs ``"EI"`` or a point-wise kind, no constraints, no hyper-parameter samples, no batch and a
    single process, and its ``trial_step`` takes the three-call route.  ``device_prior=True`` (with ``refine=True``) lets
    causal sets into that device call through a device-resident do-calculus prior.
    ``mle_optimizer="device"`` (with ``mle_restarts`` starts per model, 1..16) runs the hyper-parameter MLEs this path
    starts -- the one in front of the device HMC -- as one-launch searches; ``"host"`` (default) is scipy's
    L-BFGS-B, unchanged.  ``mle_device_rows`` (128, or 256 with ``"device"``) is the largest model the agent's
    one-launch searches take (``CBO``); the MLE in front of the device HMC keeps 128.
    ``hyper_priors`` (a dict ``"variance"`` / ``"lengthscale"`` / ``"noise_var"`` -> a prior of ``utils_functions.priors``):
    every exploration-set model carries these priors whenever it is built or rebuilt (``HipGaussianProcess.set_prior``,
    DESIGN.md §4w), so the MLEs and the HMC of this path work on the log posterior; ``None`` (default) sets none."""

    def __init__(self, gp_type, exploration_set, costs, task, data_x, data_y, space_list, mean_functions=None,
                 var_functions=None, grid_shapes=None, keep_solutions=True, comm="env", acquisition="EI",
                 acquisition_param=None, constraints=None, constraint_data_y=None, hyper_samples=None, batch_size=None,
                 update_incumbent=False, refine=False, hyper_sampler="host", device_prior=False, mle_optimizer="host",
                 mle_restarts=1, hyper_priors=None, cost_mode="batch", mle_device_rows=128, refine_constrained=False):
        from .GaussianProcessFactory import checked_mle_device_rows, checked_mle_optimizer
        from .utils_functions.priors import checked_priors
        from .utils_functions.utils import (checked_device_prior, checked_log_bei, checked_log_cei, checked_log_ei,
                                            checked_log_mei, checked_pointwise_cost, checked_refine,
                                            checked_refine_constrained, sets_acquisition_or_default as sets_acquisition)
        self.mle_optimizer, self.mle_restarts = checked_mle_optimizer(mle_optimizer, mle_restarts), int(mle_restarts)
        self.mle_device_rows = checked_mle_device_rows(mle_device_rows, mle_optimizer)
        checked_log_bei(sets_acquisition(acquisition, acquisition_param), batch_size, constraints or None, hyper_samples, refine,
                        refine_constrained, device_prior, False, cost_mode)
        checked_log_mei(sets_acquisition(acquisition, acquisition_param), hyper_samples, constraints or None, batch_size, refine,
                        refine_constrained, device_prior, False, cost_mode)
        self.device_prior = checked_device_prior(device_prior, refine)
        # priors on every exploration-set model's hyper-parameters (name -> prior), or None: today's behaviour
        self.hyper_priors = checked_priors(hyper_priors) or None
        # what every exploration set is scored with: "EI" (the reference's) or a point-wise kind with its parameter
        # (``find_next_y_points``); fixed at construction and checked here, before any device call
        self._kind = sets_acquisition(acquisition, acquisition_param)
        self.acquisition, self.acquisition_param = acquisition, acquisition_param
        checked_log_ei(self._kind, self.device_prior)
        checked_log_cei(self._kind, constraints or None, hyper_samples, batch_size, refine, device_prior, False, cost_mode)
        if self._kind[0] == "MES" and task != "min":
            raise ValueError("acquisition='MES' minimises: task must be 'min'")
        self.constraints = checked_path_constraints(constraints, self._kind)
        if self.constraints:
            if constraint_data_y is None or len(constraint_data_y) != len(exploration_set) \
                    or any(len(row) != len(self.constraints) for row in constraint_data_y):
                raise ValueError("constraint_data_y must hold, for every exploration set, one column per constraint")
        # (kept as given, like data_x / data_y: the caller appends to its lists between trials)
        self.constraint_data_y = constraint_data_y if self.constraints else None
        self.constraint_models = []
        self.hyper_samples = checked_path_hyper_samples(hyper_samples, self._kind, self.constraints)
        self.hyper_sampler = checked_hyper_sampler(hyper_sampler, self.hyper_samples)
        self.hyper_rows = [None] * len(exploration_set)
        self.batch_size = checked_batch_size(batch_size, self._kind, self.constraints, self.hyper_samples)
        self.update_incumbent = bool(update_incumbent)
        self.refine = checked_refine(refine, self._kind, self.constraints, self.hyper_samples, self.batch_size, False,
                                     space_list, len(exploration_set))
        # the constrained winners' second stage: off by default, refine=True with constraints keeps raising
        self.refine_constrained = checked_refine_constrained(
            refine_constrained, self._kind, [self.constraints] * len(exploration_set) if self.constraints else None,
            hyper_samples, batch_size, False, space_list, len(exploration_set), device_prior, cost_mode)
        # "batch": the reference's one scalar per grid; "pointwise" (DESIGN.md §4y): every candidate over its own cost
        self.cost_mode = "pointwise" if checked_pointwise_cost(cost_mode, self._kind, self.constraints, self.hyper_samples,
                                                               self.batch_size, self.device_prior) else "batch"
        if self.cost_mode == "pointwise":
            from .utils_functions.cost_functions import PointwiseCost
            for es in exploration_set:
                PointwiseCost(costs, es)                     # (a cost cost_structure does not recognise: ValueError here)
        self.gp_type = gp_type
        self.exploration_set = exploration_set
        self.es_size = len(exploration_set)
        self.costs = costs
        self.task = task
        self.data_x, self.data_y = data_x, data_y
        self.space_list = space_list
        self.mean_functions = mean_functions or [None] * self.es_size
        self.var_functions = var_functions or [None] * self.es_size
        self.grid_shapes = grid_shapes or [None] * self.es_size
        self.intervention_names = ["".join(v) for v in exploration_set]
        self.models = []
        self.last_intervention = None
        self._grids = {}          # per set: (grid shape, prior closures, device-resident candidate grid)
        self._grid_points = {}    # per set: (space object, grid shape object, shape, points)
        self._call_cache = {}     # handle arrays and batch costs of the multi-set sweep, valid while the objects are
        # Several GPUs (one process per GPU): ``comm`` is a sharding.Communicator (or anything with world / rank /
        # argmax), "env" = the launcher's (RANK / WORLD_SIZE), None = single process.  Whole exploration sets go to
        # ranks when there are at least as many sets as ranks (S = 25 coral sets on 8 GPUs: every GPU sweeps full
        # grids of three sets), candidate blocks of every set otherwise; either way one 16-byte exchange per set.
        self._comm = comm
        # keep L^-1 K* of every set's grid on the device: a trial then costs the set intervened on one forward
        # solve and one new row (append-only step) instead of a refit and a full sweep
        self.keep_solutions = bool(keep_solutions)

    def update_all_gaussian_processes(self):
        """CBO.py:209-222."""
        self._call_cache.clear()          # its handle arrays name the models and grids replaced below
        for _, grid in self._grids.values():
            grid.close()
        self._grids.clear()
        self.models = [
            GPFactory.create(self.gp_type, self.data_x[s], self.data_y[s],
                             [self.mean_functions[s], self.var_functions[s]], emukit_wrapper=True, priors=self.hyper_priors)
            for s in range(self.es_size)
        ]
        if self.constraints:
            self.constraint_models = [[self._constraint_model(s, c) for c in range(len(self.constraints))]
                                      for s in range(self.es_size)]
        if self.hyper_samples is not None and self.hyper_sampler == "device":
            # every set's chain in one launch
            from .GaussianProcessFactory import generate_hyperparameters_samples_together
            from .utils_functions.integrated_hyper import _hyper_rows
            drawn = generate_hyperparameters_samples_together(self.models, self.hyper_samples, optimizer=self.mle_optimizer,
                                                              num_restarts=self.mle_restarts)
            self.hyper_rows = [_hyper_rows(model, samples) for model, samples in zip(self.models, drawn)]
            return
        for s in range(self.es_size):
            self._draw_hyper_rows(s)

    def _draw_hyper_rows(self, s):
        """``hyper_rows[s]``: fresh samples for set s's model as the rows ``cbo_acq_sweep_sets_hyper`` takes."""
        if self.hyper_samples is None:
            return
        from .utils_functions.integrated_hyper import _hyper_rows
        model = self.models[s]
        if callable(self.hyper_samples):
            samples = self.hyper_samples(model, s)
        elif self.hyper_sampler == "device":
            samples = model.generate_hyperparameters_samples(self.hyper_samples, sampler="device")
        else:
            samples = model.generate_hyperparameters_samples(self.hyper_samples)
        self.hyper_rows[s] = _hyper_rows(model, samples)

    def _constraint_model(self, s, c, fit=True):
        from .GaussianProcessFactory import GaussianProcessType
        return GPFactory.create(GaussianProcessType.NON_CAUSAL_GP, self.data_x[s], self.constraint_data_y[s][c], [None, None],
                                emukit_wrapper=True, fit=fit)

    def set_constraints(self):
        """Per set the ``ProbabilityOfFeasibility`` factors of this path's constraints over its constraint models (what
        ``find_next_y_points`` takes), or ``None`` without constraints."""
        if not self.constraints:
            return None
        from .utils_functions.constrained import ProbabilityOfFeasibility
        return [[ProbabilityOfFeasibility(self.constraint_models[s][c], jitter, value, sense=sense)
                 for c, (_, sense, value, jitter) in enumerate(self.constraints)] for s in range(self.es_size)]

    def update_gaussian_process_of_last_intervention(self, fit=False):
        """CBO.py:224-235.  By default the rebuilt model is left unfitted: ``compute_best_acquisition_values``
        comes next (CBO.py:152-164) and its sweep over this set refits and sweeps in one overlapped device call.
        ``fit=True`` restores the reference's timing (a not-PD error then surfaces here)."""
        s = self.last_intervention
        model = self.models[s]
        for c in range(len(self.constraints)):              # (the set's constraint models take the same rows)
            self.constraint_models[s][c].rebuild(self.data_x[s], self.constraint_data_y[s][c], fit=fit)
        if model is not None and model.mean_function is self.mean_functions[s] \
                and model.variance_adjustment is self.var_functions[s]:
            model.rebuild(self.data_x[s], self.data_y[s], fit=fit)      # same handle: no allocation, no new grid
            self._draw_hyper_rows(s)
            return
        self._call_cache.clear()
        old = self._grids.pop(s, None)
        if old is not None:
            old[1].close()
        self.models[s] = GPFactory.create(self.gp_type, self.data_x[s], self.data_y[s],
                                          [self.mean_functions[s], self.var_functions[s]], emukit_wrapper=True, fit=fit,
                                          priors=self.hyper_priors)
        self._draw_hyper_rows(s)

    @property
    def comm(self):
        if isinstance(self._comm, str):                      # "env": formed on first use (touches the GPU)
            from .sharding import default_communicator
            self._comm = default_communicator()
        return self._comm

    def placement(self):
        """("single" | "sets" | "candidates", world, rank)."""
        comm = self.comm
        if comm is None or comm.world == 1:
            return "single", 1, 0
        return ("sets" if self.es_size >= comm.world else "candidates"), comm.world, comm.rank

    def grid_points(self, s):
        """(shape, points) of set s's regular grid; built once per (space object, grid shape) -- replace
        ``space_list[s]`` / ``grid_shapes[s]`` to change it (the cache keeps the space object alive, so its identity
        cannot be reused)."""
        space, want = self.space_list[s], self.grid_shapes[s]
        hit = self._grid_points.get(s)
        if hit is not None and hit[0] is space and hit[1] is want:
            return hit[2], hit[3]
        bounds = space_bounds(space)
        shape = tuple(want or default_grid_shape(len(bounds)))
        pts = meshgrid_candidates(bounds, shape)
        self._grid_points[s] = (space, want, shape, pts)
        return shape, pts

    def candidate_grid(self, s):
        """The regular grid over the set's box, resident on the device across trials (the reference draws fresh
        random anchors each trial; the grid of BASELINE.json's sweep is fixed).  Rebuilt when the grid shape, the
        model object or the prior closures change.  Under candidate placement it is this rank's contiguous block of
        the grid (``index_offset`` = the block's first row); ``full_points`` keeps the whole grid for the look-up of
        the winner."""
        mode, world, rank = self.placement()
        shape, pts = self.grid_points(s)
        key = (shape, id(self.models[s]), id(self.mean_functions[s]), id(self.var_functions[s]), mode, world, rank)
        cached = self._grids.get(s)
        if cached is None or cached[0] != key:
            if cached is not None:
                self._call_cache.clear()
                cached[1].close()
            if mode == "candidates":
                from .sharding import shard_bounds
                begin, end = shard_bounds(pts.shape[0], world, rank)
                grid = CandidateGrid(pts[begin:max(end, begin + 1)] if end > begin else pts[:1], self.models[s],
                                     index_offset=begin, keep_solution=self.keep_solutions)
                grid.empty_shard = end <= begin
            else:
                grid = CandidateGrid(pts, self.models[s], keep_solution=self.keep_solutions)
                grid.empty_shard = False
            grid.full_points = pts
            cached = (key, grid)
            self._grids[s] = cached
        return cached[1]

    def compute_best_acquisition_values(self, current_best):
        """CBO.py:237-260: the loop over the exploration sets, as ONE device call (``cbo_acq_sweep_sets``, or
        ``cbo_acq_sweep_sets_kind`` for the path's point-wise ``acquisition``); across several GPUs, this rank's share of
        it and one arg-max exchange per set.  With the path's ``batch_size`` B it is one ``cbo_acq_sweep_sets_batch`` call
        (a single process only): ``xs[s]`` is (B, d) and ``ys[s]`` (B, 1), row 0 the single-point result."""
        mode, world, rank = self.placement()
        if self.constraints and mode != "single":
            raise ValueError(f"constraints are scored by a single process: the placement is {mode!r}")
        if self.hyper_samples is not None and mode != "single":
            raise ValueError(f"the marginalised EI is scored by a single process: the placement is {mode!r}")
        if self._kind[0] == "MES" and mode != "single":
            raise ValueError(f"max-value entropy search is scored by a single process: the placement is {mode!r}")
        if self.batch_size is not None and mode != "single":
            raise ValueError(f"batch selection is scored by a single process: the placement is {mode!r}")
        if (self.refine or self.refine_constrained) and mode != "single":
            raise ValueError(f"gradient refinement is run by a single process: the placement is {mode!r}")
        if self._kind[0] in ("LOGEI", "LOGMEI", "LOGBEI") and mode != "single":
            raise ValueError(f"the log Expected Improvement is scored by a single process: the placement is {mode!r}")
        if self.cost_mode == "pointwise" and mode != "single":
            raise ValueError(f"cost_mode='pointwise' is scored by a single process: the placement is {mode!r}")
        if mode == "single":
            grids = [self.candidate_grid(s) for s in range(self.es_size)]
            return find_next_y_points(self.models, current_best, self.exploration_set, self.costs, self.task, grids,
                                      cache=self._call_cache, acquisition=self._kind, constraints=self.set_constraints(),
                                      hyper_samples=None if self.hyper_samples is None else list(self.hyper_rows),
                                      spaces=self.space_list if (self._kind[0] == "MES" or self.refine
                                                                 or self.refine_constrained) else None,
                                      batch_size=self.batch_size, update_incumbent=self.update_incumbent,
                                      refine=self.refine, device_prior=self.device_prior, cost_mode=self.cost_mode,
                                      refine_constrained=self.refine_constrained)
        from .sharding import ERROR_CANDIDATE, NO_CANDIDATE
        from .utils_functions.cost_functions import Cost
        # A rank that fails (a model that is not positive definite, a device error) must not leave the others blocked in
        # an exchange: every rank takes part in one failure-flag exchange per trial and all of them raise when it is set.
        local, failure = {}, None
        try:
            mine = [s for s in range(self.es_size) if mode == "candidates" or s % world == rank]
            mine = [s for s in mine if not (mode == "candidates" and self.candidate_grid(s).empty_shard)]
            if mine:
                grids = [self.candidate_grid(s) for s in mine]
                # batch costs are those of the WHOLE grid (a variable cost sums |x| over the batch column)
                full_cost = {s: float(Cost(self.costs, self.exploration_set[s]).evaluate(self.candidate_grid(s).full_points))
                             for s in mine}
                _, ys = find_next_y_points([self.models[s] for s in mine], current_best,
                                           [self.exploration_set[s] for s in mine], _FixedCosts(full_cost, mine), self.task,
                                           grids, cache=self._call_cache, raw=True, acquisition=self._kind)
                local = {s: ys[i] for i, s in enumerate(mine)}
        except Exception as exc:  # noqa: BLE001 -- re-raised below, after the exchanges
            failure = exc
        # One explicit flag per trial says whether any rank failed (cbo_comm_max_f64 of 0 / 1): it is not encoded in the
        # arg-max payload, where a healthy rank's genuine NaN acquisition (NaN is maximal, lowest index wins) could beat an
        # error record and leave the ranks disagreeing about whether to go on.  Every rank raises when it is set, before any
        # arg-max exchange.  (A communicator without ``max`` -- a caller's own object with only world / rank / argmax --
        # keeps the error record in the payload.)
        flag = getattr(self.comm, "max", None)
        winners, failed_somewhere = [], False
        if flag is not None:
            failed_somewhere = float(flag(1.0 if failure is not None else 0.0)) > 0.0
            if failure is not None:
                raise failure
            if failed_somewhere:
                raise RuntimeError("compute_best_acquisition_values: another rank failed during this trial's sweep")
        for s in range(self.es_size):
            val, idx = (float("nan"), ERROR_CANDIDATE) if failure is not None else local.get(s, (-np.inf, NO_CANDIDATE))
            val, idx = self.comm.argmax(val, idx)                       # identical on every rank
            failed_somewhere = failed_somewhere or idx == ERROR_CANDIDATE
            winners.append((val, idx))
        if failure is not None:
            raise failure
        if failed_somewhere:
            raise RuntimeError("compute_best_acquisition_values: another rank failed during this trial's sweep")
        xs, out = [], []
        for s in range(self.es_size):
            val, idx = winners[s]
            pts = self.grid_points(s)[1]
            x_new = pts[idx][None, :].copy()
            cost = Cost(self.costs, self.exploration_set[s])
            batch, point = float(cost.evaluate(pts)), float(cost.evaluate(x_new))
            # utils.py:36 re-evaluates EI / cost at x_new alone: the same EI over the point's own cost
            out.append(np.array([[val if point == batch else val * batch / point]]))
            xs.append(x_new)
        return xs, out

    def trial_step(self, current_best):
        """One trial of the reference's loop between two observations (src/CBO.py:143-173, ``CBO.intervene``) as ONE
        device-library call: ``update_gaussian_process_of_last_intervention`` (the model of the set intervened on last takes
        ``data_x / data_y`` of that set), ``compute_best_acquisition_values`` and ``select_next_intervention``.  Returns
        ``(xs, ys, (exploration set, index))`` -- what those three return -- and leaves ``last_intervention`` at the pick.
        At the reference's model sizes the three calls' host glue costs as much as the one launch that serves them
        (``cbo_trial_step``, ``cbo_trial_step_kind`` for a point-wise ``acquisition``); anything the one call does not cover
        (several ranks, a model rebuilt with other prior closures or other hyper-parameters, the first trial,
        constraints, hyper-parameter samples, a batch, max-value entropy search -- whose host draws its Gumbel samples between
        the Gumbel fit and the scoring) takes the three calls."""
        import ctypes
        from . import _lib
        from .utils_functions.utils import winners_to_points
        s = self.last_intervention
        st = self._call_cache.get("sweep_sets")
        model = self.models[s] if (s is not None and self.models) else None
        fast = (st is not None and model is not None and not self.constraints and self.hyper_samples is None
                and self._kind[0] not in ("MES", "LOGEI", "LOGCEI", "LOGBEI") and self.batch_size is None and not self.refine
                and self.cost_mode == "batch"
                and (self.comm is None or self.comm.world == 1)
                and model.mean_function is self.mean_functions[s] and model.variance_adjustment is self.var_functions[s]
                and model._hyper_initial and st["cost_table"] is self.costs
                and st["models"] == self.models)             # (lists of the same objects: compared by identity first)
        if fast:
            grids, cached = st["grids"], self._grids
            for i in range(self.es_size):
                entry = cached.get(i)
                if entry is None or entry[1] is not grids[i]:
                    fast = False
                    break
        if not fast:
            if s is not None:
                self.update_gaussian_process_of_last_intervention()
            xs, ys = self.compute_best_acquisition_values(current_best)
            return xs, ys, self.select_next_intervention(ys)
        model._set_arrays(self.data_x[s], self.data_y[s])
        pm, pv = model._prior(model.X)
        st["y_best"].fill(current_best if type(current_best) is float else
                          float(np.asarray(current_best, dtype=np.float64).reshape(-1)[0]))
        fixed = st.get("trial_args")             # what does not change from trial to trial, made once
        if fixed is None:
            # (the entry was made by this path's compute_best_acquisition_values: st["kind"] is this path's kind)
            chosen = ctypes.c_int(-1)
            lib = _lib.load()
            kind = st["kind"]
            fixed = st["trial_args"] = (kind, lib.cbo_trial_step if kind[0] == "EI" else lib.cbo_trial_step_kind,
                                        _lib.dptr(st["y_best"]), _lib.dptr(st["batch_cost"]),
                                        _lib.dptr(st["vals"]), st["idxs"].ctypes.data_as(_lib.c_int64_p), chosen,
                                        ctypes.byref(chosen), kind[0] == "EI")
        kind, call, y_best, batch_cost, vals, idxs, chosen, chosen_ref, ei = fixed
        if ei:
            rc = call(self.es_size, st["gps"], st["cds"], s, model.X.shape[0], _lib.dptr(model.X), _lib.dptr(model._y_flat),
                      _lib.dptr(pm), _lib.dptr(pv), y_best, _lib.TASK_CODE[self.task], 0.0, batch_cost, vals, idxs,
                      chosen_ref)
        else:
            rc = call(self.es_size, st["gps"], st["cds"], s, model.X.shape[0], _lib.dptr(model.X), _lib.dptr(model._y_flat),
                      _lib.dptr(pm), _lib.dptr(pv), _lib.ACQ_KIND_CODE[kind[0]], y_best, _lib.TASK_CODE[self.task], kind[1],
                      batch_cost, vals, idxs, chosen_ref)
        if rc:
            _lib.check(rc)
        model.stale = model.small            # (a larger model was refitted by the general path inside the call)
        for m in self.models:
            if not m.small:
                m.stale = False
        xs, ys = winners_to_points(st, self.models, st["grids"], current_best, self.task)
        pick = chosen.value
        if not ei and np.array([y[0, 0] for y in ys], dtype=np.float64).tobytes() != st["vals"].tobytes():
            # the library picked among the winners at their batch costs; a variable cost has re-evaluated some at their own:
            # the pick is ``select_next_intervention``'s over those, as the three calls make it.  (The EI's one-call form
            # keeps the library's pick, as it always has.)
            pick = self.select_next_intervention(ys)[1]
        self.last_intervention = pick
        return xs, ys, (self.exploration_set[pick], pick)

    def current_best_solution(self, current_best_y):
        """CBO.py:262-267 (the monitor's ``current_best_y`` dict is passed in)."""
        return find_current_global(current_best_y, self.intervention_names, self.task)

    def select_next_intervention(self, acquisition_ys):
        """CBO.py:269-277: first index of the maximum."""
        ys = np.asarray([np.asarray(y, dtype=np.float64).reshape(-1)[0] for y in acquisition_ys])
        indices = int(np.where(ys == np.max(ys))[0][0])
        self.last_intervention = indices
        return self.exploration_set[indices], self.last_intervention

    # BASELINE.json's north_star calls it select_intervention
    select_intervention = select_next_intervention


class CBO(CBOAcquisitionPath):
    """The reference's agent (src/CBO.py:11-291): ``run()``, its epsilon-greedy choice between ``observe()`` and
    ``intervene()``, ``epsilon``, ``compute_cost``, and a minimal monitor.  ``intervene()`` is the acquisition path of
    ``CBOAcquisitionPath``; ``observe()`` refits every graph-level GP of the graph in lockstep
    (``graph.fit_all_gaussian_processes``: one device call per L-BFGS round for all of them) and refreshes the
    do-calculus priors through ``DoCalculus``.

    Arguments are the reference's (src/ArgumentParser.py:16-33 and the data loader's fields), with the data as plain
    arrays instead of pickles: ``measurements`` / ``all_measurements`` map variable names to columns (the observational
    rows the agent starts with / the whole observational data set it draws further rows from, src/CBO.py:190-200);
    ``interventional_data[s]`` is (data_x, data_y) of exploration set s (what ``define_initial_data_cbo`` extracts from
    the interventional data, src/Monitor.py:24-27); ``target_functions[s]`` (optional) maps (1, d) intervention values
    to the (1, 1) target -- by default ``compute_interventions`` on the graph's SEM (src/Monitor.py:55-63).
    ``exploration_set``: "MIS" / "POMIS" as in the reference, or the list of sets itself.  With ``causal_prior`` every
    set's ``get_gp_name`` must name a graph GP; the constructor raises KeyError naming the first that does not.
    ``lockstep=False`` fits the graph GPs one after another (the reference's order; same models).
    ``acquisition`` / ``acquisition_param``: what ``intervene()`` scores the exploration sets with, as for
    ``CBOAcquisitionPath`` (default: the reference's causal EI; ``"MES"`` needs ``task="min"``).
    ``constraints`` (``{"node": (sense, value[, jitter])}``): other nodes of the graph that must stay in range; every set is
    scored with ``EI * prod PoF / cost``.  ``constraint_functions[s][node]`` maps (M, d) intervention values
    of set s to the (M, 1) values of the node -- by default ``compute_interventions`` on the graph's SEM with
    ``target_variable=node``.  A constrained node that is the target, or that some exploration set manipulates, raises
    ``ValueError``.  The incumbent stays the plain best observation (``find_current_global``), as in emukit's recipe; the
    monitor records ``constraint_values`` and ``feasible`` per trial.  With ``acquisition="LOGCEI"`` the score is the sum of
    the logarithms, ``log EI + sum log PoF - log cost``, as for ``CBOAcquisitionPath``.
    ``hyper_samples`` (a positive int or a callable sampler, as for ``CBOAcquisitionPath``): ``intervene()`` scores every set
    with the EI marginalised over hyper-parameter samples of its model; the closing ``optimize()`` of the
    chosen set's model stays, as in the reference.  ``hyper_sampler="device"`` draws them by the one-launch HMC (DESIGN.md
    §4s), as for ``CBOAcquisitionPath``.
    ``acquisition="LOGMEI"`` (with ``hyper_samples``) scores every set with the logarithm of that marginalised
    EI, ``log((1 / H) sum_h EI_h) - log cost``, which still ranks the sets where the average is an exact 0.0 everywhere, as
    for ``CBOAcquisitionPath``.
    ``batch_size`` (an int B in 1..64) with ``update_incumbent``: ``intervene()`` runs the B interventions of a greedy batch on
    the chosen set side by side: the monitor evaluates the B rows, appends them in order and records
    ``chosen`` as ``(set, x (B, d))``; the trial's cost is the sum of the B interventions' costs.  ``None``: the reference's
    one intervention per trial.  ``acquisition="LOGBEI"`` (with ``batch_size``) scores the batch's picks in log
    space, as for ``CBOAcquisitionPath``: B distinct interventions where ``"EI"`` would run the same one B times.
    ``refine_constrained=True`` (with ``constraints``): the constrained winners are refined likewise, on the constrained
    acquisition (``CBOAcquisitionPath(refine_constrained=True)``).
    ``refine=True``: every set's winner is refined by L-BFGS inside the set's interventional ranges before the set is chosen
    (``CBOAcquisitionPath(refine=True)``) -- the reference's continuous optimum instead of a grid point.
    ``device_prior=True`` (with ``refine=True`` and ``causal_prior=True``): the causal sets are refined inside the device launch,
    their do-calculus priors evaluated there, instead of on the host route.
    ``mle_optimizer="device"`` (with ``mle_restarts`` starts per model, 1..16): every hyper-parameter MLE of the agent -- the
    graph GPs of ``run()``'s first fit and of ``observe()``, and the closing ``optimize()`` of ``intervene()``, the chosen
    set's constraint models included, in one call -- is a one-launch device search instead of scipy's
    L-BFGS-B with a device call per evaluation; ``"host"`` (default) changes nothing.  ``mle_device_rows=256`` (with
    ``"device"``) keeps graph GPs of 129..256 observational rows inside that launch -- from the second observe
    step of a default run they have that many -- instead of sending them to the lockstep host route; 128 (default) changes
    nothing.
    ``hyper_priors`` (a dict ``"variance"`` / ``"lengthscale"`` / ``"noise_var"`` -> a prior of ``utils_functions.priors``):
    priors on the hyper-parameters of every exploration-set model, applied whenever one is built or rebuilt;
    the graph-level GPs take none.  ``None`` (default): no priors, today's behaviour to the bit."""

    TARGET = "Y"

    def __init__(self, graph, measurements, all_measurements, interventional_data, exploration_set="MIS",
                 num_interventions=10, initial_num_obs_samples=100, causal_prior=False, num_trials=40, task="min",
                 num_additional_observations=20, type_cost=1, name_index=0, target_functions=None, grid_shapes=None,
                 lockstep=True, verbose=False, acquisition="EI", acquisition_param=None, constraints=None,
                 constraint_functions=None, hyper_samples=None, batch_size=None, update_incumbent=False, refine=False,
                 hyper_sampler="host", device_prior=False, mle_optimizer="host", mle_restarts=1, hyper_priors=None,
                 cost_mode="batch", mle_device_rows=128, refine_constrained=False):
        from .DoCalculus import DoCalculus
        from .GaussianProcessFactory import GaussianProcessType, checked_mle_device_rows, checked_mle_optimizer
        checked_mle_device_rows(mle_device_rows, checked_mle_optimizer(mle_optimizer, mle_restarts))
        from .utils_functions.priors import checked_priors
        checked_priors(hyper_priors)                           # (on the host, before any device call)
        from .graphs import _columns
        from .utils_functions.utils import checked_refine, sets_acquisition_or_default as sets_acquisition
        self.graph = graph() if isinstance(graph, type) else graph
        self.measurements = _columns(measurements)
        self.all_measurements = _columns(all_measurements)
        exploration = ([list(s) for s in self.graph.get_exploration_set(exploration_set)]
                       if isinstance(exploration_set, str) else [list(s) for s in exploration_set])
        constraints = dict(constraints or {})
        for node in constraints:
            if node == self.TARGET:
                raise ValueError(f"constraint on {node!r}: the target itself cannot be constrained")
            sets = [s for s in exploration if node in s]
            if sets:
                raise ValueError(f"constraint on {node!r}: exploration set {sets[0]} manipulates it")
        path_constraints = [(node,) + tuple(spec) for node, spec in constraints.items()]
        self.num_interventions = num_interventions
        self.max_n = initial_num_obs_samples + 50
        self.initial_num_obs_samples = initial_num_obs_samples
        self.num_trials = num_trials
        self.num_additional_observations = num_additional_observations
        self.type_cost = type_cost
        self.name_index = name_index
        self.lockstep = bool(lockstep)
        self.verbose = verbose
        gp_type = GaussianProcessType.CAUSAL_GP if causal_prior else GaussianProcessType.NON_CAUSAL_GP
        if causal_prior:
            # the do-calculus prior of set s is built on the graph GP get_gp_name(s) (src/DoCalculus.py:46-47; the
            # reference raises KeyError at the first observe when the graph fits none of that name): checked up front
            fitted = {self.graph.get_gp_name(d) for d in self.graph.fit_dependencies}
            for s in exploration:
                name = self.graph.get_gp_name(s)
                if name not in fitted:
                    raise KeyError(f"causal prior of exploration set {s}: the graph fits no GP named {name!r} "
                                   f"(it fits {sorted(fitted)})")
        data_x = [np.asarray(x, dtype=np.float64).reshape(len(x), -1) for x, _ in interventional_data]
        data_y = [np.asarray(y, dtype=np.float64).reshape(-1, 1) for _, y in interventional_data]
        if len(data_x) != len(exploration):
            raise ValueError(f"interventional_data has {len(data_x)} sets, the exploration set {len(exploration)}")
        from .utils_functions.utils import checked_log_bei, checked_log_cei, checked_log_mei
        checked_log_bei(sets_acquisition(acquisition, acquisition_param), batch_size, path_constraints or None, hyper_samples,
                        refine, refine_constrained, device_prior, False, cost_mode)
        checked_log_mei(sets_acquisition(acquisition, acquisition_param), hyper_samples, path_constraints or None, batch_size,
                        refine, refine_constrained, device_prior, False, cost_mode)
        checked_log_cei(sets_acquisition(acquisition, acquisition_param), path_constraints or None, hyper_samples, batch_size,
                        refine, device_prior, False, cost_mode)
        path_constraints = checked_path_constraints(path_constraints, sets_acquisition(acquisition, acquisition_param))
        checked_path_hyper_samples(hyper_samples, sets_acquisition(acquisition, acquisition_param), path_constraints)
        checked_hyper_sampler(hyper_sampler, hyper_samples)
        checked_batch_size(batch_size, sets_acquisition(acquisition, acquisition_param), path_constraints, hyper_samples)
        checked_refine(refine, sets_acquisition(acquisition, acquisition_param), path_constraints, hyper_samples, batch_size,
                       False, [self.graph.bounds(s) for s in exploration], len(exploration))
        if device_prior and not refine:
            raise ValueError("device_prior=True puts causal sets into the refinement's device launch: refine must be True")
        from .utils_functions.utils import checked_refine_constrained
        checked_refine_constrained(refine_constrained, sets_acquisition(acquisition, acquisition_param),
                                   [path_constraints] * len(exploration) if path_constraints else None, hyper_samples,
                                   batch_size, False, [self.graph.bounds(s) for s in exploration], len(exploration), device_prior,
                                   cost_mode)
        from .utils_functions.utils import checked_log_ei
        checked_log_ei(sets_acquisition(acquisition, acquisition_param), device_prior)
        from .utils_functions.utils import checked_pointwise_cost
        checked_pointwise_cost(cost_mode, sets_acquisition(acquisition, acquisition_param), path_constraints, hyper_samples,
                               batch_size, device_prior)
        sem = None
        if path_constraints and constraint_functions is None:
            from functools import partial
            from .utils_functions.graph_functions import compute_interventions
            sem = self.graph.define_sem()
            constraint_functions = [{node: partial(compute_interventions, sem, {v: "" for v in s}, target_variable=node)
                                     for node in constraints} for s in exploration]
        self.constraint_functions = constraint_functions if path_constraints else None
        # the initial constraint data: the functions at the rows of the initial data_x[s]
        constraint_data_y = [[np.asarray(self.constraint_functions[s][node](data_x[s]), dtype=np.float64).reshape(-1, 1)
                              for node, _, _, _ in path_constraints] for s in range(len(exploration))] if path_constraints else None
        super().__init__(gp_type, exploration, self.graph.get_cost_structure(type_cost), task, data_x, data_y,
                         [self.graph.bounds(s) for s in exploration], grid_shapes=grid_shapes, comm=None,
                         acquisition=acquisition, acquisition_param=acquisition_param, constraints=path_constraints,
                         constraint_data_y=constraint_data_y, hyper_samples=hyper_samples, batch_size=batch_size,
                         update_incumbent=update_incumbent, refine=refine, hyper_sampler=hyper_sampler,
                         device_prior=device_prior, mle_optimizer=mle_optimizer, mle_restarts=mle_restarts,
                         hyper_priors=hyper_priors, cost_mode=cost_mode, mle_device_rows=mle_device_rows,
                         refine_constrained=refine_constrained)
        if target_functions is None:
            from functools import partial
            from .utils_functions.graph_functions import compute_interventions
            sem = sem or self.graph.define_sem()
            target_functions = [partial(compute_interventions, sem, {v: "" for v in s}, target_variable="Y")
                                for s in exploration]
        self.target_functions = list(target_functions)
        self.do_calculus = DoCalculus(self)
        self.graph_gps = {}
        self.monitor = _Monitor(self)

    # -- src/CBO.py:83-121 ---------------------------------------------------------------------------
    def run(self):
        """Fit the graph GPs, observe once, intervene once, then ``num_trials - 2`` epsilon-greedy trials
        (``numpy.random.uniform(0., 1.) < epsilon``: observe, else intervene)."""
        from numpy.random import uniform
        self.graph_gps = self.graph.fit_all_gaussian_processes(self.measurements, lockstep=self.lockstep, **self._mle_kwargs())
        self.observe()
        self.intervene()
        self.monitor.start()
        for _ in range(self.num_trials - 2):
            if uniform(0., 1.) < self.epsilon:
                self.observe()
            else:
                self.intervene()
        self.monitor.stop()
        return self.monitor

    def observe(self):
        """src/CBO.py:123-141: new observational rows, every graph GP refitted on all rows (in lockstep), the
        do-calculus priors rebuilt from them."""
        self.monitor.log_agent_behaviour(act=False)
        new = self.get_new_observation()
        self.measurements = {k: np.vstack([v, new[k]]) for k, v in self.measurements.items()}
        self.graph_gps = self.graph.fit_all_gaussian_processes(self.measurements, lockstep=self.lockstep, **self._mle_kwargs())
        self.mean_functions, self.var_functions = self.do_calculus.update_all_do_functions(self.graph_gps)
        self.monitor.log_agent_performance()

    def intervene(self):
        """src/CBO.py:143-173.  With ``batch_size`` B the chosen set -- picked by the first value of each ``ys[s]``, as
        always -- contributes its whole batch: ``compute_cost`` sums the B interventions' costs and the monitor evaluates and
        appends the B rows in order (``_Monitor._log_batch``), then the set's model is optimised once."""
        self.monitor.log_agent_behaviour(act=True)
        current_best = self.current_best_solution(self.monitor.current_best_y)
        if self.monitor.agent_previously_observed() or not self.models:
            self.update_all_gaussian_processes()
        else:
            self.update_gaussian_process_of_last_intervention(fit=True)
        xs, ys = self.compute_best_acquisition_values(current_best)
        intervention_set, intervention = self.select_next_intervention(ys)
        cost = self.compute_cost(intervention_set, intervention, xs)
        self.monitor.log_agent_performance(intervention_set, intervention, xs, cost)
        closing = [self.models[intervention]] + list(self.constraint_models[intervention] if self.constraints else ())
        if self.mle_optimizer == "device":
            from .GaussianProcessFactory import optimize_together
            optimize_together(closing, optimizer="device", num_restarts=self.mle_restarts, device_rows=self.mle_device_rows)
            return
        for model in closing:
            model.optimize()

    def _mle_kwargs(self):
        """What ``fit_all_gaussian_processes`` is told beside the reference's arguments: nothing on the default route."""
        if self.mle_optimizer == "host":
            return {}
        rows = {} if self.mle_device_rows == 128 else {"device_rows": self.mle_device_rows}
        return {"optimizer": self.mle_optimizer, "num_restarts": self.mle_restarts, **rows}

    @property
    def epsilon(self):
        """src/CBO.py:175-188: (hull volume of the observations of the manipulative variables / volume of their
        interventional box) / (rows / max_n)."""
        from .utils_functions.utils import compute_coverage, update_hull
        coverage_total = compute_coverage(self.measurements, self.graph.manipulative_variables,
                                          self.interventional_ranges)[2]
        coverage_obs = update_hull(self.measurements, self.graph.manipulative_variables)
        rescale = self.n_measurements / self.max_n
        return (coverage_obs / coverage_total) / rescale

    @property
    def n_measurements(self):
        return next(iter(self.measurements.values())).shape[0]

    @property
    def interventional_ranges(self):
        return self.graph.get_interventional_ranges()

    def get_new_observation(self):
        """src/CBO.py:196-200 -> cbo_functions.observe: the rows [initial_num_obs_samples, + num_additional_observations)
        of the whole observational data set (the same rows at every observe, as in the reference)."""
        lo = self.initial_num_obs_samples
        return {k: v[lo:lo + self.num_additional_observations] for k, v in self.all_measurements.items()}

    def compute_cost(self, intervention_set, intervention, acquisition_xs):
        """src/CBO.py:279-291; with a batch, the sum over the batch's interventions in order."""
        from .utils_functions.cost_functions import total_cost
        rows = np.asarray(acquisition_xs[intervention])
        if self.batch_size is None:
            x = {v: rows[0, i] for i, v in enumerate(intervention_set)}
            return total_cost(intervention_set, self.costs, x)
        cost = 0.
        for row in rows:
            cost += total_cost(intervention_set, self.costs, {v: row[i] for i, v in enumerate(intervention_set)})
        return cost


class _Monitor:
    """What src/Monitor.py records of a run: per trial whether the agent intervened (1) or observed (0), the best
    target value so far, the cumulative cost, and for interventions the set and the values chosen."""

    def __init__(self, cbo):
        import copy
        self.cbo = cbo
        task = cbo.task
        best = [(np.min(y) if task == "min" else np.max(y), s) for s, y in enumerate(cbo.data_y)]
        opt_y, s_best = (min if task == "min" else max)(best, key=lambda t: t[0])
        self.current_best_y = {n: [np.inf if task == "min" else -np.inf] for n in cbo.intervention_names}
        self.current_best_x = copy.deepcopy(self.current_best_y)
        self.current_best_y[cbo.intervention_names[s_best]].append(float(opt_y))
        self.global_opt = [float(opt_y)]
        self.current_cost = [0.]
        self.cumulative_cost = 0.
        self.type_trial = []
        self.chosen = []                 # per trial: (exploration set, values (1,d)) or None for an observe
        # with constraints, per trial: {node: value at the chosen intervention} and whether all of them are in range
        # (None for an observe)
        self.constraint_values = []
        self.feasible = []
        self.start_time = self.total_time = None

    def start(self):
        import time
        self.start_time = time.perf_counter()

    def stop(self):
        import time
        self.total_time = time.perf_counter() - self.start_time

    def log_agent_behaviour(self, act):
        self.type_trial.append(1 if act else 0)

    def agent_previously_observed(self):
        return len(self.type_trial) >= 2 and self.type_trial[-2] == 0

    def log_agent_performance(self, intervention_set=None, intervention=None, acquisition_xs=None, current_cost=None):
        if current_cost is None:
            self.global_opt.append(self.global_opt[-1])
            self.current_cost.append(self.current_cost[-1])
            self.chosen.append(None)
            self.constraint_values.append(None)
            self.feasible.append(None)
            return
        cbo = self.cbo
        if getattr(cbo, "batch_size", None) is not None:
            return self._log_batch(intervention_set, intervention, acquisition_xs, current_cost)
        x_new = np.asarray(acquisition_xs[intervention], dtype=np.float64).reshape(1, -1)
        y_new = np.asarray(cbo.target_functions[intervention](x_new), dtype=np.float64).reshape(1, 1)
        cbo.data_x[intervention] = np.vstack((cbo.data_x[intervention], x_new))
        cbo.data_y[intervention] = np.vstack((cbo.data_y[intervention], y_new))
        cbo.models[intervention].set_data(cbo.data_x[intervention], cbo.data_y[intervention])
        values, feasible = {}, True
        for c, (node, sense, bound, _) in enumerate(cbo.constraints):
            v = float(np.asarray(cbo.constraint_functions[intervention][node](x_new), dtype=np.float64).reshape(-1)[0])
            column = cbo.constraint_data_y[intervention][c] = np.vstack((cbo.constraint_data_y[intervention][c], [[v]]))
            cbo.constraint_models[intervention][c].set_data(cbo.data_x[intervention], column)
            values[node] = v
            feasible = feasible and (v <= bound if sense == "<=" else v >= bound)
        self.constraint_values.append(values if cbo.constraints else None)
        self.feasible.append(feasible if cbo.constraints else None)
        name = cbo.intervention_names[intervention]
        self.current_best_x[name].append(float(x_new[0, 0]))
        self.current_best_y[name].append(float(y_new[0, 0]))
        self.global_opt.append(float(find_current_global(self.current_best_y, cbo.intervention_names, cbo.task)))
        self.cumulative_cost += current_cost
        self.current_cost.append(self.cumulative_cost)
        self.chosen.append((list(intervention_set), x_new.copy()))

    def _log_batch(self, intervention_set, intervention, acquisition_xs, current_cost):
        """A trial that ran a batch: the B rows evaluated, appended in order (one ``set_data``), every value in order into
        the set's bests; ``chosen`` holds (set, x (B, d)).  (A batch needs no constraints: the agent refuses both.)"""
        cbo = self.cbo
        x_new = np.asarray(acquisition_xs[intervention], dtype=np.float64)
        x_new = x_new.reshape(-1, x_new.shape[-1])
        y_new = np.vstack([np.asarray(cbo.target_functions[intervention](row[None, :]), dtype=np.float64).reshape(1, 1)
                           for row in x_new])
        cbo.data_x[intervention] = np.vstack((cbo.data_x[intervention], x_new))
        cbo.data_y[intervention] = np.vstack((cbo.data_y[intervention], y_new))
        cbo.models[intervention].set_data(cbo.data_x[intervention], cbo.data_y[intervention])
        self.constraint_values.append(None)
        self.feasible.append(None)
        name = cbo.intervention_names[intervention]
        for t in range(x_new.shape[0]):
            self.current_best_x[name].append(float(x_new[t, 0]))
            self.current_best_y[name].append(float(y_new[t, 0]))
        self.global_opt.append(float(find_current_global(self.current_best_y, cbo.intervention_names, cbo.task)))
        self.cumulative_cost += current_cost
        self.current_cost.append(self.cumulative_cost)
        self.chosen.append((list(intervention_set), x_new.copy()))
