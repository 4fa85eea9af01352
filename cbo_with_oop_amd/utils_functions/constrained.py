"""Constrained acquisition on the MI355X path: Expected Improvement times probabilities of feasibility over a cost.

emukit's recipe for constrained Bayesian optimisation is
``ExpectedImprovement(model) * ProbabilityOfFeasibility(constraint_model) / Cost``: a ``Product`` of acquisitions under a
``Quotient``.  Here the whole expression is ONE device call over a candidate grid (``cbo_acq_sweep_constrained``,
include/cbo_hip.h; kernels_con.hip): every model's sweep leaves its two vectors on the device and one pass multiplies the
terms, divides by the cost and takes the arg-max.  Nothing per candidate comes back unless it is asked for.

emukit is not installed here: ``ProbabilityOfFeasibility`` restates emukit 0.4's
``emukit.bayesian_optimization.acquisitions.ProbabilityOfFeasibility`` from memory --
``evaluate(x) = scipy.stats.norm.cdf(max_value, mean + jitter, sqrt(variance))`` of ``model.predict(x)`` -- and parity is
unpinned.  ``sense=">="`` (the constrained node must stay ABOVE ``max_value``) is this package's addition:
the complement, by symmetry ``ndtr(-u)``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib
from .causal_acquisition_functions import AcquisitionQuotient, CandidateGrid, CausalExpectedImprovement

MAX_CONSTRAINTS = 8         # CBO_MAX_CONSTRAINTS
SENSE_CODE = {"<=": 0, ">=": 1}       # CBO_CON_LE, CBO_CON_GE


class ProbabilityOfFeasibility:
    has_gradients = True

    def __init__(self, model, jitter=0.0, max_value=0.0, *, sense="<="):
        """emukit's signature (``model``, ``jitter``, ``max_value``) and defaults; ``sense``: ``"<="`` (emukit's: the
        probability that the model's output is at most ``max_value``) or ``">="``.  Construction only stores its
        arguments.  Restated from memory, parity unpinned."""
        if sense not in SENSE_CODE:
            raise ValueError(f"sense must be '<=' or '>=', not {sense!r}")
        self.model = model
        self.jitter = jitter
        self.max_value = max_value
        self.sense = sense

    def sweep(self, candidates, cost=1.0, want_acq=False):
        """Score every candidate and pick the best: dict(best_val, best_idx, acq), as ``CausalExpectedImprovement.sweep``.
        ``candidates`` is a CandidateGrid built for this model or an (M,d) array."""
        return AcquisitionProduct([self]).sweep([candidates] if isinstance(candidates, CandidateGrid) else candidates,
                                                cost=cost, want_acq=want_acq)

    def evaluate(self, x):
        """(M,1) probability of feasibility: emukit's ``evaluate``.  Restated from memory, parity unpinned."""
        return self.sweep(_lib.as_f64(x), want_acq=True)["acq"]

    def evaluate_with_gradients(self, x):
        """(pof (M,1), d pof / d x (M,d)).  Posterior and its gradients come from the device; the closing arithmetic on M
        (a few) points is host numpy, as in ``CausalExpectedImprovement.evaluate_with_gradients``:
        ``d pof / dx = -pdf(u) (dmean/dx + u dsd/dx) / sd`` with ``u = (max_value - mean - jitter) / sd``, the sign
        flipped for ``">="``."""
        import scipy.stats
        x = _lib.as_f64(x)
        mean, variance = self.model.predict(x)
        standard_deviation = np.sqrt(variance)
        dmean_dx, dvariance_dx = self.model.get_prediction_gradients(x)
        dstandard_deviation_dx = dvariance_dx / (2 * standard_deviation)
        mean = mean + self.jitter
        u = (float(self.max_value) - mean) / standard_deviation
        dcdf_dx = -scipy.stats.norm.pdf(u) * (dmean_dx + u * dstandard_deviation_dx) / standard_deviation
        if self.sense == "<=":
            return scipy.stats.norm.cdf(u), dcdf_dx
        return scipy.stats.norm.cdf(-u), -dcdf_dx

    def __mul__(self, other):
        return AcquisitionProduct([self, other])

    def __truediv__(self, cost):
        return AcquisitionQuotient(AcquisitionProduct([self]), cost)


class AcquisitionProduct:
    """emukit ``Product`` of acquisitions, flattened: at most one ``CausalExpectedImprovement`` (the objective) and the
    ``ProbabilityOfFeasibility`` factors in the order they were multiplied.  The value is
    ``((EI * pof_0) * pof_1) * ...`` -- what nested emukit Products compute -- formed on the device."""
    _call = "cbo_acq_sweep_constrained"          # the device call of ``sweep``
    _term_names = ("ei", "pof")                  # the keys of ``sweep``'s per-factor outputs

    def __init__(self, factors):
        flat = []
        for f in factors:
            flat.extend(f.factors if isinstance(f, AcquisitionProduct) else [f])
        for f in flat:
            if not isinstance(f, (CausalExpectedImprovement, ProbabilityOfFeasibility)):
                raise ValueError(f"a product takes CausalExpectedImprovement and ProbabilityOfFeasibility factors, not "
                                 f"{type(f).__name__}: only their product has a device pass")
        objectives = [f for f in flat if isinstance(f, CausalExpectedImprovement)]
        if len(objectives) > 1:
            raise ValueError("a product takes at most one CausalExpectedImprovement (one objective)")
        self.objective = objectives[0] if objectives else None
        self.constraints = [f for f in flat if isinstance(f, ProbabilityOfFeasibility)]
        if len(self.constraints) > MAX_CONSTRAINTS:
            raise ValueError(f"a product takes at most {MAX_CONSTRAINTS} ProbabilityOfFeasibility factors")
        # the objective first, as the device call has it (multiplication of two doubles commutes exactly, so
        # ``pof * EI`` and ``EI * pof`` are the same bits)
        self.factors = ([self.objective] if self.objective is not None else []) + self.constraints
        self.model = self.factors[0].model
        self._cached = None         # (the caller's CandidateGrid, [CandidateGrid per factor], those built here)

    def __mul__(self, other):
        return AcquisitionProduct([self, other])

    def __truediv__(self, cost):
        """``EI * PoF / Cost``: the existing AcquisitionQuotient (the cost divides inside the device call)."""
        return AcquisitionQuotient(self, cost)

    @property
    def has_gradients(self):
        return True

    # -- candidate sets: one per factor, each scaled (and, for a causal model, given its prior closures) for its model --
    def _build(self, points):
        grids, by_model = [], {}
        for f in self.factors:
            g = by_model.get(id(f.model))
            if g is None:
                g = by_model[id(f.model)] = CandidateGrid(points, f.model)
            grids.append(g)
        return grids

    @staticmethod
    def _close(grids):
        for g in grids:
            g.close()

    def close(self):
        """Free the candidate sets kept for a CandidateGrid passed to ``sweep``."""
        if self._cached is not None:
            self._close(self._cached[2])
            self._cached = None

    def _grids_for(self, candidates):
        """([CandidateGrid per factor], whether they are closed after the call)."""
        if isinstance(candidates, CandidateGrid):
            # one grid for the whole product (the optimiser's): it serves the first factor, whose model it was built
            # for; the other models' sets are built from its points once and kept while the same grid comes back
            if self._cached is None or self._cached[0] is not candidates:
                self.close()
                others = {}
                grids = [candidates]
                for f in self.factors[1:]:
                    if f.model is self.factors[0].model:
                        grids.append(candidates)
                        continue
                    if id(f.model) not in others:
                        others[id(f.model)] = CandidateGrid(candidates.points, f.model,
                                                            index_offset=candidates.index_offset)
                    grids.append(others[id(f.model)])
                self._cached = (candidates, grids, list(others.values()))      # (the caller's grid stays the caller's)
            return self._cached[1], False
        if isinstance(candidates, (list, tuple)) and all(isinstance(g, CandidateGrid) for g in candidates):
            if len(candidates) != len(self.factors):
                raise ValueError(f"{len(self.factors)} factors need {len(self.factors)} CandidateGrids, one per factor "
                                 f"(objective first), not {len(candidates)}")
            return list(candidates), False
        return self._build(_lib.as_f64(candidates)), True

    def sweep(self, candidates, cost=1.0, want_acq=False, want_terms=False):
        """Score every candidate with ``EI * prod PoF / cost`` in one device call and pick the best: returns
        dict(best_val, best_idx, acq, ei, pof).  ``candidates``: a sequence of CandidateGrids, one per factor (the
        objective's first, then the constraints' in order), each built for its factor's model over the same points; one
        CandidateGrid built for the first factor's model (the other models' sets are then built from its points and
        kept while the same grid comes back); or an (M,d) array (the sets are built, the causal models' prior closures
        evaluated, and everything is closed afterwards).  ``want_terms``: ``ei`` (M,1) and ``pof`` (M, n_constraints)."""
        grids, own = self._grids_for(candidates)
        try:
            m = len(grids[0])
            n_con = len(self.constraints)
            acq = np.empty(m) if want_acq else None
            ei = np.empty(m) if want_terms and self.objective is not None else None
            pof = np.empty((n_con, m)) if want_terms and n_con else None
            best_val, best_idx = ctypes.c_double(0.0), ctypes.c_int64(-1)
            obj = self.objective
            con_grids = grids[1:] if obj is not None else grids
            gps = (ctypes.c_void_p * max(n_con, 1))(*[c.model._handle for c in self.constraints])
            cds = (ctypes.c_void_p * max(n_con, 1))(*[g._handle for g in con_grids])
            values = np.array([float(c.max_value) for c in self.constraints] or [0.0])
            jitters = np.array([float(c.jitter) for c in self.constraints] or [0.0])
            senses = (ctypes.c_int * max(n_con, 1))(*[SENSE_CODE[c.sense] for c in self.constraints])
            for f in self.factors:
                f.model.ensure_fitted()
            _lib.check(getattr(_lib.load(), self._call)(
                obj.model._handle if obj is not None else None, grids[0]._handle if obj is not None else None,
                float(np.asarray(obj.current_global_min).reshape(-1)[0]) if obj is not None else 0.0,
                _lib.TASK_CODE[obj.task] if obj is not None else 0, float(obj.jitter) if obj is not None else 0.0,
                float(cost), n_con, gps, cds, _lib.dptr(values), _lib.dptr(jitters), senses, _lib.dptr(acq),
                _lib.dptr(ei), _lib.dptr(pof), ctypes.byref(best_val), ctypes.byref(best_idx)))
        finally:
            if own:
                self._close(grids)
        col = lambda a: None if a is None else a[:, None]
        return {"best_val": best_val.value, "best_idx": best_idx.value, "acq": col(acq), self._term_names[0]: col(ei),
                self._term_names[1]: None if pof is None else np.ascontiguousarray(pof.T)}

    def evaluate(self, x):
        """(M,1) value of the product (emukit ``Product.evaluate``)."""
        return self.sweep(_lib.as_f64(x), want_acq=True)["acq"]

    def evaluate_with_gradients(self, x):
        """(value (M,1), gradient (M,d)): the product rule on the host over the factors' own
        ``evaluate_with_gradients``, left to right as emukit's nested Products apply it."""
        x = _lib.as_f64(x)
        f, df = self.factors[0].evaluate_with_gradients(x)
        for factor in self.factors[1:]:
            g, dg = factor.evaluate_with_gradients(x)
            f, df = f * g, df * g + f * dg
        return f, df

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ConstrainedLogExpectedImprovement(AcquisitionProduct):
    """The constrained acquisition in log space: ``log EI + sum_k log PoF_k`` -- and, under a ``Cost``,
    ``- log cost`` -- formed on the device by ``cbo_acq_sweep_constrained_log``.  ``log_ei`` is a
    ``CausalLogExpectedImprovement``, ``constraints`` a list of at most 8 ``ProbabilityOfFeasibility``.  Where the EI, a
    probability or their product underflows to an exact 0.0 -- most of a grid for the noise-free models the exploration
    sets carry -- this is finite and strictly ordered; where the product is representable it is its logarithm.
    ``task='max'`` is ``CausalLogExpectedImprovement``'s mirror, not the product form's ``-EI``.

    The candidate-grid handling is ``AcquisitionProduct``'s; ``sweep`` returns dict(best_val, best_idx, acq, logei,
    logpof)."""
    _call = "cbo_acq_sweep_constrained_log"
    _term_names = ("logei", "logpof")

    def __init__(self, log_ei, constraints):
        from .pointwise_acquisitions import CausalLogExpectedImprovement
        if type(log_ei) is not CausalLogExpectedImprovement:
            raise ValueError(f"log_ei must be a CausalLogExpectedImprovement, not {type(log_ei).__name__}")
        constraints = list(constraints)
        for c in constraints:
            if not isinstance(c, ProbabilityOfFeasibility):
                raise ValueError(f"a constraint must be a ProbabilityOfFeasibility, not {type(c).__name__}")
        if len(constraints) > MAX_CONSTRAINTS:
            raise ValueError(f"at most {MAX_CONSTRAINTS} ProbabilityOfFeasibility constraints, not {len(constraints)}")
        self.objective = log_ei
        self.constraints = constraints
        self.factors = [log_ei] + constraints
        self.model = log_ei.model
        self._cached = None

    def __mul__(self, other):
        raise TypeError("a ConstrainedLogExpectedImprovement is a sum of logarithms: it is not multiplied")

    def __truediv__(self, cost):
        """``log EI + sum log PoF - log cost``: a ``LogAcquisitionQuotient`` (the device call subtracts the logarithm)."""
        from .pointwise_acquisitions import LogAcquisitionQuotient
        return LogAcquisitionQuotient(self, cost)

    @staticmethod
    def log_feasibility(mean, sd, max_value, jitter=0.0, sense="<="):
        """The device's constraint term in numpy / scipy (the host reference): ``log_ndtr(+-(max_value - (mean + jitter)) /
        sd)``."""
        import scipy.special
        u = (float(max_value) - (np.asarray(mean, dtype=np.float64) + jitter)) / np.asarray(sd, dtype=np.float64)
        return scipy.special.log_ndtr(u if sense == "<=" else -u)

    @staticmethod
    def hazard_ratio(u):
        """``pdf(u) / cdf(u) = d log_ndtr / du`` as the device forms it for the refinement under constraints (DESIGN.md §4ab,
        ``log_ndtr_and_ratio``), in numpy / scipy: the plain ratio above ``u = -1``; below, ``sqrt(2 / pi) / erfcx(-u / sqrt
        2)`` -- ``exp(-u^2 / 2)`` cancels analytically, so nothing underflows down to ``u = -1e300``."""
        import scipy.special
        u = np.asarray(u, dtype=np.float64)
        low = u < -1.0
        safe_low, safe_high = np.where(low, u, -2.0), np.where(low, 0.0, u)
        below = 0.797884560802865355880 / scipy.special.erfcx(-safe_low * 7.07106781186547524401E-1)
        above = (np.exp(-(safe_high * safe_high) / 2.0) * 0.3989422804014327) / scipy.special.ndtr(safe_high)
        return np.where(np.isnan(u), np.nan, np.where(low, below, above))

    def evaluate_with_gradients(self, x):
        """(value (M,1), gradient (M,d)) on the host: the log EI's own gradient plus, per constraint,
        ``exp(log pdf(u) - log cdf(u)) du/dx`` -- the ratio from the two logarithms, never from an underflowed ``pdf`` over
        an underflowed ``cdf`` -- with ``du/dx = -(dmean/dx + u dsd/dx) / sd``, the sign flipped for ``">="``."""
        import scipy.special
        x = _lib.as_f64(x)
        f, df = self.objective.evaluate_with_gradients(x)
        for c in self.constraints:
            mean, variance = c.model.predict(x)
            sd = np.sqrt(variance)
            dmean_dx, dvariance_dx = c.model.get_prediction_gradients(x)
            dsd_dx = dvariance_dx / (2 * sd)
            u = (float(c.max_value) - (mean + c.jitter)) / sd
            du_dx = -(dmean_dx + u * dsd_dx) / sd
            if c.sense != "<=":
                u, du_dx = -u, -du_dx
            log_cdf = scipy.special.log_ndtr(u)
            ratio = np.exp((-(u * u) / 2.0 - 0.918938533204672741780) - log_cdf)
            f, df = f + log_cdf, df + ratio * du_dx
        return f, df
