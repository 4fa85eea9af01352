"""Acquisition optimiser of the MI355X path, mirroring the class name and ``optimize`` contract of
/root/reference/src/utils_functions/causal_optimizer.py:15-71.

The reference samples ``num_anchor_points`` uniform random anchors, scores them with one batched
``acquisition.evaluate`` (:52-55), keeps the best and refines it with L-BFGS (:59-65).  Here the batched
scoring IS the optimiser: a deterministic regular grid over the space (BASELINE.json's "N-candidate sweep",
SURVEY.md §0.7), scored on the GPU, arg-max taken on the GPU.  Gradient refinement is SURVEY.md §8 f3.

``anchors="uniform"`` is the reference's own mode, for use under runCBO.py where the trajectory of numpy's global
generator matters (``--seed``, src/ArgumentParser.py:47): ``num_anchor_points`` (100) uniform anchors drawn from the
GLOBAL generator in emukit's order, scored by one batched ``acquisition.evaluate`` (one device sweep), the top one by
``argsort()[::-1][:1]`` as emukit takes it, then L-BFGS from that anchor (scipy ``fmin_l_bfgs_b``, bounds, maxfun=1000 --
emukit's ``OptLbfgs``), whose result is returned as it comes (:59-65: no comparison with the anchor's own value).
emukit is absent here: its order of draws -- ``ParameterSpace.sample_uniform`` samples parameter by
parameter, each ``np.random.uniform(low, high, (n, 1))`` -- is recalled from emukit 0.4.10, parity unpinned.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..graphs import meshgrid_candidates
from .causal_acquisition_functions import CandidateGrid


class CausalGradientAcquisitionOptimizer:
    def __init__(self, space, num_anchor_points=None, grid_shape=None, anchors="grid"):
        """``space``: emukit ParameterSpace / object with ``parameters`` / list of (lo, hi).  ``anchors="grid"``
        (default): ``grid_shape`` (points per dimension) defaults to ``default_grid_shape``; ``num_anchor_points``, if
        given, is used as the candidate budget instead of 16384.  ``anchors="uniform"``: the reference's 100 (or
        ``num_anchor_points``) uniform random anchors and L-BFGS from the best (module docstring)."""
        from .utils import default_grid_shape, space_bounds
        if anchors not in ("grid", "uniform"):
            raise ValueError(f"anchors must be 'grid' or 'uniform', not {anchors!r}")
        self.space = space
        self.bounds = space_bounds(space)
        self.anchors = anchors
        self.num_anchor_points = 100 if num_anchor_points is None else int(num_anchor_points)    # (causal_optimizer.py:19)
        self.grid_shape = list(grid_shape) if grid_shape is not None else default_grid_shape(
            len(self.bounds), budget=num_anchor_points)
        self._grid, self._grid_model = None, None

    def sample_uniform(self, point_count):
        """emukit ``ParameterSpace.sample_uniform`` on the GLOBAL numpy generator (``sample_uniform`` below)."""
        return sample_uniform(self.bounds, point_count)

    def optimize_from_uniform_anchors(self, acquisition):
        """The reference's ``_optimize`` (:26-65) for a space without context or constraints."""
        x_anchors = self.sample_uniform(self.num_anchor_points)
        scores = np.asarray(acquisition.evaluate(x_anchors), dtype=np.float64)[:, 0]      # ONE batched device sweep (:52-55)
        anchor = x_anchors[np.argsort(scores)[::-1][:1]]                                # emukit AnchorPointsGenerator.get
        return self.refine(acquisition, anchor)                                         # OptLbfgs from it (:59-65)

    def candidates(self):
        return meshgrid_candidates(self.bounds, self.grid_shape)

    def refine(self, acquisition, x0):
        """The reference's second stage (causal_optimizer.py:59-65; emukit OptLbfgs = scipy fmin_l_bfgs_b with
        bounds and maxfun=1000, minimising -acquisition with its gradient) started from ``x0`` ((1,d))."""
        from scipy.optimize import fmin_l_bfgs_b

        def f_df(v):
            f, df = acquisition.evaluate_with_gradients(v[None, :])
            return -float(f[0, 0]), -df[0]

        x, fx, _ = fmin_l_bfgs_b(f_df, np.asarray(x0, dtype=np.float64).reshape(-1), bounds=self.bounds, maxfun=1000)
        return x[None, :], np.array([[-fx]])

    def refine_batched(self, acquisition, x0, max_rounds=200, history=8):
        """Multi-start refinement ("batched multi-start L-BFGS from top-k grid points"): every row of
        ``x0`` ((k,d)) is the start of its own projected L-BFGS ascent, and the k searches advance in lockstep -- one
        ``evaluate_with_gradients`` call on a (k,d) batch per round (one pair of batched device solves), whatever each
        search is doing (a first trial step, a backtracked one).  Returns (points (k,d), values (k,))."""
        lo = np.array([b[0] for b in self.bounds], dtype=np.float64)
        hi = np.array([b[1] for b in self.bounds], dtype=np.float64)
        return lockstep_lbfgs(lambda X: _values_and_gradients(acquisition, X), np.asarray(x0, dtype=np.float64), lo, hi,
                              max_rounds=max_rounds, history=history)

    def optimize(self, acquisition, context=None, refine=False, num_starts=1, device=False, device_prior=False,
                 cost_mode="batch"):
        """(x_max (1,d), acquisition value at x_max (1,1)) -- emukit ``AcquisitionOptimizerBase.optimize``.
        ``acquisition`` is ``CausalExpectedImprovement(...) / Cost(...)`` (an ``AcquisitionQuotient``) or a bare
        ``CausalExpectedImprovement``.  ``refine=True`` adds the reference's gradient stage: from the best grid point
        with scipy's L-BFGS-B (``num_starts=1``, what the reference does with its best anchor), or from the
        ``num_starts`` best grid points at once (``refine_batched``).  ``device=True`` (with ``refine=True``) runs the
        searches from the ``num_starts`` best grid points inside one device launch (``refine_sets``) and
        raises ``ValueError`` when the set is not eligible for it: a causal, large or fp32 model, a cost that is not the
        graphs' own, an acquisition the launch does not know.  ``device_prior=True`` (with ``refine=True`` and
        ``device=True``) lets a causal set into the launch through a device-resident do-calculus prior (``DoPrior``, DESIGN.md
        §4u) when ``prior_spec`` recognises its closures.  The default is today's path.
        ``cost_mode="pointwise"`` says that ``acquisition`` is a quotient by a ``PointwiseCost``: the grid is
        scored per candidate over its own cost and the device form of the refinement climbs with the cost's own gradient
        (``cbo_acq_refine_sets_pointcost``); a mismatch between the keyword and the quotient raises ``ValueError``."""
        from .cost_functions import checked_cost_mode
        if (checked_cost_mode(cost_mode) == "pointwise") != bool(getattr(acquisition, "pointwise_cost", False)):
            raise ValueError("cost_mode='pointwise' goes with acquisition / PointwiseCost(...), cost_mode='batch' with "
                             "acquisition / Cost(...)")
        if cost_mode == "pointwise" and device_prior:
            raise ValueError("cost_mode='pointwise' refines causal sets through the host route: device_prior must be False")
        if device_prior and not refine:
            raise ValueError("device_prior=True selects the device form of a causal set's refinement: refine must be True")
        if device_prior and not device:
            raise ValueError("device_prior=True belongs to the device form of the refinement: device must be True")
        if device and not refine:
            raise ValueError("device=True selects the device form of the refinement: refine must be True")
        if (refine or self.anchors == "uniform") and not has_gradients(acquisition):
            raise ValueError(f"{type(_numerator(acquisition)).__name__} has no gradients: it cannot be refined with "
                             "L-BFGS (use refine=False and anchors='grid')")
        if self.anchors == "uniform":
            return self.optimize_from_uniform_anchors(acquisition)
        # the grid of this optimiser stays on the device while the model object is the same (no allocation per call)
        model = acquisition.model
        if self._grid is None or self._grid_model is not model:
            if self._grid is not None:
                self._grid.close()
            self._grid, self._grid_model = CandidateGrid(self.candidates(), model), model
        grid, pts = self._grid, self._grid.points
        k = max(1, min(int(num_starts), pts.shape[0])) if refine else 1
        res = acquisition.sweep(grid, want_acq=k > 1)
        x = pts[res["best_idx"]][None, :].copy()
        fx = np.array([[res["best_val"]]])
        if refine and device:
            kind, model, y_best, task, cost = _device_refinable(acquisition, device_prior)
            if k > 1:
                acq = np.asarray(res["acq"], dtype=np.float64).reshape(-1)
                top = np.argpartition(-acq, k - 1)[:k]
                starts = pts[top[np.argsort(-acq[top], kind="stable")]]
            else:
                starts = x
            cons = _product_constraints(_numerator(acquisition))
            (xs, fs, status), = refine_sets([model], [starts], [self.bounds], y_best, task, [cost], kind=kind,
                                            host_fallback=False, device_prior=device_prior, cost_mode=cost_mode,
                                            constraints=None if cons is None else [cons])
            if status[0] == _lib.REFINE_DECLINED:
                raise ValueError("device=True: the device launch declined the set (its model is not positive definite "
                                 "without jitter, or the one-workgroup kernels are switched off with CBO_HIP_SMALL_SETS=0)")
            best = int(np.argmax(fs))
            if fs[best] >= fx[0, 0]:
                x, fx = xs[best][None, :].copy(), np.array([[fs[best]]])
        elif refine and k == 1:
            xr, fr = self.refine(acquisition, x)
            if fr[0, 0] >= fx[0, 0]:
                x, fx = xr, fr
        elif refine:
            acq = np.asarray(res["acq"], dtype=np.float64).reshape(-1)
            top = np.argpartition(-acq, k - 1)[:k]
            top = top[np.argsort(-acq[top], kind="stable")]
            xs, fs = self.refine_batched(acquisition, pts[top])
            best = int(np.argmax(fs))
            if fs[best] >= fx[0, 0]:
                x, fx = xs[best][None, :].copy(), np.array([[fs[best]]])
        return x, fx


def sample_uniform(bounds, point_count):
    """emukit ``ParameterSpace.sample_uniform`` on the GLOBAL numpy generator: one ``np.random.uniform(low, high,
    (point_count, 1))`` per parameter, in the parameters' order, stacked as columns."""
    return np.hstack([np.random.uniform(low=lo, high=hi, size=(point_count, 1)) for lo, hi in bounds])


def _numerator(acquisition):
    num = getattr(acquisition, "numerator", None)
    return acquisition if num is None else num


def has_gradients(acquisition):
    """Whether ``acquisition`` can be refined by gradient: for a quotient, whether its numerator can (the quotient reports
    gradients whatever it divides, as emukit's does).  An object that does not say is taken to have them."""
    return bool(getattr(_numerator(acquisition), "has_gradients", True))


def _values_and_gradients(acquisition, X):
    """(values (k,), gradients (k,d)) of every row of X taken as a batch of ONE point: the posterior and its gradients
    for all rows come from one batched device call; a cost that depends on the point (cost_functions.py:11-17 sums
    |x| over the batch it is given) is evaluated row by row, as k single-point calls of the reference would."""
    num = getattr(acquisition, "numerator", None)
    if num is None or getattr(acquisition, "pointwise_cost", False):   # (PointCostQuotient prices every row itself)
        f, df = acquisition.evaluate_with_gradients(X)
        return f[:, 0], df
    f, df = num.evaluate_with_gradients(X)
    c = np.array([float(acquisition.denominator.evaluate(X[i:i + 1])) for i in range(X.shape[0])])
    if getattr(acquisition, "is_log", False):         # (LogAcquisitionQuotient: the logarithm of the quotient)
        return f[:, 0] - np.log(c), df
    return f[:, 0] / c, df / c[:, None]


def lockstep_lbfgs(fun, x0, lo, hi, max_rounds=200, history=8, pgtol=1e-5, ftol=2.2e-9, c1=1e-4):
    """Maximise ``fun`` over the box [lo, hi] from every row of ``x0`` at once.  ``fun(X)`` -> (values (k,),
    gradients (k,d)) is called ONCE per round on the (k,d) array of the searches' current trial points.  Each search
    is a projected L-BFGS iteration with Armijo backtracking (two-loop recursion over ``history`` pairs, steps
    clipped to the box, curvature pairs with s.y <= 0 dropped); a search that has converged (projected gradient below
    ``pgtol``, relative gain below ``ftol`` -- scipy's L-BFGS-B defaults -- or a vanishing step) keeps its point and
    is re-evaluated along with the others (the batch shape stays fixed).  Returns (points (k,d), values (k,))."""
    X = np.clip(np.asarray(x0, dtype=np.float64).copy(), lo, hi)
    k, d = X.shape
    F, G = fun(X)
    F, G = -np.asarray(F, dtype=np.float64), -np.asarray(G, dtype=np.float64)          # minimise -fun
    S = [[] for _ in range(k)]
    Y = [[] for _ in range(k)]
    done = np.zeros(k, dtype=bool)
    D = np.zeros((k, d))
    T = np.zeros(k)

    def projected_gradient(x, g):
        pg = g.copy()
        pg[(x <= lo) & (g > 0)] = 0.0                # cannot go below the lower bound
        pg[(x >= hi) & (g < 0)] = 0.0
        return pg

    def direction(i):
        pg = projected_gradient(X[i], G[i])
        q = pg.copy()
        alphas = []
        for s, y in zip(reversed(S[i]), reversed(Y[i])):
            a = s.dot(q) / y.dot(s)
            alphas.append(a)
            q -= a * y
        if S[i]:
            q *= S[i][-1].dot(Y[i][-1]) / Y[i][-1].dot(Y[i][-1])
        for (s, y), a in zip(zip(S[i], Y[i]), reversed(alphas)):
            q += (a - y.dot(q) / y.dot(s)) * s
        dvec = -q
        if dvec.dot(pg) >= 0.0:                      # not a descent direction (stale curvature at a bound)
            dvec = -pg
            S[i].clear(); Y[i].clear()
        return dvec, pg

    for i in range(k):
        D[i], pg = direction(i)
        n = np.linalg.norm(pg)
        done[i] = np.max(np.abs(pg)) <= pgtol
        T[i] = min(1.0, 1.0 / n) if n > 0 else 0.0
    for _ in range(max_rounds):
        if done.all():
            break
        trial = np.where(done[:, None], X, np.clip(X + T[:, None] * D, lo, hi))
        Ft, Gt = fun(trial)
        Ft, Gt = -np.asarray(Ft, dtype=np.float64), -np.asarray(Gt, dtype=np.float64)
        for i in range(k):
            if done[i]:
                continue
            step = trial[i] - X[i]
            if not np.isfinite(Ft[i]) or Ft[i] > F[i] + c1 * G[i].dot(step):
                T[i] *= 0.5                          # Armijo failed: shorter step next round
                if T[i] * np.max(np.abs(D[i])) < 1e-14:
                    done[i] = True
                continue
            y = Gt[i] - G[i]
            gain = F[i] - Ft[i]
            if step.dot(y) > 1e-12 * np.linalg.norm(step) * np.linalg.norm(y):
                S[i].append(step.copy()); Y[i].append(y)
                if len(S[i]) > history:
                    S[i].pop(0); Y[i].pop(0)
            small = gain <= ftol * max(abs(F[i]), abs(Ft[i]), 1.0)
            X[i], F[i], G[i] = trial[i], Ft[i], Gt[i]
            D[i], pg = direction(i)
            T[i] = 1.0
            if small or np.max(np.abs(pg)) <= pgtol:
                done[i] = True
    return X, -F



def cost_structure(cost):
    """``(fix (d,), variable (d,) int32)`` of a ``Cost`` whose every function, for its own evaluated set, is a
    ``functools.partial`` of ``graphs.cost`` with both parameters bound -- what ``get_cost_structure`` builds, for all four
    cost types -- so that a one-row cost is ``(fix_0 + variable_0 |x_0|) + (fix_1 + ...) + ...`` from 0; ``None`` for anything
    else (a lambda, another callable, keyword arguments): such a cost can only be evaluated in Python."""
    import functools
    from ..graphs import cost as graph_cost
    fix, variable = [], []
    for name in getattr(cost, "evaluated_set", ()):
        f = getattr(cost, "costs_functions", {}).get(name)
        if not isinstance(f, functools.partial) or f.func is not graph_cost or len(f.args) != 2 or f.keywords:
            return None
        fixed, var = f.args
        if isinstance(fixed, (bool, np.bool_)) or not isinstance(fixed, (int, float, np.integer, np.floating)):
            return None
        if not np.isfinite(float(fixed)):
            return None
        fix.append(float(fixed))
        variable.append(1 if var is True else 0)          # (graphs.cost adds the variable part for ``True`` alone)
    if not fix:
        return None
    return np.array(fix, dtype=np.float64), np.array(variable, dtype=np.int32)


def one_row_cost(fix, variable, x):
    """``Cost.evaluate`` of the one-row batch ``x`` ((d,)) from ``cost_structure``'s pair, bit for bit: the terms added
    from 0 in the evaluated set's order -- the arithmetic of the device launch."""
    c = 0.0
    for f, v, xi in zip(fix, variable, x):
        c = c + (f + abs(float(xi)) if v else f)
    return c


def _device_refinable(acquisition, device_prior=False):
    """(kind, model, y_best, task, Cost) of an acquisition ``optimize(device=True)`` can hand to ``refine_sets``;
    ``ValueError`` says why another cannot."""
    from .causal_acquisition_functions import CausalExpectedImprovement
    from . import pointwise_acquisitions as pw
    from .constrained import ConstrainedLogExpectedImprovement
    from .cost_functions import Cost
    num, cost = getattr(acquisition, "numerator", None), getattr(acquisition, "denominator", None)
    if num is None or not isinstance(cost, Cost):
        raise ValueError("device=True refines acquisition / Cost(...): the acquisition must be such a quotient")
    cons = _product_constraints(num)
    if cons is not None:                             # (the constrained launch; the objective names the form)
        if device_prior:
            raise ValueError("device=True: constraints are not refined with a device-resident prior: device_prior must be False")
        obj = num.objective
        if isinstance(num, ConstrainedLogExpectedImprovement):
            y_best, task, param = obj._scalars()
            kind = ("LOGCEI", param)
        else:
            kind = ("EI", float(obj.jitter) if obj.jitter != 0.0 else None)
            y_best, task = float(np.asarray(obj.current_global_min, dtype=np.float64).reshape(-1)[0]), obj.task
        why = _not_eligible(obj.model, cost)
        for c in cons:
            why = why or _constraint_not_eligible(obj.model, c.model)
        if why:
            raise ValueError(f"device=True: {why}")
        return kind, obj.model, y_best, task, cost
    if type(num) is CausalExpectedImprovement:
        kind = ("EI", None)
        if num.jitter != 0.0:
            kind = ("EI", float(num.jitter))
        y_best, task = float(np.asarray(num.current_global_min, dtype=np.float64).reshape(-1)[0]), num.task
    elif isinstance(num, pw._PointwiseAcquisition) and (num.kind in _lib.ACQ_KIND_CODE or num.kind == _lib.LOGEI):
        y_best, task, param = num._scalars()
        kind = (num.kind, param)
    else:
        raise ValueError(f"device=True: {type(num).__name__} is not an acquisition the device launch refines")
    why = _not_eligible(num.model, cost, device_prior)
    if why:
        raise ValueError(f"device=True: {why}")
    return kind, num.model, y_best, task, cost


def _product_constraints(numerator):
    """The ``ProbabilityOfFeasibility`` factors of a numerator the constrained launch refines -- an ``AcquisitionProduct`` with
    an objective, or a ``ConstrainedLogExpectedImprovement`` -- else ``None``."""
    from .constrained import AcquisitionProduct
    if isinstance(numerator, AcquisitionProduct) and numerator.objective is not None:
        return list(numerator.constraints)
    return None


def _not_eligible(model, cost, device_prior=False):
    """Why the device launch does not take this (model, Cost), or None when it does.  ``device_prior``: a causal model whose
    closures ``prior_spec`` recognises is taken (its ``DoPrior`` has yet to be created: that can still decline it)."""
    if getattr(model, "causal", False):
        if not device_prior:
            return "a causal model's prior closures are Python: they cannot be evaluated at a moving point on the device"
        from ..DoCalculus import prior_spec
        if prior_spec(model) is None:
            return "the causal model's prior closures are not the do-calculus closures of DoCalculus.py"
    if not getattr(model, "small", False):
        return "the model has more than 128 observations or is fp32"
    if cost_structure(cost) is None:
        return "the cost is not a table of functools.partial(graphs.cost, fix, variable)"
    return None


def _acquisition_of_kind(kind, model, current_global_best, task, cost):
    from .causal_acquisition_functions import CausalExpectedImprovement
    from .utils import _acquisition_for
    if kind[0] == "EI":
        return CausalExpectedImprovement(current_global_best, task, model, 0.0 if kind[1] is None else kind[1]) / cost
    return _acquisition_for(kind[0], model, current_global_best, task, None, None if kind[0] == "VAR" else kind[1]) / cost


def _refine_on_device(dev, priors, models, X0, los, his, costs, kind, y_best, task, param, max_rounds, out,
                      pointwise=False):
    """``refine_sets``' one library call for the sets ``dev`` (``priors``: the ``DoPrior`` of each causal one): fills ``out[i]``
    of every set the launch took."""
    import ctypes
    if not dev:
        return
    n = len(dev)
    sets, structs, (x_out, v_out, g_out, rounds, status) = _refine_call_arrays(dev, X0, los, his, costs)
    gps = (ctypes.c_void_p * n)(*[models[i]._handle for i in dev])
    yb = np.full(n, y_best)
    if pointwise:                                    # (the gradient carries the cost's own derivative)
        _lib.check(_lib.load().cbo_acq_refine_sets_pointcost(
            n, gps, sets, int(kind[0] == _lib.LOGEI), _lib.dptr(yb), _lib.TASK_CODE[task], param, max_rounds,
            _lib.dptr(x_out), _lib.dptr(v_out), _lib.dptr(g_out), rounds.ctypes.data_as(_lib.c_int_p),
            status.ctypes.data_as(_lib.c_int_p)))
        outs = None
    elif kind[0] == _lib.LOGEI:                      # (no kind code: an entry point of its own; refine_sets has refused priors)
        _lib.check(_lib.load().cbo_acq_refine_sets_logei(
            n, gps, sets, _lib.dptr(yb), _lib.TASK_CODE[task], param, max_rounds, _lib.dptr(x_out), _lib.dptr(v_out),
            _lib.dptr(g_out), rounds.ctypes.data_as(_lib.c_int_p), status.ctypes.data_as(_lib.c_int_p)))
        outs = None
    else:
        outs = (_lib.REFINE_KIND_CODE[kind[0]], _lib.dptr(yb), _lib.TASK_CODE[task], param, max_rounds, _lib.dptr(x_out),
                _lib.dptr(v_out), _lib.dptr(g_out), rounds.ctypes.data_as(_lib.c_int_p), status.ctypes.data_as(_lib.c_int_p))
    if outs is None:
        pass
    elif priors:
        handles = (ctypes.c_void_p * n)(*[priors[i]._handle if i in priors else None for i in dev])
        _lib.check(_lib.load().cbo_acq_refine_sets_prior(n, gps, sets, handles, *outs))
    else:
        _lib.check(_lib.load().cbo_acq_refine_sets(n, gps, sets, *outs))
    _refine_call_harvest(dev, X0, x_out, v_out, status, out)


def _refine_call_arrays(dev, X0, los, his, costs):
    """The ``cbo_refine_set`` array of the sets ``dev``, the cost tables it points into (kept alive by the caller) and the
    five output arrays of a refinement call, laid out as the library lays them out."""
    n = len(dev)
    structs = [cost_structure(costs[i]) for i in dev]
    for i, (fix, _) in zip(dev, structs):
        if not fix.sum() > 0.0:
            raise ValueError(f"refine_sets: the fixed costs of set {i} must sum to a positive cost")
    sets = (_lib.CboRefineSet * n)()
    for j, i in enumerate(dev):
        fix, variable = structs[j]
        sets[j].k = X0[i].shape[0]
        sets[j].starts = X0[i].ctypes.data_as(_lib.c_double_p)
        sets[j].lo = los[i].ctypes.data_as(_lib.c_double_p)
        sets[j].hi = his[i].ctypes.data_as(_lib.c_double_p)
        sets[j].cost_fix = fix.ctypes.data_as(_lib.c_double_p)
        sets[j].cost_variable = variable.ctypes.data_as(_lib.c_int_p)
    rows = sum(X0[i].size for i in dev)
    total = sum(X0[i].shape[0] for i in dev)
    return sets, structs, (np.zeros(rows), np.zeros(total), np.zeros(rows), np.zeros(total, dtype=np.int32),
                           np.zeros(total, dtype=np.int32))


def _refine_call_harvest(dev, X0, x_out, v_out, status, out):
    """``out[i]`` of every set of ``dev`` the launch took, from the call's flat output arrays."""
    r0 = o0 = 0
    for i in dev:
        k, d = X0[i].shape
        if status[o0] != _lib.REFINE_DECLINED:
            out[i] = (x_out[r0:r0 + k * d].reshape(k, d).copy(), v_out[o0:o0 + k].copy(), status[o0:o0 + k].copy())
        r0 += k * d
        o0 += k


def _checked_refine_constraints(constraints, n_sets, kind, device_prior, cost_mode):
    """``refine_sets``' ``constraints``, checked on the host before any device call: per set a list of at most 8
    ``ProbabilityOfFeasibility`` under the product form (``"EI"``) or the log form (``"LOGCEI"``) alone, with one cost per
    point from the sets' tables and no device-resident prior."""
    from .constrained import MAX_CONSTRAINTS, ProbabilityOfFeasibility
    if kind[0] == "LOGCEI" and constraints is None:
        raise ValueError("refine_sets: kind 'LOGCEI' sums the logarithms of the constraints' probabilities: constraints must "
                         "be given (without constraints the kind is 'LOGEI')")
    if constraints is None:
        return None
    if kind[0] not in ("EI", "LOGCEI"):
        raise ValueError("refine_sets: constraints multiply the causal EI: kind must be ('EI', jitter or None) or "
                         f"('LOGCEI', jitter), not {kind[0]!r}")
    if device_prior:
        raise ValueError("refine_sets: constraints are not refined with a device-resident prior: device_prior must be False")
    if cost_mode != "batch":
        raise ValueError("refine_sets: constraints are refined with the reference's zero cost gradient: cost_mode must be "
                         f"'batch', not {cost_mode!r}")
    if not hasattr(constraints, "__len__") or len(constraints) != n_sets:
        raise ValueError(f"refine_sets: constraints must have one list per exploration set ({n_sets})")
    checked = []
    for i, cons in enumerate(constraints):
        cons = list(cons or [])
        if len(cons) > MAX_CONSTRAINTS:
            raise ValueError(f"refine_sets: at most {MAX_CONSTRAINTS} constraints per set, not {len(cons)} (set {i})")
        for c in cons:
            if not isinstance(c, ProbabilityOfFeasibility):
                raise ValueError(f"refine_sets: a constraint must be a ProbabilityOfFeasibility, not {type(c).__name__} "
                                 f"(set {i})")
        checked.append(cons)
    return checked


def _constrained_acquisition(kind, model, current_global_best, task, cost, cons):
    """The host acquisition of a constrained set: ``AcquisitionProduct([EI] + cons) / cost`` or
    ``ConstrainedLogExpectedImprovement(log EI, cons) / cost`` -- what the device launch climbs."""
    from .causal_acquisition_functions import CausalExpectedImprovement
    from .constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement
    jitter = 0.0 if kind[1] is None else float(kind[1])
    if kind[0] == "LOGCEI":
        from .pointwise_acquisitions import CausalLogExpectedImprovement
        return ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(current_global_best, task, model, jitter),
                                                 cons) / cost
    return AcquisitionProduct([CausalExpectedImprovement(current_global_best, task, model, jitter)] + list(cons)) / cost


def _constraint_not_eligible(model, con_model):
    """Why the constrained launch does not take a set with this constraint model, or None when it does."""
    if getattr(con_model, "causal", False):
        return "a causal constraint model's prior closures are Python"
    if not getattr(con_model, "small", False):
        return "a constraint model has more than 128 observations or is fp32"
    if con_model.input_dim != model.input_dim:
        return "a constraint model's input dimension differs from the set's"
    return None


def _refine_constrained_on_device(dev, models, cons, X0, los, his, costs, kind, y_best, task, param, max_rounds, out):
    """``refine_sets``' one library call for the sets ``dev`` under constraints (``cbo_acq_refine_sets_constrained``, DESIGN.md
    §4ab): fills ``out[i]`` of every set the launch took."""
    import ctypes
    from .constrained import SENSE_CODE
    if not dev:
        return
    n = len(dev)
    sets, structs, (x_out, v_out, g_out, rounds, status) = _refine_call_arrays(dev, X0, los, his, costs)
    gps = (ctypes.c_void_p * n)(*[models[i]._handle for i in dev])
    flat = [c for i in dev for c in cons[i]]
    n_con = (ctypes.c_int * n)(*[len(cons[i]) for i in dev])
    con_gps = (ctypes.c_void_p * max(len(flat), 1))(*[c.model._handle for c in flat])
    values = np.array([float(c.max_value) for c in flat] or [0.0])
    jitters = np.array([float(c.jitter) for c in flat] or [0.0])
    senses = (ctypes.c_int * max(len(flat), 1))(*[SENSE_CODE[c.sense] for c in flat])
    _lib.check(_lib.load().cbo_acq_refine_sets_constrained(
        n, gps, sets, int(kind[0] == "LOGCEI"), _lib.dptr(np.full(n, y_best)), _lib.TASK_CODE[task], param, n_con, con_gps,
        _lib.dptr(values), _lib.dptr(jitters), senses, max_rounds, _lib.dptr(x_out), _lib.dptr(v_out), _lib.dptr(g_out),
        rounds.ctypes.data_as(_lib.c_int_p), status.ctypes.data_as(_lib.c_int_p)))
    _refine_call_harvest(dev, X0, x_out, v_out, status, out)


def refine_sets(models, starts, bounds, current_global_best, task, costs, kind=("EI", None), max_rounds=200,
                host_fallback=True, device_prior=False, cost_mode="batch", constraints=None):
    """The reference's second stage (causal_optimizer.py:59-65) for every exploration set at once: from every row of
    ``starts[s]`` ((k_s, d_s), 1 <= k_s <= 64) a projected L-BFGS ascent of ``acquisition / Cost`` inside ``bounds[s]``
    (``lockstep_lbfgs``'s iteration), returning per set ``(points (k_s, d_s), values (k_s,), status (k_s,) int)``.
    Eligible sets -- a non-causal fp64 model of at most 128 observations whose ``costs[s]`` ``cost_structure`` recognises --
    advance inside ONE device launch (``cbo_acq_refine_sets``, DESIGN.md §4q: the model factored in LDS once, every round's
    value and gradient from one tile solve); ``status`` is the launch's reason for stopping (``_lib.REFINE_*``).  Every
    other set, and a set the launch declined, goes through ``refine_batched`` inside the same call: its points and values
    are that method's own and its status entries are ``_lib.REFINE_DECLINED``.
    ``kind`` is ``sets_acquisition``'s pair: ``("EI", None)``, ``("LCB", beta)``, ``("PI", jitter)``, ``("MPEI", jitter)``,
    ``("VAR", 0.0)`` -- it is checked and completed by ``sets_acquisition`` here, so a ``None`` parameter means the kind's
    default (beta 1, jitter 0) on both routes; ``("EI", jitter)`` with a finite jitter is accepted too (what
    ``optimize(device=True)`` passes for a jittered EI) and reaches both routes.  Models are only read by the launch; the
    host route fits a model that is not.  ``host_fallback=False``: a set the launch does not take is not refined at all --
    its points are its starts, its values NaN, its status ``_lib.REFINE_DECLINED``.
    ``device_prior=True``: a causal set is eligible too when ``prior_spec`` recognises its closures, its model
    is small and fp64, ``cost_structure`` recognises its cost and a ``DoPrior`` of its graph GP can be created
    (``cbo_acq_refine_sets_prior``); the priors are built for this call and closed after it.  A causal set that misses one of
    these takes today's route.  The default does exactly what it did.
    ``kind=("LOGEI", jitter)``: value ``log EI - log cost``, gradient ``d log EI``, through
    ``cbo_acq_refine_sets_logei``; a causal set takes the host route, and ``device_prior=True`` raises ``ValueError``.
    ``cost_mode="pointwise"`` (``("EI", ...)`` and ``("LOGEI", ...)`` alone, no ``device_prior``): the same
    values with the TRUE gradient of ``EI / c`` or ``log EI - log c`` -- ``d c / d x_k = variable_k sign(x_k)`` -- through
    ``cbo_acq_refine_sets_pointcost``; the sets the launch does not take go through ``refine_batched`` with
    ``acquisition / PointwiseCost``, the same gradient on the host.  Every cost must be one ``cost_structure`` recognises.
    ``constraints`` (per set a list of at most 8 ``ProbabilityOfFeasibility``, possibly empty) with
    ``kind=("EI", jitter | None)`` -- ``EI prod PoF / cost`` -- or ``("LOGCEI", jitter)`` -- ``log EI + sum log PoF - log cost``:
    the sets all of whose models are non-causal, fp64, of at most 128 observations and of the set's dimension advance inside
    one launch of ``cbo_acq_refine_sets_constrained`` (a set with an empty list inside the unconstrained launch of the same
    call); every other set, and every set the launch declines, goes through ``refine_batched`` with ``AcquisitionProduct([...])
    / cost`` or ``ConstrainedLogExpectedImprovement(...) / cost``.  Another kind, ``device_prior=True`` and
    ``cost_mode="pointwise"`` raise ``ValueError`` with constraints, as does ``"LOGCEI"`` without them."""
    import ctypes
    import math
    from .utils import checked_log_ei, checked_pointwise_cost, sets_acquisition
    if not (isinstance(kind, tuple) and len(kind) == 2):
        raise ValueError(f"refine_sets: kind must be a (name, parameter) pair, not {kind!r}")
    if kind[0] == "MES":
        raise ValueError("refine_sets: acquisition must be 'EI', 'LCB', 'PI', 'MPEI' or 'VAR', not 'MES'")
    if kind[0] == "EI" and kind[1] is not None:
        if isinstance(kind[1], bool) or not isinstance(kind[1], (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(kind[1])):
            raise ValueError(f"refine_sets: the EI's jitter must be a finite number, not {kind[1]!r}")
        kind = ("EI", float(kind[1]))
    else:
        kind = sets_acquisition(kind[0], None if kind[0] in ("EI", "VAR") else kind[1])
    checked_log_ei(kind, device_prior)
    s = len(models)
    constraints = _checked_refine_constraints(constraints, s, kind, device_prior, cost_mode)
    pointwise = checked_pointwise_cost(cost_mode, kind, device_prior=device_prior)
    if pointwise:
        from .cost_functions import PointwiseCost
        costs = [c if isinstance(c, PointwiseCost) else PointwiseCost(getattr(c, "costs_functions", None) or {},
                                                                      getattr(c, "evaluated_set", ())) for c in costs]
    if not (len(starts) == len(bounds) == len(costs) == s) or s == 0:
        raise ValueError("refine_sets: models, starts, bounds and costs must have one entry per exploration set")
    if task not in _lib.TASK_CODE:
        raise ValueError(f"task must be 'min' or 'max', not {task!r}")
    max_rounds = int(max_rounds)
    if not 0 <= max_rounds <= _lib.REFINE_ROUNDS_LIMIT:
        raise ValueError(f"max_rounds must be in 0..{_lib.REFINE_ROUNDS_LIMIT}, not {max_rounds}")
    y_best = float(np.asarray(current_global_best, dtype=np.float64).reshape(-1)[0])
    param = 0.0 if kind[1] is None else float(kind[1])
    X0, los, his = [], [], []
    for i in range(s):
        x0 = _lib.as_f64(starts[i])
        d = models[i].input_dim
        if x0.ndim != 2 or x0.shape[1] != d or not 1 <= x0.shape[0] <= _lib.REFINE_MAX_STARTS:
            raise ValueError(f"refine_sets: starts of set {i} must be (k, {d}) with 1 <= k <= {_lib.REFINE_MAX_STARTS}, "
                             f"not {x0.shape}")
        lo = np.array([b[0] for b in bounds[i]], dtype=np.float64)
        hi = np.array([b[1] for b in bounds[i]], dtype=np.float64)
        if lo.shape != (d,) or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
            raise ValueError(f"refine_sets: bounds of set {i} must be {d} finite (lo, hi) pairs with lo <= hi")
        if not np.all(np.isfinite(x0)):
            raise ValueError(f"refine_sets: starts of set {i} must be finite")
        X0.append(x0); los.append(lo); his.append(hi)
    out = [None] * s
    dev = [i for i in range(s) if _not_eligible(models[i], costs[i], device_prior) is None]
    priors = {}
    if device_prior:
        from ..DoCalculus import DoPrior, prior_spec
        for i in list(dev):
            if not getattr(models[i], "causal", False):
                continue
            try:
                priors[i] = DoPrior(*prior_spec(models[i]))
                if priors[i].n_iv != models[i].input_dim:
                    raise ValueError("the prior's value columns are not the model's inputs")
            except (_lib.CboHipError, ValueError):
                if i in priors:
                    priors.pop(i).close()
                dev.remove(i)                  # (unsupported graph GP: today's route)
    try:
        if constraints is not None:
            dev = [i for i in dev if all(_constraint_not_eligible(models[i], c.model) is None for c in constraints[i])]
            _refine_constrained_on_device(dev, models, constraints, X0, los, his, costs, kind, y_best, task, param, max_rounds,
                                          out)
        else:
            _refine_on_device(dev, priors, models, X0, los, his, costs, kind, y_best, task, param, max_rounds, out, pointwise)
    finally:
        for p in priors.values():
            p.close()

    for i in range(s):
        if out[i] is None and not host_fallback:
            out[i] = (X0[i].copy(), np.full(X0[i].shape[0], np.nan), np.full(X0[i].shape[0], _lib.REFINE_DECLINED, dtype=np.int32))
        if out[i] is None:
            acq = (_acquisition_of_kind(kind, models[i], current_global_best, task, costs[i]) if constraints is None else
                   _constrained_acquisition(kind, models[i], current_global_best, task, costs[i], constraints[i]))
            x, f = CausalGradientAcquisitionOptimizer(list(zip(los[i].tolist(), his[i].tolist()))).refine_batched(
                acq, X0[i], max_rounds=max_rounds)
            out[i] = (x, f, np.full(X0[i].shape[0], _lib.REFINE_DECLINED, dtype=np.int32))
    return out
