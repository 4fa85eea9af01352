"""Many independent ``scipy.optimize.fmin_l_bfgs_b`` runs advanced together, one batched evaluation per round.

An observe step of the reference (src/CBO.py:123-141) fits one graph-level GP per fit dependency, each with GPy's
``gp.optimize()`` (src/utils_functions/utils.py:40-45): paramz runs ``fmin_l_bfgs_b(f_fp, x0, maxfun=1000,
maxiter=1000)`` on every model in turn.  The problems are independent, so each round here asks every run that is
still going which point it wants evaluated next, evaluates all those points in ONE call (``evaluate``: on the device,
one launch for every small model) and hands the values back.

Each run is scipy's own L-BFGS-B: the reverse-communication loop of ``_minimize_lbfgsb`` (scipy 1.15,
``_lbfgsb.setulb``) restated with one state per problem, with ``fmin_l_bfgs_b``'s defaults and the bookkeeping of
its ``ScalarFunction`` (the start point evaluated first, a point equal to the last one not evaluated again, ``nfev``
counting evaluations, the ``maxiter`` / ``maxfun`` stops).  Every problem therefore follows exactly the trajectory it
would follow alone.  ``setulb`` is private: when its signature is not the one this loop was written against, the
problems are solved one after another with ``fmin_l_bfgs_b`` itself (a warning says so).
"""
from __future__ import annotations

import warnings

import numpy as np

_SETULB_DOC = "setulb(m,x,l,u,nbd,f,g,factr,pgtol,wa,iwa,task,lsave,isave,dsave,maxls,ln_task)"


def _setulb():
    """scipy's reverse-communication L-BFGS-B step and its message tables, or None when they are not the known ones."""
    try:
        from scipy.optimize import _lbfgsb_py as mod
        fn = mod._lbfgsb.setulb
        doc = (getattr(fn, "__doc__", "") or "").replace(" ", "")
        if _SETULB_DOC not in doc:
            return None
        return fn, mod.status_messages, mod.task_messages
    except (ImportError, AttributeError):
        return None


class _Run:
    """One problem's ``_minimize_lbfgsb`` state (scipy 1.15, unbounded, ``fmin_l_bfgs_b`` defaults)."""

    def __init__(self, x0, m):
        self.x = np.array(np.asarray(x0).ravel(), dtype=np.float64)
        n = self.x.size
        self.n = n
        self.low = np.zeros(n, np.float64)
        self.up = np.zeros(n, np.float64)
        self.nbd = np.zeros(n, np.int32)
        self.f = np.array(0.0, dtype=np.int32)
        self.g = np.zeros((n,), dtype=np.int32)
        self.wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m, np.float64)
        self.iwa = np.zeros(3 * n, dtype=np.int32)
        self.task = np.zeros(2, dtype=np.int32)
        self.ln_task = np.zeros(2, dtype=np.int32)
        self.lsave = np.zeros(4, dtype=np.int32)
        self.isave = np.zeros(44, dtype=np.int32)
        self.dsave = np.zeros(29, np.float64)
        self.nit = 0
        self.nfev = 0
        self.sf_x = None            # ScalarFunction's memo: the last point evaluated and its values
        self.sf_f = None
        self.sf_g = None
        self.done = False


def _scalar(fx):
    """ScalarFunction's check that the objective returned a true scalar."""
    if not np.isscalar(fx):
        fx = np.asarray(fx).item()
    return fx


def lockstep_fmin_l_bfgs_b(evaluate, x0s, m=10, factr=1e7, pgtol=1e-5, maxfun=15000, maxiter=15000, maxls=20):
    """``[fmin_l_bfgs_b(f_k, x0s[k], m=m, factr=factr, pgtol=pgtol, maxfun=maxfun, maxiter=maxiter, maxls=maxls)
    for k]`` with every round's evaluations batched: ``evaluate(ks, xs)`` gets the problem indices that need a value
    and their points (copies) and returns one ``(f, gradient)`` per index, in order.  Returns one ``(x, f, d)`` per
    problem, as ``fmin_l_bfgs_b`` does (``d``: grad, task, funcalls, nit, warnflag)."""
    x0s = [np.asarray(x0, dtype=np.float64) for x0 in x0s]
    k = len(x0s)
    if k == 0:
        return []
    step = _setulb()
    if step is None:
        warnings.warn("scipy's L-BFGS-B step (_lbfgsb.setulb) is not the known one: the problems are solved one after "
                      "another with fmin_l_bfgs_b", RuntimeWarning, stacklevel=2)
        return _sequential(evaluate, x0s, m, factr, pgtol, maxfun, maxiter, maxls)
    setulb, status_messages, task_messages = step
    runs = [_Run(x0, m) for x0 in x0s]
    # ScalarFunction evaluates the start point when it is built
    _evaluate_into(evaluate, runs, list(range(k)), [r.x for r in runs])
    while True:
        want, pts = [], []
        for i, r in enumerate(runs):
            if r.done:
                continue
            while True:
                r.g = r.g.astype(np.float64)
                setulb(m, r.x, r.low, r.up, r.nbd, r.f, r.g, factr, pgtol, r.wa, r.iwa, r.task, r.lsave, r.isave,
                       r.dsave, maxls, r.ln_task)
                if r.task[0] == 3:                     # f and g wanted at r.x
                    if np.array_equal(r.x, r.sf_x):
                        r.f, r.g = r.sf_f, r.sf_g
                        continue
                    want.append(i)
                    pts.append(r.x)
                    break
                if r.task[0] == 1:                     # a new iterate
                    r.nit += 1
                    if r.nit >= maxiter:
                        r.task[0] = 5
                        r.task[1] = 504
                    elif r.nfev > maxfun:
                        r.task[0] = 5
                        r.task[1] = 502
                    continue
                r.done = True
                break
        if not want:
            break
        _evaluate_into(evaluate, runs, want, pts)
        for i in want:
            r = runs[i]
            r.f, r.g = r.sf_f, r.sf_g
    out = []
    for r in runs:
        if r.task[0] == 4:
            warnflag = 0
        elif r.nfev > maxfun or r.nit >= maxiter:
            warnflag = 1
        else:
            warnflag = 2
        msg = status_messages[r.task[0]] + ": " + task_messages[r.task[1]]
        out.append((r.x, r.f, {"grad": r.g, "task": msg, "funcalls": r.nfev, "nit": r.nit, "warnflag": warnflag}))
    return out


def _evaluate_into(evaluate, runs, ks, xs):
    values = evaluate(list(ks), [np.copy(x) for x in xs])
    if len(values) != len(ks):
        raise ValueError("evaluate returned a different number of values than points")
    for i, x, (fx, gx) in zip(ks, xs, values):
        r = runs[i]
        r.sf_x = np.array(x, dtype=np.float64, copy=True)
        r.sf_f = _scalar(fx)
        r.sf_g = np.atleast_1d(gx)
        r.nfev += 1


def _sequential(evaluate, x0s, m, factr, pgtol, maxfun, maxiter, maxls):
    from scipy.optimize import fmin_l_bfgs_b
    out = []
    for i, x0 in enumerate(x0s):
        out.append(fmin_l_bfgs_b(lambda x, i=i: evaluate([i], [x])[0], x0, m=m, factr=factr, pgtol=pgtol, maxfun=maxfun,
                                 maxiter=maxiter, maxls=maxls))
    return out
