"""Support for the tests of greedy batch selection in the one-launch multi-set sweep (tests/test_sets_batch_gpu.py): the
numpy restatement of emukit's GreedyBatchPointCalculator on the oracle and the accuracy helpers -- copies of
tests/test_batch_host.believer and of tests/test_batch_gpu's truth_acq / check_values, which judge the single-set call
cbo_acq_sweep_batch by the same bar (conftest.assert_parity) -- and the pairs of (model under test, fitted twin) the
bit-for-bit comparisons run on."""
import ctypes
import warnings

import numpy as np

from conftest import assert_parity, load_fixture
from oracle import gp_oracle as O
from oracle.truth import truth_predict


def model_args(f):
    return dict(variance=float(f["variance"]), lengthscale=f["lengthscale_arg"], noise_var=float(f["noise_var"]))


def believer(f, batch_size, y_best=None, task=None, cost=None, update_incumbent=False, ei_jitter=0.0):
    """emukit's GreedyBatchPointCalculator on the oracle.  f: a golden fixture (X, y, priors, hyper-parameters, candidates).
    Returns a dict: idx (B,), val (B,), gap (B,) -- the relative distance between the best and the runner-up acquisition at
    every pick -- the data every pick was fitted on (`data`: list of (X, y, mX, vX)) and the incumbent every pick saw."""
    X, y, mX, vX = f["X"], f["y"], f["mX"], f["vX"]
    Xs, mXs, vXs = f["Xs"], f["mXs"], f["vXs"]
    y_best = float(f["y_best"]) if y_best is None else float(y_best)
    task = f["task"] if task is None else task
    cost = float(f["cost"]) if cost is None else float(cost)
    out = dict(idx=[], val=[], gap=[], data=[], y_best=[])
    for _ in range(batch_size):
        post = O.fit(X, y, mX, vX, **model_args(f))
        acq, val, idx, mean, var = O.acquisition_sweep(post, Xs, y_best, mXs, vXs, task, cost, ei_jitter)
        a = acq[:, 0]
        runner_up = np.max(np.delete(a, idx)) if a.size > 1 else -np.inf
        out["gap"].append(abs(val - runner_up) / max(abs(val), 1e-300))
        out["idx"].append(idx); out["val"].append(val); out["data"].append((X, y, mX, vX)); out["y_best"].append(y_best)
        y_new = float(mean[idx, 0])                                   # model.predict(x_new)[0]
        X = np.vstack([X, Xs[idx:idx + 1]])
        y = np.vstack([y, [[y_new]]])
        if mX is not None:
            mX = np.vstack([mX, mXs[idx:idx + 1]])
            vX = np.vstack([vX, vXs[idx:idx + 1]])
        if update_incumbent:
            y_best = min(y_best, y_new) if task == "min" else max(y_best, y_new)
    out["idx"] = np.array(out["idx"], dtype=np.int64)
    out["val"] = np.array(out["val"])
    out["gap"] = np.array(out["gap"])
    return out


def truth_acq(f, ref, t, task, cost):
    """EI / cost over the candidates from the long-double posterior of the data the restatement's pick t was fitted on."""
    X, y, mX, vX = ref["data"][t]
    mean_t, var_t, _ = truth_predict(X, y, f["Xs"], mX, vX, f["mXs"], f["vXs"], variance=float(f["variance"]),
                                     lengthscale=f["lengthscale_arg"], noise_var=float(f["noise_var"]),
                                     diag_add=float(f["noise_var"]) + 1e-8)
    return O.expected_improvement(mean_t, var_t, ref["y_best"][t], task) / cost


def check_values(f, ref, vals, task, cost):
    """best_vals[t] under the parity rule, every pick against the long-double acquisition of its own data."""
    for t in range(len(vals)):
        p = int(ref["idx"][t])
        assert_parity(vals[t], ref["val"][t], truth_acq(f, ref, t, task, cost)[p, 0], f"best_vals[{t}]")


def gp(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def fixture_model(name, fit):
    """(model, grid, fixture) of a golden fixture; a causal fixture's prior closures look their rows up."""
    from cbo_with_oop_amd import CandidateGrid
    f = load_fixture(name)
    ls = f["lengthscale_arg"]
    kw = {}
    if f["mX"] is not None:
        tables = {"m": np.vstack([f["mX"], f["mXs"]]), "v": np.vstack([f["vX"], f["vXs"]])}
        pts = np.vstack([f["X"], f["Xs"]])

        def lookup(which):
            def fn(a):
                a = np.atleast_2d(a)
                rows = [int(np.flatnonzero(np.all(pts == r[None, :], axis=1))[0]) for r in a]
                return tables[which][rows]
            return fn
        kw = dict(mean_function=lookup("m"), variance_adjustment=lookup("v"))
    g = gp(f["X"], f["y"], fit=fit, variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls),
           noise_var=float(f["noise_var"]), **kw)
    return g, CandidateGrid(f["Xs"], g), f


def mean_f(a):
    return 0.3 * np.sin(a).sum(1, keepdims=True)


def var_f(a):
    return 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2


class Pair:
    """One exploration set twice: the model under test (not fitted unless `fit`) with its grid, and the fitted twin with
    its own."""

    def __init__(self, n, m, d, causal=False, ard=False, offset=0, seed=0, dtype="f64", fit=False):
        from cbo_with_oop_amd import CandidateGrid
        rng = np.random.default_rng(1000 * n + 10 * m + d + seed)
        X = rng.uniform(-2.0, 2.0, (n, d))
        y = np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))
        pts = rng.uniform(-2.5, 2.5, (m, d))
        kw = dict(variance=1.3, lengthscale=(0.7 + 0.2 * np.arange(d)) if ard else 0.9, ard=ard, noise_var=1e-3, dtype=dtype)
        if causal:
            kw.update(mean_function=mean_f, variance_adjustment=var_f)
        self.n, self.m, self.dtype = n, m, dtype
        self.model, self.twin = gp(X, y, fit=fit, **kw), gp(X, y, **kw)
        self.grid = CandidateGrid(pts, self.model, index_offset=offset)
        self.twin_grid = CandidateGrid(pts, self.twin, index_offset=offset)

    def close(self):
        for o in (self.grid, self.twin_grid, self.model, self.twin):
            o.close()


def handles(objs):
    return (ctypes.c_void_p * len(objs))(*[o._handle for o in objs])


def sets_batch(lib, models, grids, y_best, task, B, costs, update=0, jitter=0.0):
    """cbo_acq_sweep_sets_batch: (rc, values (S, B), indices (S, B))."""
    s = len(models)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)))
    cs = np.ascontiguousarray(np.broadcast_to(np.asarray(costs, dtype=np.float64), (s,)))
    vals, idxs = np.full(s * B, -7.0), np.full(s * B, -7, dtype=np.int64)
    rc = lib.load().cbo_acq_sweep_sets_batch(s, handles(models), handles(grids), lib.dptr(yb), lib.TASK_CODE.get(task, task),
                                             float(jitter), lib.dptr(cs), int(B), int(update), lib.dptr(vals),
                                             idxs.ctypes.data_as(lib.c_int64_p))
    return rc, vals.reshape(s, B), idxs.reshape(s, B)


def per_set_batch(lib, twins, twin_grids, y_best, task, B, costs, update=0, jitter=0.0):
    """The reference: cbo_acq_sweep_batch set by set on fitted twins."""
    s = len(twins)
    yb, cs = np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)), np.broadcast_to(np.asarray(costs, float), (s,))
    vals, idxs = np.empty((s, B)), np.empty((s, B), dtype=np.int64)
    for i, (g, grid) in enumerate(zip(twins, twin_grids)):
        g.ensure_fitted()
        v, ix = np.empty(B), np.empty(B, dtype=np.int64)
        lib.check(lib.load().cbo_acq_sweep_batch(g._handle, grid._handle, float(yb[i]), lib.TASK_CODE[task], float(jitter),
                                                 float(cs[i]), int(B), int(update), lib.dptr(v),
                                                 ix.ctypes.data_as(lib.c_int64_p), None, None, None))
        vals[i], idxs[i] = v, ix
    return vals, idxs


def assert_same(got, want, what=""):
    (gv, gi), (wv, wi) = got, want
    print(what, "indices", gi.tolist(), "reference", wi.tolist())
    print(what, "values", gv.tolist(), "reference", wv.tolist())
    assert np.array_equal(gi, wi), (what, gi, wi)
    assert np.array_equal(np.ascontiguousarray(gv).view(np.uint64), np.ascontiguousarray(wv).view(np.uint64)), (what, gv, wv)


def check_call(lib, pairs, y_best, task, B, costs, update=0, jitter=0.0, what=""):
    rc, vals, idxs = sets_batch(lib, [p.model for p in pairs], [p.grid for p in pairs], y_best, task, B, costs, update, jitter)
    lib.check(rc)
    want = per_set_batch(lib, [p.twin for p in pairs], [p.twin_grid for p in pairs], y_best, task, B, costs, update, jitter)
    assert_same((vals, idxs), want, what)
    return vals, idxs
