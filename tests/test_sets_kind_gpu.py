"""GPU tests of the point-wise acquisitions in the one-launch multi-set sweep and the agent:
cbo_acq_sweep_sets_kind / cbo_trial_step_kind (small_sets_kernel<KIND>, kernels_sets.hip) and the Python layer on top.

Every comparison is exact -- values as bit patterns (NaN equals NaN), indices equal -- and the reference is always the
per-set cbo_acq_sweep_kind (for the plug-in EI also cbo_acq_sweep at cbo_gp_plugin_incumbent) on freshly FITTED twin models,
never the code under test.  Equality is the contract, not a hope: the launch runs kernel_value, the decoupled-wave block
factorisation, the tile solve, posterior_of and pointwise_of / acquisition_of -- the general path's own device functions in
the general path's summation orders -- and the plug-in incumbent goes through plugin_incumbent_kernel's reduction operation
for operation."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu

INVALID, NOT_FITTED = -1, -5
LCB, PI, VAR, MPEI = 1, 2, 3, 4
KINDS = {"LCB": (LCB, 1.5), "PI": (PI, 0.01), "VAR": (VAR, 0.0), "MPEI": (MPEI, 0.01)}


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def gp(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def mean_f(a):
    return 0.3 * np.sin(a).sum(1, keepdims=True)


def var_f(a):
    return 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2


class Pair:
    """One exploration set twice: the model under test (never fitted) with its grid, and the fitted twin with its own."""

    def __init__(self, n, m, d, causal=False, ard=False, offset=0, seed=0, shift=0.0, kw=None, data=None, cand=None):
        from cbo_with_oop_amd import CandidateGrid
        rng = np.random.default_rng(1000 * n + 10 * m + d + seed)
        X = rng.uniform(-2.0, 2.0, (n, d)) if data is None else data[0]
        y = shift + np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1)) if data is None else data[1]
        pts = rng.uniform(-2.5, 2.5, (m, d)) if cand is None else cand
        if kw is None:
            kw = dict(variance=1.3, lengthscale=(0.7 + 0.2 * np.arange(d)) if ard else 0.9, ard=ard, noise_var=1e-3)
            if causal:
                kw.update(mean_function=mean_f, variance_adjustment=var_f)
        self.model, self.twin = gp(X, y, fit=False, **kw), gp(X, y, **kw)
        self.grid = CandidateGrid(pts, self.model, index_offset=offset)
        self.twin_grid = CandidateGrid(pts, self.twin, index_offset=offset)

    def close(self):
        for o in (self.grid, self.twin_grid, self.model, self.twin):
            o.close()


def handles(objs):
    return (ctypes.c_void_p * len(objs))(*[o._handle for o in objs])


def sweep_sets_kind(lib, models, grids, kind, y_best, task, param, costs):
    """cbo_acq_sweep_sets_kind: (rc, values, indices)."""
    s = len(models)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)))
    cs = np.ascontiguousarray(np.broadcast_to(np.asarray(costs, dtype=np.float64), (s,)))
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    rc = lib.load().cbo_acq_sweep_sets_kind(s, handles(models), handles(grids), int(kind), lib.dptr(yb),
                                            lib.TASK_CODE.get(task, task), float(param), lib.dptr(cs), lib.dptr(vals),
                                            idxs.ctypes.data_as(lib.c_int64_p))
    return rc, vals, idxs


def per_set(lib, twins, twin_grids, kind, y_best, task, param, costs):
    """The reference: cbo_acq_sweep_kind set by set on fitted twins."""
    s = len(twins)
    yb, cs = np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)), np.broadcast_to(np.asarray(costs, float), (s,))
    vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
    for i, (g, grid) in enumerate(zip(twins, twin_grids)):
        g.ensure_fitted()
        bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
        lib.check(lib.load().cbo_acq_sweep_kind(g._handle, grid._handle, int(kind), float(yb[i]), lib.TASK_CODE[task],
                                                float(param), float(cs[i]), None, None, None, ctypes.byref(bv),
                                                ctypes.byref(bi)))
        vals[i], idxs[i] = bv.value, bi.value
    return vals, idxs


def assert_same(got, want, what=""):
    (gv, gi), (wv, wi) = got, want
    print(what, "values", gv.tolist(), "reference", wv.tolist(), "indices", gi.tolist(), "reference", wi.tolist())
    assert np.array_equal(gi, wi), (what, gi, wi)
    assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)), (what, gv, wv)


def check_call(lib, pairs, kind, y_best, task, param, costs, what=""):
    models, grids = [p.model for p in pairs], [p.grid for p in pairs]
    rc, vals, idxs = sweep_sets_kind(lib, models, grids, kind, y_best, task, param, costs)
    lib.check(rc)
    want = per_set(lib, [p.twin for p in pairs], [p.twin_grid for p in pairs], kind, y_best, task, param, costs)
    assert_same((vals, idxs), want, what)
    return vals, idxs


# ---- the kernel's edges ----------------------------------------------------------------------------------------------------
# n: 16-row tile boundaries and the largest model the launch takes; m: 64 candidates per workgroup; 704 / 705 candidates: 11
# and 12 workgroups per set, the two sides of the one- / two-launch split (the widest set of a call decides for the call)
ONE_LAUNCH = [dict(n=1, m=1, d=1), dict(n=15, m=63, d=2, causal=True), dict(n=16, m=64, d=3, offset=5000),
              dict(n=17, m=65, d=8, ard=True), dict(n=50, m=200, d=1, causal=True), dict(n=128, m=704, d=2)]
TWO_LAUNCHES = [dict(n=128, m=705, d=3, causal=True), dict(n=17, m=1, d=1), dict(n=50, m=200, d=2, ard=True, offset=77),
                dict(n=16, m=65, d=8, causal=True)]


@pytest.fixture(scope="module")
def zoo(lib):
    groups = {"one launch": [Pair(**kw) for kw in ONE_LAUNCH], "two launches": [Pair(**kw) for kw in TWO_LAUNCHES]}
    yield groups
    for pairs in groups.values():
        for p in pairs:
            p.close()


@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("name", list(KINDS))
def test_shapes(lib, zoo, name, task):
    kind, param = KINDS[name]
    for what, pairs in zoo.items():
        s = len(pairs)
        y_best = np.linspace(-0.4, 0.6, s)                    # (inside the targets' range: PI neither 0 nor 1 everywhere)
        costs = 1.0 + np.arange(s) % 3
        check_call(lib, pairs, kind, y_best, task, param, costs, f"{name} {task} {what}")
        # the launch needs no fit and leaves the models alone
        assert all(p.model.stale for p in pairs)
        out = np.empty(1)
        assert all(lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == NOT_FITTED for p in pairs), "a model was fitted"


# ---- the plug-in EI ----------------------------------------------------------------------------------------------------------
def plain_sweep(lib, g, grid, y_best, task, jitter, cost):
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                       float(cost), None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
    return bv.value, bi.value


def incumbent(lib, g, task):
    out = ctypes.c_double()
    lib.check(lib.load().cbo_gp_plugin_incumbent(g._handle, lib.TASK_CODE[task], ctypes.byref(out)))
    return out.value


@pytest.mark.parametrize("task", ["min", "max"])
def test_mpei_is_the_ei_at_the_plugin_incumbent(lib, zoo, task):
    for what, pairs in zoo.items():
        s = len(pairs)
        costs = 1.0 + np.arange(s) % 3
        # y_best is not read: garbage must not matter
        rc, vals, idxs = sweep_sets_kind(lib, [p.model for p in pairs], [p.grid for p in pairs], MPEI, np.nan, task, 0.01, costs)
        lib.check(rc)
        want_v, want_i = np.empty(s), np.empty(s, dtype=np.int64)
        for i, p in enumerate(pairs):
            inc = incumbent(lib, p.twin, task)
            assert np.isfinite(inc)
            want_v[i], want_i[i] = plain_sweep(lib, p.twin, p.twin_grid, inc, task, 0.01, costs[i])
        assert_same((vals, idxs), (want_v, want_i), f"MPEI {task} {what}")


def test_mpei_nan_prior_mean_at_a_training_point(lib):
    """A NaN prior mean at one training point: the incumbent is NaN (np.min / np.max), and the result cbo_acq_sweep's for
    y_best = NaN -- in the one launch and in the two."""
    for n, m in ((40, 150), (70, 800)):
        rng = np.random.default_rng(n)
        X = rng.uniform(-2.0, 2.0, (n, 2))
        y = np.cos(X).sum(1, keepdims=True)
        bad = X[5].copy()

        def mf(a):
            out = mean_f(a)
            out[np.all(a == bad[None, :], axis=1)] = np.nan
            return out
        kw = dict(variance=1.3, lengthscale=0.9, noise_var=1e-4, mean_function=mf, variance_adjustment=var_f)
        healthy = Pair(30, 100, 2, causal=True)
        pair = Pair(n, m, 2, kw=kw, data=(X, y))
        for task in ("min", "max"):
            assert np.isnan(incumbent(lib, pair.twin, task))
            rc, vals, idxs = sweep_sets_kind(lib, [healthy.model, pair.model], [healthy.grid, pair.grid], MPEI, 0.0, task, 0.0,
                                             [1.0, 2.0])
            lib.check(rc)
            want = [plain_sweep(lib, healthy.twin, healthy.twin_grid, incumbent(lib, healthy.twin, task), task, 0.0, 1.0),
                    plain_sweep(lib, pair.twin, pair.twin_grid, np.nan, task, 0.0, 2.0)]
            assert_same((vals, idxs), (np.array([w[0] for w in want]), np.array([w[1] for w in want], dtype=np.int64)),
                        f"NaN prior mean {task} n={n} m={m}")
        healthy.close(); pair.close()


# ---- a negative bound over a cost ----------------------------------------------------------------------------------------------
def test_lcb_negative_bound_is_divided_by_the_cost_all_the_same(lib):
    """Means well above zero with task 'min': -(mean - beta sd) is negative, and divided by the cost all the same."""
    # (candidates inside the cloud of observations: the posterior mean stays near the targets' level of 6)
    pairs = [Pair(60, 200, 2, shift=6.0, seed=s, cand=np.random.default_rng(s).uniform(-1.5, 1.5, (200, 2))) for s in range(3)]
    costs = [1.0, 10.0, 3.0]
    vals, _ = check_call(lib, pairs, LCB, 0.0, "min", 1.0, costs, "negative LCB")
    assert np.all(vals < 0.0)
    for p in pairs:
        p.close()


# ---- 25 sets: the descriptors are read from the pinned array ---------------------------------------------------------------------
def test_twenty_five_sets(lib):
    pairs = []
    for sidx in range(25):
        d = 1 + sidx % 3
        pairs.append(Pair(8 + (7 * sidx) % 60, [150, 221, 210][d - 1] + sidx, d, causal=sidx % 4 == 1, seed=sidx))
    costs = [1.0 + s % 3 for s in range(25)]
    for name, (kind, param) in KINDS.items():
        check_call(lib, pairs, kind, 0.1, "min", param, costs, f"25 sets {name}")
    for p in pairs:
        p.close()


# ---- mixed routing ------------------------------------------------------------------------------------------------------------------
def fixture_kwargs(f):
    ls = f["lengthscale_arg"]
    kw = dict(variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls), noise_var=float(f["noise_var"]))
    if f["mX"] is not None:
        lut_m = {**{tuple(r): v for r, v in zip(map(tuple, f["X"]), f["mX"][:, 0])},
                 **{tuple(r): v for r, v in zip(map(tuple, f["Xs"]), f["mXs"][:, 0])}}
        lut_v = {**{tuple(r): v for r, v in zip(map(tuple, f["X"]), f["vX"][:, 0])},
                 **{tuple(r): v for r, v in zip(map(tuple, f["Xs"]), f["vXs"][:, 0])}}
        kw["mean_function"] = lambda a: np.array([[lut_m[tuple(r)]] for r in a])
        kw["variance_adjustment"] = lambda a: np.array([[lut_v[tuple(r)]] for r in a])
    return kw


def mixed_pairs():
    """A small causal model; a small model with duplicate rows (its factorisation needs jitchol's jitter: the general path
    takes over for that set); a 200-row model; an fp32 model."""
    fc, fj = load_fixture("causal_d2"), load_fixture("jitter_ladder")
    rng = np.random.default_rng(3)
    Xb = rng.uniform(-3, 3, (200, 3))
    yb = np.cos(Xb).sum(1, keepdims=True)
    cand = rng.uniform(-3, 3, (300, 3))
    return [Pair(len(fc["X"]), len(fc["Xs"]), 2, kw=fixture_kwargs(fc), data=(fc["X"], fc["y"]), cand=fc["Xs"]),
            Pair(len(fj["X"]), len(fj["Xs"]), 0, kw=fixture_kwargs(fj), data=(fj["X"], fj["y"]), cand=fj["Xs"]),
            Pair(200, 300, 3, kw=dict(noise_var=1e-3), data=(Xb, yb), cand=cand),
            Pair(200, 300, 3, kw=dict(noise_var=1e-2, dtype="f32"), data=(Xb, yb), cand=cand)]


def mixed_answers(lib, pairs):
    out = []
    for name, (kind, param) in KINDS.items():
        rc, vals, idxs = sweep_sets_kind(lib, [p.model for p in pairs], [p.grid for p in pairs], kind, 0.1, "min", param,
                                         [2.0, 1.0, 3.0, 3.0])
        lib.check(rc)
        out.append((name, vals, idxs))
    return out


def child_mixed():
    """(the child process of test_mixed_routing: the answers of the code under test, one line per kind)"""
    from cbo_with_oop_amd import _lib
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        pairs = [p for p in mixed_pairs()]
        for name, vals, idxs in mixed_answers(_lib, pairs):
            print("ANSWER", name, vals.view(np.uint64).tolist(), idxs.tolist())


def test_mixed_routing(lib):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        pairs = mixed_pairs()
        got = mixed_answers(lib, pairs)
        for (name, vals, idxs), (kind, param) in zip(got, KINDS.values()):
            want = per_set(lib, [p.twin for p in pairs], [p.twin_grid for p in pairs], kind, 0.1, "min", param,
                           [2.0, 1.0, 3.0, 3.0])
            assert_same((vals, idxs), want, f"mixed {name}")
    assert pairs[1].twin.jitter_tries >= 1                                         # that set did need the ladder
    # the same call with the one launch switched off (read when the context is created: a process of its own)
    env = dict(os.environ, CBO_HIP_SMALL_SETS="0")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_sets_kind_gpu as t; t.child_mixed()"
            % (ROOT, os.path.join(ROOT, "tests")))
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln.split(" ", 2) for ln in run.stdout.splitlines() if ln.startswith("ANSWER ")]
    assert [ln[1] for ln in lines] == [name for name, _, _ in got]
    for (_, name, rest), (_, vals, idxs) in zip(lines, got):
        assert rest == f"{vals.view(np.uint64).tolist()} {idxs.tolist()}", (name, rest)
    for p in pairs:
        p.close()


# ---- the trial step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal,ard,cand_sizes", [(True, False, [200, 800, 300]), (False, True, [200, 130, 300])])
def test_trial_step_kind_is_the_three_calls(lib, causal, ard, cand_sizes):
    """cbo_trial_step_kind against cbo_gp_upload_data + cbo_acq_sweep_sets_kind + cbo_argmax_sets on twin models, for every
    kind, d = 3, over a trajectory on which the staged set grows 63 -> 66 observations (across a tile boundary); with prior
    closures (the plug-in incumbent then reads them from the staging buffer) and 800 candidates (the two-launch form, where
    it reads the resident copies the first launch wrote), and with per-dimension lengthscales."""
    from cbo_with_oop_amd import CandidateGrid
    L = lib.load()
    rng = np.random.default_rng(17)
    d, sizes = 3, [40, 63, 100]
    kw = dict(variance=1.4, lengthscale=np.array([0.8, 1.7, 1.2]) if ard else 1.3, ard=ard, noise_var=1e-3)
    if causal:
        kw.update(mean_function=mean_f, variance_adjustment=var_f)
    f = lambda x: np.sin(x).sum(1, keepdims=True) + 0.05 * rng.standard_normal((x.shape[0], 1))      # noqa: E731
    data = [rng.uniform(-3, 3, (n, d)) for n in sizes]
    obs = [f(x) for x in data]
    cand = [rng.uniform(-3, 3, (m, d)) for m in cand_sizes]

    def build():
        models = [gp(x, y, fit=False, **kw) for x, y in zip(data, obs)]
        return models, [CandidateGrid(c, m) for c, m in zip(cand, models)]
    one, one_grids = build()
    three, three_grids = build()
    S = len(sizes)
    y_best = np.array([-2.6, -2.4, -2.5])                     # (near the targets' minimum: PI is no step function)
    costs = np.array([1.0, 2.0, 3.0])
    for trial in range(3):
        x_new = rng.uniform(-3, 3, (1, d))
        data[1] = np.vstack([data[1], x_new]); obs[1] = np.vstack([obs[1], f(x_new)])
        for name, (kind, param) in KINDS.items():
            results = []
            for models, grids, fused in ((one, one_grids, True), (three, three_grids, False)):
                m = models[1]
                m._set_arrays(data[1], obs[1])
                pm, pv = m._prior(m.X)
                vals, idxs, chosen = np.empty(S), np.empty(S, dtype=np.int64), ctypes.c_int(-1)
                if fused:
                    lib.check(L.cbo_trial_step_kind(S, handles(models), handles(grids), 1, m.X.shape[0], lib.dptr(m.X),
                                                    lib.dptr(m._y_flat), lib.dptr(pm), lib.dptr(pv), kind, lib.dptr(y_best), 0,
                                                    param, lib.dptr(costs), lib.dptr(vals), idxs.ctypes.data_as(lib.c_int64_p),
                                                    ctypes.byref(chosen)))
                else:
                    lib.check(L.cbo_gp_upload_data(m._handle, m.X.shape[0], lib.dptr(m.X), lib.dptr(m._y_flat), lib.dptr(pm),
                                                   lib.dptr(pv)))
                    lib.check(L.cbo_acq_sweep_sets_kind(S, handles(models), handles(grids), kind, lib.dptr(y_best), 0, param,
                                                        lib.dptr(costs), lib.dptr(vals), idxs.ctypes.data_as(lib.c_int64_p)))
                    lib.check(L.cbo_argmax_sets(lib.dptr(vals), S, ctypes.byref(chosen)))
                m.stale = True
                results.append((vals, idxs, chosen.value))
            assert_same(results[0][:2], results[1][:2], f"trial {trial} {name}")
            assert results[0][2] == results[1][2]
            assert L.cbo_gp_n(one[1]._handle) == data[1].shape[0]
    assert data[1].shape[0] == 66
    # and against the per-set call on fresh twins, once, at the end of the trajectory
    twins = [gp(x, y, **kw) for x, y in zip(data, obs)]
    twin_grids = [CandidateGrid(c, m) for c, m in zip(cand, twins)]
    for name, (kind, param) in KINDS.items():
        rc, vals, idxs = sweep_sets_kind(lib, one, one_grids, kind, y_best, "min", param, costs)
        lib.check(rc)
        assert_same((vals, idxs), per_set(lib, twins, twin_grids, kind, y_best, "min", param, costs), f"after the steps {name}")
    for o in one_grids + three_grids + twin_grids + one + three + twins:
        o.close()


# ---- the Python path ----------------------------------------------------------------------------------------------------------------
def per_set_point(model, space, best, evaluated_set, cost_table, task, beta):
    """find_next_y_point(acquisition="LCB") on the grid, line for line (utils.py), with the bound's beta given: the grid's
    winner at the batch cost, re-evaluated at the point's own cost where that differs."""
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import CausalNegativeLowerConfidenceBound, Cost
    cost = Cost(cost_table, evaluated_set)
    acq = CausalNegativeLowerConfidenceBound(task, model, beta=beta)
    grid = CandidateGrid(meshgrid_candidates(space, [200]), model)
    batch_cost = float(cost.evaluate(grid.points))
    res = acq.sweep(grid, cost=batch_cost)
    x_new = grid.points[res["best_idx"] - grid.index_offset][None, :].copy()
    point_cost = float(cost.evaluate(x_new))
    y = np.array([[res["best_val"]]]) if point_cost == batch_cost else acq.sweep(x_new, cost=point_cost, want_acq=True)["acq"]
    grid.close()
    return y, x_new


@pytest.mark.parametrize("beta", [None, 2.0])
def test_path_trial_step_with_a_lower_confidence_bound(lib, beta):
    """CBOAcquisitionPath(acquisition="LCB", acquisition_param=beta).trial_step over several trials on the toy graph returns
    what find_next_y_point(acquisition="LCB") per set plus select_next_intervention return (beta None: the default bound,
    find_next_y_point itself; beta 2: its lines with the bound's beta given, per_set_point); the cost table is variable
    (1 + |x|), so every winner is re-evaluated at its own cost (winners_to_points)."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory as GPFactory
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import find_next_y_point
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    cost_table = ToyGraph.get_cost_structure(4)
    rng = np.random.default_rng(4)
    xs = [rng.uniform(-5, 5, (12, 1)), rng.uniform(-5, 20, (12, 1))]
    ys = [targets[0](xs[0]), targets[1](xs[1])]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, cost_table, "min", xs, ys,
                              [ToyGraph.bounds(s) for s in es], grid_shapes=[[200], [200]], comm=None, acquisition="LCB",
                              acquisition_param=beta)
    path.update_all_gaussian_processes()
    kind = ("LCB", 1.0 if beta is None else beta)
    calls = []
    for trial in range(4):
        best = min(float(ys[0].min()), float(ys[1].min()))
        a_x, a_y, (a_set, a_idx) = path.trial_step(best)
        b_x, b_y = [], []
        for s in range(2):
            twin = GPFactory.create(GaussianProcessType.NON_CAUSAL_GP, xs[s], ys[s], [None, None], emukit_wrapper=True)
            if beta is None:
                y, x = find_next_y_point(ToyGraph.bounds(es[s]), twin, best, es[s], cost_table, task="min", grid_shape=[200],
                                         acquisition="LCB")
            else:
                y, x = per_set_point(twin, ToyGraph.bounds(es[s]), best, es[s], cost_table, "min", beta)
            b_x.append(x); b_y.append(y)
            twin.close()
        b_idx = int(np.argmax([float(y[0, 0]) for y in b_y]))
        print("trial", trial, [y.tolist() for y in a_y], [y.tolist() for y in b_y])
        assert a_idx == b_idx and a_set == es[b_idx]
        assert all(np.array_equal(p, q) for p, q in zip(a_x, b_x))
        assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(a_y, b_y))
        # the winners were re-evaluated: no set's point cost is its batch cost
        st = path._call_cache["sweep_sets"]
        assert st["kind"] == kind
        assert all(float(st["costs"][s].evaluate(a_x[s])) != st["batch_cost"][s] for s in range(2))
        calls.append("trial_args" in st)
        xs[a_idx] = np.vstack([xs[a_idx], a_x[a_idx]])
        ys[a_idx] = np.vstack([ys[a_idx], targets[a_idx](a_x[a_idx])])
    # from the second trial on the one-call form (cbo_trial_step_kind) was taken
    assert calls == [False, True, True, True]
    assert path._call_cache["sweep_sets"]["trial_args"][0] == kind


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_models_untouched(lib):
    L = lib.load()
    pairs = [Pair(20, 100, 2, causal=True), Pair(33, 70, 2)]
    models, grids = [p.model for p in pairs], [p.grid for p in pairs]

    def untouched():
        out = np.empty(1)
        return (all(m.stale for m in models) and [L.cbo_gp_n(m._handle) for m in models] == [20, 33]
                and all(L.cbo_gp_log_marginal(m._handle, lib.dptr(out)) == NOT_FITTED for m in models))

    def refused(kind, y_best=0.1, task="min", param=0.5, costs=(1.0, 2.0)):
        rc, vals, idxs = sweep_sets_kind(lib, models, grids, kind, y_best, task, param, costs)
        assert rc == INVALID and L.cbo_last_error(), (kind, y_best, task, param, costs)
        assert np.all(vals == -7.0) and np.all(idxs == -7) and untouched()
        x = pairs[1].model.X
        bigger = np.vstack([x, x[:1] + 0.5])
        vals, idxs, chosen = np.empty(2), np.empty(2, dtype=np.int64), ctypes.c_int(-1)
        yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (2,)))
        cs = np.ascontiguousarray(np.broadcast_to(np.asarray(costs, dtype=np.float64), (2,)))
        rc = L.cbo_trial_step_kind(2, handles(models), handles(grids), 1, bigger.shape[0], lib.dptr(bigger),
                                   lib.dptr(np.zeros(bigger.shape[0])), None, None, int(kind), lib.dptr(yb),
                                   lib.TASK_CODE.get(task, task), float(param), lib.dptr(cs), lib.dptr(vals),
                                   idxs.ctypes.data_as(lib.c_int64_p), ctypes.byref(chosen))
        assert rc == INVALID and untouched() and chosen.value == -1

    for kind in (0, 5, -1):
        refused(kind)
    for kind in (LCB, PI, MPEI):
        for param in (np.nan, np.inf, -np.inf):
            refused(kind, param=param)
        for task in (2, -1):
            refused(kind, task=task)
    refused(LCB, param=-1e-300)
    for y_best in (np.nan, np.inf, [0.1, np.nan]):
        refused(PI, y_best=y_best)
    for kind in (LCB, PI, VAR, MPEI):
        for costs in ((0.0, 1.0), (1.0, -1.0), (1.0, np.nan)):
            refused(kind, costs=costs)
    # cbo_acq_sweep_sets' own checks
    vals, idxs = np.empty(2), np.empty(2, dtype=np.int64)
    yb, cs = np.full(2, 0.1), np.ones(2)
    ok = (2, handles(models), handles(grids), LCB, lib.dptr(yb), 0, 1.0, lib.dptr(cs), lib.dptr(vals),
          idxs.ctypes.data_as(lib.c_int64_p))
    for at, bad in ((0, 0), (1, None), (2, None), (4, None), (7, None), (8, None), (9, None)):
        args = list(ok)
        args[at] = bad
        assert L.cbo_acq_sweep_sets_kind(*args) == INVALID and untouched(), at
    # what the model variance does not read is not checked; the refusals left the valid calls working
    for kind, y_best, task, param in ((VAR, np.nan, 7, np.nan), (MPEI, np.nan, "max", 0.0), (LCB, np.inf, "min", 0.0)):
        rc, vals, idxs = sweep_sets_kind(lib, models, grids, kind, y_best, task, param, (1.0, 2.0))
        assert rc == 0
        want = per_set(lib, [p.twin for p in pairs], [p.twin_grid for p in pairs], kind, 0.0, "min" if kind == VAR else task,
                       0.0, (1.0, 2.0))
        assert_same((vals, idxs), want, f"valid call {kind}")
    for p in pairs:
        p.close()
