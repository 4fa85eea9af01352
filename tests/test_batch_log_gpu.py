"""GPU tests of greedy batch selection in log space: cbo_acq_sweep_batch_logei (the believer's kernels of
kernels_batch.hip behind the log-EI candidate pass), cbo_acq_sweep_sets_batch_logei (small_sets_batch_kernel's log
instantiation) and the Python layer on top.

What is exact is compared as bit patterns: pick 0 and a batch of one against cbo_acq_sweep_logei, a batch against the longer
batch it is a prefix of, the one launch against the per-set call on freshly fitted twins.  The formula is judged as
tests/test_logei_gpu.py judges the single pick -- mpmath at 60 digits from the mean and variance doubles the call returned,
within its ACCURACY_BOUND (6.9e-15 max(1, |ref|)): the pass is the same arithmetic on another q -- and the posterior as
tests/test_batch_gpu.py judges the EI form's (conftest.assert_parity against the long-double refit).  The picks are compared
with the numpy restatement test_batch_log_host.log_believer where its best and runner-up are more than 1e-6 apart in log
value."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import assert_parity
from oracle import gp_oracle as O
from oracle.truth import truth_predict
from sets_batch_support import Pair, assert_same, gp, handles
from test_batch_gpu import CASES, HYPER, batch, fixture_case, make_case, same_bits
from test_batch_log_host import dead_region_problem, log_believer
from test_logei_gpu import ACCURACY_BOUND, mp_log_ei, scaled_error

pytestmark = pytest.mark.gpu

NOT_FITTED = -5


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def batch_log(lib, g, grid, y_best, task, B, cost=1.0, jitter=0.0, update=0, want=True):
    """cbo_acq_sweep_batch_logei: (best_vals, best_idxs, acq, mean, var)."""
    m = len(grid)
    acq, mean, var = (np.empty(m), np.empty(m), np.empty(m)) if want else (None, None, None)
    bv, bi = np.full(B, np.nan), np.full(B, -1, dtype=np.int64)
    lib.check(lib.load().cbo_acq_sweep_batch_logei(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                                   float(cost), B, update, lib.dptr(bv), bi.ctypes.data_as(lib.c_int64_p),
                                                   lib.dptr(acq), lib.dptr(mean), lib.dptr(var)))
    return bv, bi, acq, mean, var


def single_log(lib, g, grid, y_best, task, cost=1.0, jitter=0.0):
    """cbo_acq_sweep_logei: (acq, mean, var, best_val, best_idx)."""
    m = len(grid)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep_logei(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                             float(cost), lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                             ctypes.byref(bi)))
    return acq, mean, var, bv.value, bi.value


# ---- pick 0 and a batch of one -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,d,B,causal,task,offset", CASES)
def test_pick_0_and_a_batch_of_one_are_the_log_ei_sweeps_bits(lib, n, m, d, B, causal, task, offset):
    g, grid, data = make_case(n, m, d, causal, offset=offset)
    y_best = float(data["y"].min() if task == "min" else data["y"].max())
    acq, mean, var, bv, bi = single_log(lib, g, grid, y_best, task, cost=2.0, jitter=0.01)
    vals, idxs, acq1, mean1, var1 = batch_log(lib, g, grid, y_best, task, 1, cost=2.0, jitter=0.01)
    assert same_bits(vals[0], bv) and idxs[0] == bi
    assert same_bits(acq1, acq) and same_bits(mean1, mean) and same_bits(var1, var)
    for update in (0, 1):
        vals, idxs, _, mean_b, _ = batch_log(lib, g, grid, y_best, task, B, cost=2.0, jitter=0.01, update=update)
        assert same_bits(vals[0], bv) and idxs[0] == bi
        assert same_bits(mean_b, mean)                             # the believed residual is zero: mu never moves
        assert np.all((idxs >= offset) & (idxs < offset + m)) and np.all(np.isfinite(vals))
    grid.close()


# ---- prefix, formula ---------------------------------------------------------------------------------------------------------
PREFIX_CASES = {"n17 m257 d3 ard": dict(n=17, m=257, d=3, ard=True), "n300 m257 d1 causal": dict(n=300, m=257, d=1, causal=True)}


@pytest.fixture(scope="module")
def prefix_pairs(lib):
    pairs = {name: Pair(fit=True, **kw) for name, kw in PREFIX_CASES.items()}
    yield pairs
    for p in pairs.values():
        p.close()


@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("name", list(PREFIX_CASES))
def test_a_batch_is_the_prefix_of_a_longer_one(lib, prefix_pairs, name, update):
    p = prefix_pairs[name]
    B = 3
    for task, y_best in (("min", 0.1), ("max", 0.4)):
        short = batch_log(lib, p.model, p.grid, y_best, task, B, cost=0.5, update=update)
        long = batch_log(lib, p.model, p.grid, y_best, task, B + 3, cost=0.5, update=update)
        print(name, task, update, long[1].tolist(), long[0].tolist())
        assert np.array_equal(short[1], long[1][:B]) and same_bits(short[0], long[0][:B])
        again = batch_log(lib, p.model, p.grid, y_best, task, B + 3, cost=0.5, update=update)
        assert all(same_bits(a, b) for a, b in zip(long, again))   # two identical calls: the same bits


@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("name", list(PREFIX_CASES))
def test_the_last_picks_values_against_mpmath(lib, prefix_pairs, name, task, update):
    """acq_out of the last pick from the returned mean_out / var_out doubles and the cost.  With update_incumbent the
    incumbent of the last pick is the given one moved by the means at the earlier picks (the means never change)."""
    p = prefix_pairs[name]
    B, cost, jitter = 4, 2.0, 0.01
    # incumbents that the believed means do reach, so that update_incumbent moves them
    y_best = 1.5 if task == "min" else -1.5
    vals, idxs, acq, mean, var = batch_log(lib, p.model, p.grid, y_best, task, B, cost=cost, jitter=jitter, update=update)
    seen = y_best
    if update:
        earlier = mean[idxs[:B - 1] - p.grid.index_offset]
        seen = min(y_best, earlier.min()) if task == "min" else max(y_best, earlier.max())
        assert seen != y_best, "the case does not move the incumbent"
    err = scaled_error(acq, mp_log_ei(mean, var, seen, task, jitter, cost))
    print(name, task, update, "worst scaled error", err.max(), "bound", ACCURACY_BOUND)
    assert err.max() <= ACCURACY_BOUND, err.max()
    last = int(idxs[B - 1] - p.grid.index_offset)
    assert last == int(np.argmax(acq)) and same_bits(vals[B - 1], acq[last])


# ---- posterior ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,d,B,causal,task,offset", CASES)
def test_last_pick_against_the_long_double_refit(lib, n, m, d, B, causal, task, offset):
    g, grid, data = make_case(n, m, d, causal, offset=offset)
    X, y, Xs = data["X"], data["y"], data["Xs"]
    y_best = float(y.min() if task == "min" else y.max())
    vals, idxs, acq, mean, var = batch_log(lib, g, grid, y_best, task, B)
    picks = (idxs - offset)[:B - 1]                               # the device's own picks: no near-tie decides this check
    tk = dict(variance=HYPER["variance"], lengthscale=HYPER["lengthscale"], noise_var=HYPER["noise_var"],
              diag_add=HYPER["noise_var"] + 1e-8)
    mean_t0, _, _ = truth_predict(X, y, Xs, data["mX"], data["vX"], data["mXs"], data["vXs"], **tk)
    Xa = np.vstack([X, Xs[picks]])
    ya = np.vstack([y, mean_t0[picks]])
    mXa = vXa = None
    if causal:
        mXa = np.vstack([data["mX"], data["mXs"][picks]])
        vXa = np.vstack([data["vX"], data["vXs"][picks]])
    mean_t, var_t, _ = truth_predict(Xa, ya, Xs, mXa, vXa, data["mXs"], data["vXs"], **tk)
    post = O.fit(Xa, ya, mXa, vXa, **HYPER)
    mean_o, var_o = O.predict(post, Xs, data["mXs"], data["vXs"])
    print("var: ", assert_parity(var, var_o, var_t, "variance at the last pick"))
    print("mean:", assert_parity(mean, mean_o, mean_t, "mean at the last pick"))
    grid.close()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("name", ["causal_d2", "graph_ard_d4", "complete_bo_d3"])
def test_the_picks_are_the_restatements(lib, name, update):
    B = 4
    g, grid, f = fixture_case(name)
    ref = log_believer(f, B, update_incumbent=bool(update))
    assert np.all(ref["log_gap"] > 1e-6), ref["log_gap"]           # no near-tie decides a pick of the restatement
    vals, idxs, *_ = batch_log(lib, g, grid, float(f["y_best"]), f["task"], B, cost=float(f["cost"]), update=update)
    print(name, update, "device", idxs, vals, "restatement", ref["idx"], ref["val"], "log gaps", ref["log_gap"])
    assert np.array_equal(idxs, ref["idx"])
    # where the EI is representable the EI form picks the same points
    rc, _, ei_idxs, *_ = batch(lib, g, grid, float(f["y_best"]), f["task"], B, cost=float(f["cost"]), update=update)
    assert rc == 0 and np.array_equal(ei_idxs, idxs)
    grid.close()


def test_update_incumbent_for_the_max_task(lib):
    """Task 'max' is the mirror: y_best <- max(y_best, mean_p), on the fixture test_batch_gpu's max-task test mirrors."""
    g, grid, f = fixture_case("graph_ard_d4")
    first = log_believer(f, 1, task="max", y_best=0.0)
    y_best = float(first["mean"][first["idx"][0], 0]) - 1.0
    moved = log_believer(f, 3, y_best=y_best, task="max", update_incumbent=True)
    fixed = log_believer(f, 3, y_best=y_best, task="max")
    assert np.all(moved["log_gap"] > 1e-6) and np.all(fixed["log_gap"] > 1e-6)
    assert moved["y_best"][1] > y_best                             # the incumbent does move
    for ref, update in ((moved, 1), (fixed, 0)):
        vals, idxs, *_ = batch_log(lib, g, grid, y_best, "max", 3, cost=float(f["cost"]), update=update)
        print("max", update, idxs, vals, ref["idx"], ref["val"])
        assert np.array_equal(idxs, ref["idx"])
    grid.close()


# ---- the dead region ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below,B,ei_idx,log_idx", [(0.5, 3, [69, 15, 0], [69, 15, 191]), (3.0, 2, [0, 0], [79, 191])])
def test_where_the_ei_is_an_exact_zero_the_log_batch_still_picks(lib, below, B, ei_idx, log_idx):
    from cbo_with_oop_amd import CandidateGrid
    f = dead_region_problem()
    g = gp(f["X"], f["y"], variance=1.0, lengthscale=1.0, noise_var=1e-10)
    grid = CandidateGrid(f["Xs"], g)
    y_best = f["y_best"] - below
    for update in (0, 1):
        rc, ei_vals, ei_idxs, *_ = batch(lib, g, grid, y_best, "min", B, update=update)
        assert rc == 0
        vals, idxs, *_ = batch_log(lib, g, grid, y_best, "min", B, update=update)
        print(below, update, "EI", ei_idxs.tolist(), ei_vals.tolist(), "log", idxs.tolist(), vals.tolist())
        assert ei_idxs.tolist() == ei_idx and ei_vals[-1] == 0.0
        assert idxs.tolist() == log_idx
        assert np.all(np.isfinite(vals)) and np.all(np.diff(vals) < 0)
    grid.close(); g.close()


# ---- the one launch against the per-set calls --------------------------------------------------------------------------------
def sets_batch_log(lib, models, grids, y_best, task, B, costs, update=0, jitter=0.0):
    """cbo_acq_sweep_sets_batch_logei: (values (S, B), indices (S, B))."""
    s = len(models)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)))
    cs = np.ascontiguousarray(np.broadcast_to(np.asarray(costs, dtype=np.float64), (s,)))
    vals, idxs = np.full(s * B, -7.0), np.full(s * B, -7, dtype=np.int64)
    lib.check(lib.load().cbo_acq_sweep_sets_batch_logei(s, handles(models), handles(grids), lib.dptr(yb), lib.TASK_CODE[task],
                                                        float(jitter), lib.dptr(cs), int(B), int(update), lib.dptr(vals),
                                                        idxs.ctypes.data_as(lib.c_int64_p)))
    return vals.reshape(s, B), idxs.reshape(s, B)


def per_set_batch_log(lib, twins, twin_grids, y_best, task, B, costs, update=0, jitter=0.0):
    """The reference: cbo_acq_sweep_batch_logei set by set on fitted twins."""
    s = len(twins)
    yb, cs = np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)), np.broadcast_to(np.asarray(costs, float), (s,))
    vals, idxs = np.empty((s, B)), np.empty((s, B), dtype=np.int64)
    for i, (g, grid) in enumerate(zip(twins, twin_grids)):
        g.ensure_fitted()
        vals[i], idxs[i] = batch_log(lib, g, grid, yb[i], task, B, cost=cs[i], jitter=jitter, update=update, want=False)[:2]
    return vals, idxs


def check_log_call(lib, pairs, y_best, task, B, costs, update=0, jitter=0.0, what=""):
    got = sets_batch_log(lib, [p.model for p in pairs], [p.grid for p in pairs], y_best, task, B, costs, update, jitter)
    want = per_set_batch_log(lib, [p.twin for p in pairs], [p.twin_grid for p in pairs], y_best, task, B, costs, update, jitter)
    assert_same(got, want, what)
    return got


# (n, m, B): one row and one candidate; a ragged tile; 16 rows under one strip; more than one block of candidates; a full
# block of rows; the one launch's cap; B = m
SHAPES = [(1, 1, 1), (1, 5, 3), (16, 63, 5), (17, 257, 5), (128, 200, 4), (50, 1024, 3), (64, 64, 64)]
COSTS = (2.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def shape_pairs(lib):
    """Per shape two sets, a causal one in one dimension behind an index offset and an ARD one in three."""
    pairs = {(n, m): [Pair(n=n, m=m, d=1, causal=True, offset=1000 + n), Pair(n=n, m=m, d=3, ard=True)] for n, m, _ in SHAPES}
    yield pairs
    for two in pairs.values():
        for p in two:
            p.close()


@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("n,m,B", SHAPES)
def test_two_sets_in_one_launch_are_the_per_set_calls(lib, shape_pairs, n, m, B, task, update):
    pairs = shape_pairs[(n, m)]
    # a live incumbent for one set, a dead one (far outside the targets' range) for the other
    y_best = [0.1, -40.0] if task == "min" else [40.0, 0.3]
    check_log_call(lib, pairs, y_best, task, B, COSTS[:2], update, jitter=0.01, what=f"n={n} m={m} B={B} {task} update={update}")
    out = np.empty(1)
    for p in pairs:                                                # the one launch needs no fit and touches no model
        assert lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == NOT_FITTED, "a model was fitted"


@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
def test_nine_sets_in_one_launch_are_the_per_set_calls(lib, shape_pairs, task, update):
    """Nine sets: the descriptors travel through the pinned array.  Every shape with at least three candidates, both sets of
    the first three."""
    keys = [(n, m) for n, m, _ in SHAPES if m >= 3]
    pairs = [shape_pairs[k][i % 2] for i, k in enumerate(keys)] + [shape_pairs[k][(i + 1) % 2] for i, k in enumerate(keys[:3])]
    assert len(pairs) == 9
    y_best = np.where(np.arange(9) % 2 == 0, 0.2, -25.0 if task == "min" else 25.0)
    costs = [COSTS[i % 3] for i in range(9)]
    check_log_call(lib, pairs, y_best, task, 3, costs, update, what=f"nine sets {task} update={update}")


def test_a_batch_of_one_is_the_multi_set_log_ei_sweep(lib, shape_pairs):
    pairs = shape_pairs[(17, 257)] + shape_pairs[(1, 1)]
    models, grids = [p.model for p in pairs], [p.grid for p in pairs]
    s = len(pairs)
    yb, cs = np.array([0.1, -30.0, 0.2, 0.3]), np.array([2.0, 1.0, 0.5, 2.0])
    vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
    lib.check(lib.load().cbo_acq_sweep_sets_logei(s, handles(models), handles(grids), lib.dptr(yb), 0, 0.01, lib.dptr(cs),
                                                  lib.dptr(vals), idxs.ctypes.data_as(lib.c_int64_p)))
    got = sets_batch_log(lib, models, grids, yb, "min", 1, cs, 0, 0.01)
    assert_same((got[0][:, 0], got[1][:, 0]), (vals, idxs), "B = 1")


# ---- the general path inside the call ----------------------------------------------------------------------------------------
def test_wide_large_and_fp32_sets_take_the_general_path_inside_the_call(lib):
    from cbo_with_oop_amd import CandidateGrid
    wide, large, single = Pair(n=50, m=1025, d=1), Pair(n=129, m=100, d=3, ard=True), Pair(n=50, m=100, d=1, dtype="f32")
    small, fitted = Pair(n=17, m=65, d=1, causal=True), Pair(n=50, m=200, d=3, causal=True, fit=True)
    kept = CandidateGrid(fitted.grid.points, fitted.model, keep_solution=True)
    pairs = [wide, small, large, single, fitted]
    models = [p.model for p in pairs]
    grids = [wide.grid, small.grid, large.grid, single.grid, kept]
    y_best, costs = [0.1, -20.0, 0.2, 0.0, -15.0], [2.0, 1.0, 0.5, 1.0, 2.0]
    out, lml0, lml1 = np.empty(1), np.empty(1), np.empty(1)
    lib.check(lib.load().cbo_gp_log_marginal(fitted.model._handle, lib.dptr(lml0)))
    before = single_log(lib, fitted.model, kept, -15.0, "min", cost=2.0)
    for update in (0, 1):
        got = sets_batch_log(lib, models, grids, y_best, "min", 3, costs, update)
        want = per_set_batch_log(lib, [p.twin for p in pairs], [p.twin_grid for p in pairs], y_best, "min", 3, costs, update)
        assert_same(got, want, f"general path, update={update}")
        assert lib.load().cbo_gp_log_marginal(small.model._handle, lib.dptr(out)) == NOT_FITTED   # the one launch's: untouched
        for p in (wide, large, single):                           # the general path fitted them inside the call
            assert lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == 0
    # the fitted model: its likelihood, its cached sweep and its kept solution are what they were
    lib.check(lib.load().cbo_gp_log_marginal(fitted.model._handle, lib.dptr(lml1)))
    assert same_bits(lml0, lml1)
    after = single_log(lib, fitted.model, kept, -15.0, "min", cost=2.0)
    assert all(same_bits(a, b) for a, b in zip(before, after))
    kept.close()
    for p in pairs:
        p.close()


# ---- the two forms together --------------------------------------------------------------------------------------------------
def test_on_a_live_fixture_the_log_form_is_the_logarithm_of_the_ei_form(lib):
    p = Pair(n=17, m=257, d=3, fit=True)
    B = 4
    worst = 0.0
    for update in (0, 1):
        rc, ei_vals, ei_idxs, *_ = batch(lib, p.model, p.grid, 0.1, "min", B, cost=2.0, update=update)
        assert rc == 0 and np.all(ei_vals > 0)
        vals, idxs, *_ = batch_log(lib, p.model, p.grid, 0.1, "min", B, cost=2.0, update=update)
        rel = np.abs(np.exp(vals) - ei_vals) / ei_vals
        print("update", update, idxs.tolist(), "EI", ei_vals.tolist(), "exp(log)", np.exp(vals).tolist(), "relative", rel.tolist())
        assert np.array_equal(idxs, ei_idxs)
        worst = max(worst, rel.max())
    print("worst relative difference", worst)
    assert worst <= 1e-12
    p.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------
def test_the_python_layers_return_the_c_calls_points(lib):
    """The toy graph's two sets under its variable cost (type 4): find_next_y_points against the multi-set call, and per set
    find_next_y_point and the calculator over log EI / Cost against the single-set call."""
    from cbo_with_oop_amd import find_next_y_point
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import (CausalGradientAcquisitionOptimizer, Cost, GreedyBatchPointCalculator,
                                                  find_next_y_points)
    from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement
    es, table = ToyGraph.get_exploration_set("MIS"), ToyGraph.get_cost_structure(4)
    pairs = [Pair(n=50, m=200, d=1, causal=True, fit=True), Pair(n=17, m=65, d=1, fit=True)]
    models, grids = [p.model for p in pairs], [p.grid for p in pairs]
    batch_costs = [float(Cost(table, es[i]).evaluate(grids[i].points)) for i in range(2)]
    y_best = -30.0                                                 # a dead incumbent: the EI form's picks would all be 0
    for update in (False, True):
        xs, ys = find_next_y_points(models, y_best, es, table, "min", grids, acquisition="LOGBEI", acquisition_param=0.01,
                                    batch_size=3, update_incumbent=update)
        vals, idxs = sets_batch_log(lib, models, grids, y_best, "min", 3, batch_costs, int(update), 0.01)
        for i in range(2):
            assert xs[i].shape == (3, 1) and ys[i].shape == (3, 1)
            assert np.array_equal(xs[i], grids[i].points[idxs[i]])
            assert len(set(idxs[i].tolist())) == 3                 # three distinct interventions
            for t in (1, 2):                                       # the later picks: the batch's log cost for the point's own
                point = float(Cost(table, es[i]).evaluate(xs[i][t:t + 1]))
                assert ys[i][t, 0] == (vals[i][t] + np.log(batch_costs[i])) - np.log(point)
    xs, ys = find_next_y_points(models, y_best, es, table, "min", grids, acquisition="LOGBEI", batch_size=3)
    for i in range(2):
        v, ix, *_ = batch_log(lib, pairs[i].twin, pairs[i].twin_grid, y_best, "min", 3, cost=batch_costs[i], want=False)
        y, x = find_next_y_point(None, pairs[i].twin, y_best, es[i], table, candidates=pairs[i].twin_grid, acquisition="LOGBEI",
                                 batch_size=3)
        assert np.array_equal(x, pairs[i].twin_grid.points[ix]) and np.array_equal(x, xs[i])
        assert np.array_equal(y.view(np.uint64), ys[i].view(np.uint64)), (y, ys[i])
        # the calculator over log EI / Cost: the same rows
        pts = pairs[i].twin_grid.points
        opt = CausalGradientAcquisitionOptimizer([(-2.5, 2.5)], grid_shape=[8])
        opt.candidates = lambda pts=pts: pts
        acquisition = CausalLogExpectedImprovement(y_best, "min", pairs[i].twin) / Cost(table, es[i])
        calc = GreedyBatchPointCalculator(pairs[i].twin, acquisition, opt, 3)
        rows = calc.compute_next_points()
        assert np.array_equal(rows, x) and same_bits(calc.last_result["best_val"], v)
        opt._grid.close()
    for p in pairs:
        p.close()


def test_the_agent_runs_its_log_batches(lib):
    """CBO(toy graph, acquisition="LOGBEI", batch_size=3).run(): four trials; every intervention grows the chosen set's data
    -- and the monitor's record of it -- by its three rows, in order."""
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model

    class Toy(ToyGraph):
        """The toy graph with what an observe step needs: its manipulative variables and one graph GP per set."""
        manipulative_variables = ("X", "Z")
        _fit_dependencies = (("X",), ("Z",))
        _fit_parameters = ([1.0, 1.0, 10.0, False], [1.0, 1.0, 10.0, False])

    sem = Toy.define_sem()
    rng = np.random.default_rng(11)
    draws = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(60)]
    obs = {v: np.array([r[v] for r in draws]) for v in draws[0] if not v.startswith("U")}
    init = {k: v[:40] for k, v in obs.items()}
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    xs = [rng.uniform(-5, 5, (6, 1)), rng.uniform(-5, 20, (6, 1))]
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=4, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, acquisition="LOGBEI",
                    batch_size=3, update_incumbent=True)
        mon = agent.run()
    assert len(mon.type_trial) == 4 and 1 in mon.type_trial
    chosen = [c for c in mon.chosen if c is not None]
    assert len(chosen) == sum(mon.type_trial)
    rows = [6, 6]
    grown = [xs[0].copy(), xs[1].copy()]
    for picked_set, picked_x in chosen:
        s = [list(e) for e in es].index(list(picked_set))
        assert picked_x.shape == (3, 1)
        rows[s] += 3
        grown[s] = np.vstack([grown[s], picked_x])
    assert [x.shape[0] for x in agent.data_x] == rows and [y.shape[0] for y in agent.data_y] == rows
    assert all(np.array_equal(a, b) for a, b in zip(agent.data_x, grown))                  # rows appended in order
    assert len(mon.global_opt) == len(mon.current_cost) and mon.cumulative_cost > 0
