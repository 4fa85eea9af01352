"""GPU tests of greedy batch selection in the one-launch multi-set sweep and the agent:
cbo_acq_sweep_sets_batch (small_sets_batch_kernel, kernels_sets_batch.hip) and the Python layer on top.

The contract is bit for bit: values as bit patterns, indices equal, every pick -- against cbo_acq_sweep_batch set by set on
freshly FITTED twin models, never the code under test.  Shapes are the smallest at which each piece can go wrong:
n in {1, 17, 50, 64, 65, 128} (one row; a ragged tile; 64 / 65 either side of the one- / two-slice boundary of the pass over
V, rows_per_slice 64 / 40; a full block), m in {2, 64, 65, 130, 200} with sets narrower than the call's widest (a spare
workgroup can be the last arriver), 704 / 768 candidates (11 and 12 blocks: either side of the two-launch threshold), 1024 /
1025 (either side of the one launch's cap), B in {1, 2, 3, 9} and 64 at m = 64, d in {1, 3, 8}, ARD and not, causal and
plain, both tasks, update_incumbent 0 and 1, index offsets, three sets (descriptors by value) and nine (the pinned array).
One accuracy check uses the bar tests/test_batch_gpu.py applies to the single-set call (conftest.assert_parity against the
restatement of emukit's loop on the oracle, sets_batch_support.believer)."""
import ctypes

import numpy as np
import pytest

from sets_batch_support import (Pair, assert_same, believer, check_call, check_values, fixture_model, handles, per_set_batch,
                                sets_batch)

pytestmark = pytest.mark.gpu

NOT_FITTED = -5


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


# group -> (sets, batch sizes); the widest set of a call decides its grid and its one- / two-launch form
GROUPS = {
    "three sets": ([dict(n=1, m=2, d=1), dict(n=17, m=65, d=3, ard=True, offset=5000), dict(n=50, m=200, d=1, causal=True)],
                   (2,)),
    "nine sets": ([dict(n=1, m=64, d=1), dict(n=17, m=64, d=3, causal=True), dict(n=50, m=65, d=8, ard=True),
                   dict(n=64, m=130, d=1), dict(n=65, m=200, d=3, causal=True, offset=77), dict(n=128, m=200, d=8),
                   dict(n=64, m=64, d=1, causal=True), dict(n=65, m=65, d=3, ard=True),
                   dict(n=128, m=130, d=1, causal=True, offset=123456)], (3, 9)),
    "11 blocks": ([dict(n=50, m=704, d=2), dict(n=17, m=65, d=1, causal=True)], (2, 9)),
    "12 blocks": ([dict(n=50, m=768, d=2, causal=True), dict(n=17, m=65, d=1), dict(n=65, m=130, d=3, ard=True)], (2, 9)),
    "the cap": ([dict(n=50, m=1024, d=1), dict(n=50, m=1025, d=1), dict(n=65, m=64, d=1, causal=True)], (3,)),
    "mixed": ([dict(n=50, m=130, d=1, causal=True), dict(n=50, m=100, d=1, dtype="f32"), dict(n=200, m=100, d=3)], (3,)),
}


@pytest.fixture(scope="module")
def zoo(lib):
    groups = {name: [Pair(**kw) for kw in sets] for name, (sets, _) in GROUPS.items()}
    yield groups
    for pairs in groups.values():
        for p in pairs:
            p.close()


def scalars(pairs):
    s = len(pairs)
    return np.linspace(-0.4, 0.6, s), 1.0 + np.arange(s) % 3           # incumbents inside the targets' range; costs


@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("task", ["min", "max"])
@pytest.mark.parametrize("name", list(GROUPS))
def test_every_pick_is_the_single_set_calls(lib, zoo, name, task, update):
    pairs = zoo[name]
    y_best, costs = scalars(pairs)
    for B in GROUPS[name][1]:
        check_call(lib, pairs, y_best, task, B, costs, update, jitter=0.01, what=f"{name} {task} update={update} B={B}")
    # the one launch needs no fit and leaves the models alone: an unfitted small model is still unfitted
    out = np.empty(1)
    for p in pairs:
        if p.n <= 128 and p.m <= 1024 and p.dtype == "f64":
            assert lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == NOT_FITTED, "a model was fitted"


def test_a_batch_of_64_at_64_candidates(lib):
    pairs = [Pair(n=50, m=64, d=1), Pair(n=17, m=200, d=3, causal=True)]
    y_best, costs = scalars(pairs)
    vals, idxs = check_call(lib, pairs, y_best, "min", 64, costs, 1, what="B = 64")
    assert np.all((idxs[0] >= 0) & (idxs[0] < 64))
    for p in pairs:
        p.close()


def sweep_sets(lib, models, grids, y_best, task, costs, jitter=0.0):
    s = len(models)
    yb, cs = np.ascontiguousarray(y_best, dtype=np.float64), np.ascontiguousarray(costs, dtype=np.float64)
    vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
    lib.check(lib.load().cbo_acq_sweep_sets(s, handles(models), handles(grids), lib.dptr(yb), lib.TASK_CODE[task], float(jitter),
                                            lib.dptr(cs), lib.dptr(vals), idxs.ctypes.data_as(lib.c_int64_p)))
    return vals, idxs


@pytest.mark.parametrize("name", ["three sets", "12 blocks", "mixed"])
def test_a_batch_of_one_and_pick_0_are_the_plain_multi_set_sweep(lib, zoo, name):
    pairs = zoo[name]
    models, grids = [p.model for p in pairs], [p.grid for p in pairs]
    y_best, costs = scalars(pairs)
    want = sweep_sets(lib, models, grids, y_best, "min", costs, 0.01)
    rc, vals, idxs = sets_batch(lib, models, grids, y_best, "min", 1, costs, 0, 0.01)
    lib.check(rc)
    assert_same((vals[:, 0], idxs[:, 0]), want, "B = 1")
    rc, vals, idxs = sets_batch(lib, models, grids, y_best, "min", 2, costs, 0, 0.01)
    lib.check(rc)
    # (an fp32 model's batch answers from its fp64 factor -- cbo_acq_sweep_batch's contract -- its plain sweep from the fp32 one)
    f64 = [i for i, p in enumerate(pairs) if p.dtype == "f64"]
    assert_same((vals[f64, 0], idxs[f64, 0]), (want[0][f64], want[1][f64]), "pick 0")


def plain(lib, g, grid, y_best, cost):
    m = len(grid)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep(g._handle, grid._handle, float(y_best), 0, 0.0, float(cost), lib.dptr(acq),
                                       lib.dptr(mean), lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi)))
    return acq, mean, var, np.array([bv.value]), np.array([bi.value])


@pytest.mark.parametrize("keep", [False, True])
def test_models_and_candidates_are_left_as_they_were_and_two_calls_agree(lib, keep):
    from cbo_with_oop_amd import CandidateGrid
    fitted, unfitted = Pair(n=50, m=200, d=3, causal=True, fit=True), Pair(n=65, m=130, d=1)
    grid = CandidateGrid(fitted.grid.points, fitted.model, keep_solution=keep)
    models, grids = [fitted.model, unfitted.model], [grid, unfitted.grid]
    before = plain(lib, fitted.model, grid, 0.1, 2.0)
    rc, vals, idxs = sets_batch(lib, models, grids, [0.1, 0.2], "min", 5, [2.0, 1.0], 1)
    lib.check(rc)
    after = plain(lib, fitted.model, grid, 0.1, 2.0)
    for x, z in zip(before, after):
        assert np.array_equal(x.view(np.uint64), z.view(np.uint64))
    out = np.empty(1)
    assert lib.load().cbo_gp_log_marginal(unfitted.model._handle, lib.dptr(out)) == NOT_FITTED
    rc, vals2, idxs2 = sets_batch(lib, models, grids, [0.1, 0.2], "min", 5, [2.0, 1.0], 1)
    lib.check(rc)
    assert_same((vals2, idxs2), (vals, idxs), "the second call")
    want = per_set_batch(lib, [fitted.twin, unfitted.twin], [fitted.twin_grid, unfitted.twin_grid], [0.1, 0.2], "min", 5,
                         [2.0, 1.0], 1)
    assert_same((vals, idxs), want, "against the twins")
    grid.close(); fitted.close(); unfitted.close()


def test_a_set_the_launch_declines_takes_the_general_path_between_its_neighbours(lib):
    """The jitter fixture (duplicate rows under a negative noise: the launch's pivot at the duplicate is about -2e-9, far
    below rounding, so it declines there) between two ordinary small sets: every set's picks are cbo_acq_sweep_batch's on a
    fitted twin; the declined set's model was fitted by the general path, with jitter, the neighbours' were not; the same
    call again and a call of the neighbours alone return the same bits."""
    ladder, ladder_grid, f = fixture_model("jitter_ladder", fit=False)
    twin, twin_grid, _ = fixture_model("jitter_ladder", fit=True)
    first, last = Pair(n=17, m=65, d=1), Pair(n=25, m=70, d=1, causal=True)
    models, grids = [first.model, ladder, last.model], [first.grid, ladder_grid, last.grid]
    twins, twin_grids = [first.twin, twin, last.twin], [first.twin_grid, twin_grid, last.twin_grid]
    y_best, costs = [-0.1, float(f["y_best"]), 0.2], [2.0, 1.0, 3.0]
    out, tries = np.empty(1), ctypes.c_int(-1)
    for update in (0, 1):
        rc, vals, idxs = sets_batch(lib, models, grids, y_best, "min", 3, costs, update)
        lib.check(rc)
        want = per_set_batch(lib, twins, twin_grids, y_best, "min", 3, costs, update)
        assert_same((vals, idxs), want, f"ladder between neighbours, update={update}")
        assert lib.load().cbo_gp_log_marginal(ladder._handle, lib.dptr(out)) == 0          # the general path fitted it ...
        assert lib.load().cbo_gp_jitter(ladder._handle, ctypes.byref(tries), None) == 0 and tries.value >= 1   # ... by the ladder
        for p in (first, last):
            assert lib.load().cbo_gp_log_marginal(p.model._handle, lib.dptr(out)) == NOT_FITTED
        rc, vals2, idxs2 = sets_batch(lib, models, grids, y_best, "min", 3, costs, update)
        lib.check(rc)
        assert_same((vals2, idxs2), (vals, idxs), "the same call again")
        rc, vals3, idxs3 = sets_batch(lib, models[::2], grids[::2], y_best[::2], "min", 3, costs[::2], update)
        lib.check(rc)
        assert_same((vals3, idxs3), (want[0][::2], want[1][::2]), "the neighbours alone, right after")
    assert twin.jitter_tries >= 1                                                          # the premise: the fixture needs it
    for o in (ladder_grid, twin_grid, ladder, twin):
        o.close()
    first.close(); last.close()


def test_the_picks_are_the_restatements_under_the_single_set_calls_bar(lib):
    B = 5
    cases = [fixture_model(name, fit=False) for name in ("causal_d2", "complete_bo_d3")]
    for g, grid, f in cases:
        assert f["X"].shape[0] <= 128 and f["Xs"].shape[0] <= 1024          # (the one launch takes them)
    y_best = [float(f["y_best"]) for _, _, f in cases]
    costs = [float(f["cost"]) for _, _, f in cases]
    assert len({f["task"] for _, _, f in cases}) == 1
    task = cases[0][2]["task"]
    rc, vals, idxs = sets_batch(lib, [c[0] for c in cases], [c[1] for c in cases], y_best, task, B, costs)
    lib.check(rc)
    for i, (g, grid, f) in enumerate(cases):
        ref = believer(f, B)
        assert np.all(ref["gap"] > 1e-6), ref["gap"]                   # no near-tie decides a pick of the restatement
        print("device", idxs[i], vals[i], "restatement", ref["idx"], ref["val"])
        assert np.array_equal(idxs[i], ref["idx"])
        check_values(f, ref, vals[i], task, costs[i])
        grid.close()


@pytest.mark.parametrize("cost_type", [1, 4])
def test_find_next_y_points_is_find_next_y_point_per_set(lib, cost_type):
    """Fixed costs and variable ones (pick 0 re-evaluated, the later picks rescaled), on fitted models."""
    from cbo_with_oop_amd import find_next_y_point
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import Cost, find_next_y_points
    es, table = ToyGraph.get_exploration_set("MIS"), ToyGraph.get_cost_structure(cost_type)
    pairs = [Pair(n=50, m=200, d=1, causal=True, fit=True), Pair(n=17, m=65, d=1, fit=True)]
    models, grids = [p.model for p in pairs], [p.grid for p in pairs]
    for update in (False, True):
        xs, ys = find_next_y_points(models, 0.1, es, table, "min", grids, batch_size=3, update_incumbent=update)
        rc, vals, idxs = sets_batch(lib, models, grids, 0.1, "min", 3, [float(Cost(table, es[i]).evaluate(grids[i].points))
                                                                        for i in range(2)], int(update))
        lib.check(rc)
        for i in range(2):
            assert xs[i].shape == (3, 1) and ys[i].shape == (3, 1)
            assert np.array_equal(xs[i], grids[i].points[idxs[i]])
        if not update:                                               # (the per-set Python call has no update_incumbent)
            for i in range(2):
                y, x = find_next_y_point(None, pairs[i].twin, 0.1, es[i], table, candidates=pairs[i].twin_grid, batch_size=3)
                assert np.array_equal(xs[i], x)
                assert np.array_equal(ys[i].view(np.uint64), y.view(np.uint64)), (ys[i], y)
    for p in pairs:
        p.close()


@pytest.mark.parametrize("cost_type", [1, 4])
def test_a_batch_of_one_above_the_cap_leaves_a_small_model_unfitted_and_python_knows(lib, cost_type):
    """batch_size=1 is cbo_acq_sweep_sets' route: a small model is swept in the one launch whatever its grid, so with 1025
    candidates it is still unfitted afterwards and its wrapper still says so -- the variable-cost re-evaluation of pick 0
    (cost type 4) then fits it on demand instead of meeting an unfitted device model.  From B = 2 on the general path fits it."""
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import find_next_y_points
    table = ToyGraph.get_cost_structure(cost_type)
    pair = Pair(n=50, m=1025, d=1)
    out = np.empty(1)
    assert pair.model.stale and lib.load().cbo_gp_log_marginal(pair.model._handle, lib.dptr(out)) == NOT_FITTED
    xs, ys = find_next_y_points([pair.model], 0.1, [["X"]], {"X": lambda col: 2.0}, "min", [pair.grid], batch_size=1)
    assert xs[0].shape == (1, 1) and ys[0].shape == (1, 1)
    assert pair.model.stale and lib.load().cbo_gp_log_marginal(pair.model._handle, lib.dptr(out)) == NOT_FITTED
    want = per_set_batch(lib, [pair.twin], [pair.twin_grid], 0.1, "min", 1, 2.0)
    assert np.array_equal(xs[0], pair.grid.points[want[1][0]]) and ys[0][0, 0] == want[0][0, 0]
    xs, ys = find_next_y_points([pair.model], 0.1, [["X"]], table, "min", [pair.grid], batch_size=1)
    assert np.array_equal(xs[0], pair.grid.points[want[1][0]]) and np.isfinite(ys[0][0, 0])
    if cost_type == 1:
        assert pair.model.stale and lib.load().cbo_gp_log_marginal(pair.model._handle, lib.dptr(out)) == NOT_FITTED
    other = Pair(n=50, m=1025, d=1, seed=1)
    xs, ys = find_next_y_points([other.model], 0.1, [["X"]], table, "min", [other.grid], batch_size=2)
    assert xs[0].shape == (2, 1) and not other.model.stale
    assert lib.load().cbo_gp_log_marginal(other.model._handle, lib.dptr(out)) == 0
    pair.close(); other.close()


def test_the_agent_runs_its_batches(lib):
    """CBO(toy graph, batch_size=3).run(): every intervention grows the chosen set's data by its 3 rows, in order."""
    import warnings
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
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, batch_size=3,
                    update_incumbent=True)
        mon = agent.run()
    assert len(mon.type_trial) == 4 and 1 in mon.type_trial
    chosen = [c for c in mon.chosen if c is not None]
    assert len(chosen) == sum(mon.type_trial)
    rows = [6, 6]
    grown = [xs[0].copy(), xs[1].copy()]
    for picked_set, picked_x in chosen:
        s = es.index(picked_set) if picked_set in es else [list(e) for e in es].index(picked_set)
        assert picked_x.shape == (3, 1)
        rows[s] += 3
        grown[s] = np.vstack([grown[s], picked_x])
    assert [x.shape[0] for x in agent.data_x] == rows and [y.shape[0] for y in agent.data_y] == rows
    assert all(np.array_equal(a, b) for a, b in zip(agent.data_x, grown))                  # rows appended in order
    assert len(mon.global_opt) == len(mon.current_cost) and mon.cumulative_cost > 0
