"""CPU tests of the observe step's host logic: the lockstep L-BFGS-B driver (every problem on the trajectory
``fmin_l_bfgs_b`` gives it alone), the convex-hull coverage behind epsilon, the graph-GP tables and the agent's
epsilon-greedy loop."""
import itertools

import numpy as np
import pytest
from scipy.optimize import fmin_l_bfgs_b

from oracle import gp_oracle as O


def _graph_gp_problem(seed, n, d, ard, fail_below=None):
    """paramz's objective of a graph GP (noise fixed at 1e-2, Logexp) with the oracle's likelihood and gradients.
    ``fail_below``: points whose first parameter is below it fail like a factorisation that is not positive definite."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X[:, :1]) + 0.3 * X[:, -1:] + 0.1 * rng.standard_normal((n, 1))
    nl = d if ard else 1

    def f(x):
        th = O.logexp_f(x)
        if fail_below is not None and x[0] < fail_below:
            return 1e25, np.zeros_like(x)
        post = O.fit(X, y, variance=th[0], lengthscale=th[1:1 + nl] if ard else th[1], noise_var=1e-2)
        dv, dls, _ = O.log_marginal_likelihood_gradients(post)
        g = np.asarray([dv, *np.atleast_1d(dls)]) * O.logexp_gradfactor(th)
        return -O.log_marginal_likelihood(post), -g

    return f, O.logexp_finv(np.ones(1 + nl))


PROBLEMS = [(0, 12, 1, False, None), (1, 30, 2, True, None), (2, 45, 3, False, None), (3, 25, 4, True, None),
            (4, 60, 1, False, -0.3), (5, 18, 5, True, None), (6, 40, 2, False, None)]


@pytest.mark.parametrize("maxfun", [1000, 9])
def test_lockstep_lbfgsb_follows_each_problem_alone(maxfun):
    """K = 7 problems advanced together, one batched evaluation per round, end where ``fmin_l_bfgs_b`` ends each
    alone: same x (bitwise), f, nfev, nit, warnflag and message; they converge at different rounds, and with
    ``maxfun`` = 9 some stop on it."""
    from cbo_with_oop_amd.utils_functions.lockstep_lbfgsb import lockstep_fmin_l_bfgs_b
    probs = [_graph_gp_problem(*p) for p in PROBLEMS]
    alone = [fmin_l_bfgs_b(f, x0, maxfun=maxfun, maxiter=maxfun) for f, x0 in probs]
    rounds = []

    def evaluate(ks, xs):
        rounds.append(list(ks))
        return [probs[k][0](x) for k, x in zip(ks, xs)]

    together = lockstep_fmin_l_bfgs_b(evaluate, [x0 for _, x0 in probs], maxfun=maxfun, maxiter=maxfun)
    for (xa, fa, da), (xb, fb, db) in zip(alone, together):
        np.testing.assert_array_equal(xa, xb)
        assert fa == fb
        assert (da["funcalls"], da["nit"], da["warnflag"], da["task"]) == \
               (db["funcalls"], db["nit"], db["warnflag"], db["task"])
        np.testing.assert_array_equal(da["grad"], db["grad"])
    # every evaluation went through a batched round; the batches shrink as problems finish
    assert sum(len(r) for r in rounds) == sum(d["funcalls"] for _, _, d in alone)
    assert len(rounds) == max(d["funcalls"] for _, _, d in alone)
    if maxfun == 9:
        assert any(d["warnflag"] == 1 for _, _, d in alone)
    else:
        assert all(d["warnflag"] == 0 for _, _, d in alone)
        assert len({d["funcalls"] for _, _, d in alone}) > 1


def test_lockstep_lbfgsb_falls_back_to_sequential_runs(monkeypatch):
    """An unknown scipy L-BFGS-B step: a warning, and the problems are solved one by one with the same results."""
    from cbo_with_oop_amd.utils_functions import lockstep_lbfgsb as L
    probs = [_graph_gp_problem(*p) for p in PROBLEMS[:3]]
    monkeypatch.setattr(L, "_setulb", lambda: None)
    with pytest.warns(RuntimeWarning, match="one after another"):
        out = L.lockstep_fmin_l_bfgs_b(lambda ks, xs: [probs[k][0](x) for k, x in zip(ks, xs)],
                                       [x0 for _, x0 in probs], maxfun=1000, maxiter=1000)
    for (f, x0), (x, fx, d) in zip(probs, out):
        xa, fa, da = fmin_l_bfgs_b(f, x0, maxfun=1000, maxiter=1000)
        np.testing.assert_array_equal(xa, x)
        assert fa == fx and da["funcalls"] == d["funcalls"]


def test_hull_and_coverage_known_volumes():
    from cbo_with_oop_amd.utils_functions.utils import compute_coverage, update_hull
    rng = np.random.default_rng(0)
    cube = np.array(list(itertools.product([-1.0, 2.0], [0.0, 1.0], [3.0, 5.0])))
    pts = np.vstack([cube, rng.uniform([-1, 0, 3], [2, 1, 5], (40, 3))])
    obs = {"a": pts[:, 0], "b": pts[:, 1], "c": pts[:, 2], "other": np.zeros(len(pts))}
    assert update_hull(obs, ["a", "b", "c"]) == pytest.approx(6.0, rel=1e-12)
    simplex = {"a": np.array([0.0, 1, 0, 0]), "b": np.array([0.0, 0, 1, 0]), "c": np.array([0.0, 0, 0, 1])}
    assert update_hull(simplex, ["a", "b", "c"]) == pytest.approx(1.0 / 6.0, rel=1e-12)
    ranges = {"a": [0, 2], "b": [0, 2], "c": [0, 3]}
    alpha, hull, total = compute_coverage(simplex, ["a", "b", "c"], ranges)
    assert total == pytest.approx(12.0, rel=1e-12)
    assert hull.volume == pytest.approx(1.0 / 6.0, rel=1e-12)
    assert alpha == pytest.approx(1.0 / 72.0, rel=1e-12)


def test_graph_fit_tables():
    from cbo_with_oop_amd.graphs import CompleteGraph, CoralGraph, SimplifiedCoralGraph
    # the reference's complete graph lists ten fit dependencies (CompleteGraph.py:31-42), the coral graphs fifteen
    for graph, count, manip in ((CompleteGraph, 10, ["B", "D", "E"]), (CoralGraph, 15, ["N", "O", "C", "T", "D"]),
                                (SimplifiedCoralGraph, 15, ["N", "O", "C", "T", "D"])):
        g = graph()
        assert len(g.fit_dependencies) == count and len(g.fit_parameters) == count
        assert list(g.manipulative_variables) == manip
        assert all(1 <= len(d) <= 8 for d in g.fit_dependencies)
        assert all(len(p) == 4 and isinstance(p[3], bool) for p in g.fit_parameters)
        names = [g.get_gp_name(d) for d in g.fit_dependencies]
        assert names == ["gp_" + "_".join(d) for d in g.fit_dependencies] and len(set(names)) == count
    assert CompleteGraph().fit_dependencies[0] == ["B"] and CompleteGraph().fit_dependencies[-1] == list("ABCDEF")
    assert CoralGraph().fit_dependencies[12] == ["N", "C", "T", "S", "N", "L", "TE"]
    assert [p[3] for p in CoralGraph().fit_parameters[:6]] == [False, True, True, True, True, False]
    assert CompleteGraph.get_gp_name(["B", "D"]) == "gp_B_D"


def _stub_agent(n0=100, trials=12):
    """A complete-graph agent on host data whose GP work is stubbed out: observe adds the reference's rows, intervene
    only records itself."""
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import CompleteGraph
    rng = np.random.default_rng(1)
    cols = {v: rng.standard_normal(n0 + 40) * 2.0 for v in ["A", "B", "C", "D", "E", "F", "Y"]}
    data = [(rng.uniform(-1, 1, (3, len(s))), rng.standard_normal((3, 1)))
            for s in CompleteGraph.get_exploration_set("MIS")]
    agent = CBO(CompleteGraph, {k: v[:n0] for k, v in cols.items()}, cols, data, num_trials=trials,
                initial_num_obs_samples=n0, num_additional_observations=20,
                target_functions=[lambda x: np.zeros((1, 1))] * len(data))
    calls = []

    def observe():
        agent.monitor.log_agent_behaviour(act=False)
        new = agent.get_new_observation()
        agent.measurements = {k: np.vstack([v, new[k]]) for k, v in agent.measurements.items()}
        calls.append(("observe", agent.n_measurements))

    def intervene():
        agent.monitor.log_agent_behaviour(act=True)
        calls.append(("intervene", agent.n_measurements))

    agent.observe, agent.intervene = observe, intervene
    agent.graph.fit_all_gaussian_processes = lambda *a, **k: {}
    return agent, cols, calls


def test_epsilon_is_the_reference_formula():
    """CBO.py:175-188: (hull volume of B, D, E over the volume of their interventional box) / (rows / max_n)."""
    from scipy.spatial import ConvexHull
    agent, cols, _ = _stub_agent()
    pts = np.column_stack([cols[v][:100] for v in ["B", "D", "E"]])
    box = ConvexHull(list(itertools.product([-5, 4], [-5, 5], [-6, 3]))).volume
    assert box == pytest.approx(9 * 10 * 9)
    assert agent.epsilon == pytest.approx((ConvexHull(pts).volume / box) / (100 / 150), rel=1e-12)


def test_epsilon_greedy_sequence_matches_the_reference_loop():
    """With observe / intervene stubbed, a seeded run makes the choices of src/CBO.py:83-111: observe, intervene, then
    observe when numpy.random.uniform(0, 1) < epsilon (recomputed from the rows observed so far), else intervene."""
    from scipy.spatial import ConvexHull
    agent, cols, calls = _stub_agent(trials=14)
    np.random.seed(4)
    agent.run()
    # the reference's loop, replayed
    np.random.seed(4)
    rows = 100
    expected = [("observe", 120), ("intervene", 120)]
    rows = 120
    obs_rows = np.vstack([np.column_stack([cols[v][:100] for v in "BDE"]),
                          np.column_stack([cols[v][100:120] for v in "BDE"])])
    for _ in range(12):
        eps = (ConvexHull(obs_rows).volume / (9 * 10 * 9)) / (rows / 150)
        if np.random.uniform(0., 1.) < eps:
            rows += 20
            obs_rows = np.vstack([obs_rows, np.column_stack([cols[v][100:120] for v in "BDE"])])
            expected.append(("observe", rows))
        else:
            expected.append(("intervene", rows))
    assert calls == expected
    assert agent.monitor.type_trial == [0 if c == "observe" else 1 for c, _ in expected]
    assert {c for c, _ in calls} == {"observe", "intervene"}


def test_compute_cost_is_the_reference_formula():
    agent, _, _ = _stub_agent()
    xs = [np.array([[0.5]]), np.array([[-2.0]]), np.array([[1.0]]), np.array([[3.0, -1.5]])]
    agent.costs = agent.graph.get_cost_structure(3)            # fixed (different) + |x| per variable
    # set ['B', 'D'] (index 3): B costs 10, D costs 5, plus |3| + |-1.5|
    assert agent.compute_cost(["B", "D"], 3, xs) == pytest.approx(10 + 5 + 3.0 + 1.5)
