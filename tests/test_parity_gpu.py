"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the C-ABI of
libcbo_hip.so and is compared with the numpy/scipy oracle on the same seeded inputs, with the committed
golden fixtures, and -- at BASELINE.json's full size -- through size-independent properties.

Tolerance (BASELINE.json north_star): rtol 1e-5 on posterior mean/variance, identical arg-max.  See
conftest.assert_parity for how ill-conditioned cases are arbitrated by the 80-bit restatement.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import assert_parity, load_fixture
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def make_model(hip, f):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    ls = f["lengthscale_arg"]
    kw = dict(variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls), noise_var=float(f["noise_var"]))
    if f["mX"] is not None:
        lut_m = {**{tuple(r): v for r, v in zip(map(tuple, f["X"]), f["mX"][:, 0])},
                 **{tuple(r): v for r, v in zip(map(tuple, f["Xs"]), f["mXs"][:, 0])}}
        lut_v = {**{tuple(r): v for r, v in zip(map(tuple, f["X"]), f["vX"][:, 0])},
                 **{tuple(r): v for r, v in zip(map(tuple, f["Xs"]), f["vXs"][:, 0])}}
        kw["mean_function"] = lambda a: np.array([[lut_m[tuple(r)]] for r in a])
        kw["variance_adjustment"] = lambda a: np.array([[lut_v[tuple(r)]] for r in a])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(f["X"], f["y"], **kw)


def test_device_and_mfma_lane_map(hip):
    from cbo_with_oop_amd import _lib
    ctx = _lib.Context.get()
    assert "gfx950" in ctx.name()
    assert ctx.selftest_mfma() == 0.0


def test_kxx_assembly_matches_oracle(hip, golden):
    f = golden
    m = make_model(hip, f)
    K = m.assembled_Ky()
    Kref = O.causal_K(f["X"], f["X"], f["vX"], f["vX"], float(f["variance"]), f["lengthscale_arg"],
                      zero_diag=f["vX"] is None)
    Kref[np.diag_indices_from(Kref)] += float(f["noise_var"]) + 1e-8
    assert np.array_equal(K, K.T)
    # same operation order as GPy; only exp() and BLAS's dot association differ: a few ulp
    assert np.max(np.abs(K - Kref) / np.abs(Kref).clip(1e-300)) < 1e-12, golden["name"]


def test_cholesky_and_alpha(hip, golden):
    f = golden
    m = make_model(hip, f)
    assert m.jitter_tries == int(f["tries"])
    assert np.isclose(m.jitter, float(f["jitter"]), rtol=1e-12, atol=0)
    L, alpha = m.posterior_state()
    Ky = m.assembled_Ky() + m.jitter * np.eye(L.shape[0])
    resid = np.linalg.norm(L @ L.T - Ky) / np.linalg.norm(Ky)
    assert resid < 1e-14 * max(4, L.shape[0]) ** 0.5, resid          # backward stable factorisation
    assert np.all(np.triu(L, 1) == 0)
    # alpha: both fp64 solves are accurate to eps*cond(Ky); compare through the residual Ky alpha = r
    r = f["y"] - (f["mX"] if f["mX"] is not None else 0.0)
    res_hip = np.linalg.norm(Ky @ alpha - r) / (np.linalg.norm(Ky) * np.linalg.norm(alpha))
    res_orc = np.linalg.norm(Ky @ f["alpha"] - r) / (np.linalg.norm(Ky) * np.linalg.norm(f["alpha"]))
    assert res_hip < max(1e-15, 20 * res_orc), (res_hip, res_orc)
    assert_parity(alpha, f["alpha"], f["alpha_truth"], "alpha", rtol=1e-5, slack=20.0)


def test_predict_matches_oracle(hip, golden):
    f = golden
    m = make_model(hip, f)
    mean, var = m.predict(f["Xs"])
    assert mean.shape == var.shape == (f["Xs"].shape[0], 1)
    scale = np.max(np.abs(f["y"]))
    # mean: relative to the data scale (means cross zero)
    assert_parity(mean + 3 * scale, f["mean"] + 3 * scale, f["mean_truth"] + 3 * scale, f"mean[{f['name']}]")
    assert_parity(var, f["var"], f["var_truth"], f"var[{f['name']}]")
    mean0, var0 = m.predict_noiseless(f["Xs"])
    assert np.array_equal(mean0, mean)
    assert np.allclose(var0 + float(f["noise_var"]), var, rtol=1e-15, atol=0)


def test_acquisition_sweep_matches_oracle(hip, golden):
    f = golden
    from cbo_with_oop_amd import CausalExpectedImprovement
    m = make_model(hip, f)
    ei = CausalExpectedImprovement(float(f["y_best"]), f["task"], m)
    res = ei.sweep(f["Xs"], cost=float(f["cost"]), want_acq=True, want_posterior=True)
    assert res["best_idx"] == int(f["best_idx"]), (res["best_idx"], int(f["best_idx"]), f["name"])
    acq = res["acq"]
    assert acq[res["best_idx"], 0] == res["best_val"] or (res["best_val"] == 0 and acq[res["best_idx"], 0] == 0)
    assert int(np.argmax(acq[:, 0])) == res["best_idx"]                     # device arg-max == numpy's on its own output
    # EI inherits the posterior's error amplified by |u| when s is tiny; compare where EI is not negligible
    big = np.abs(f["acq"][:, 0]) > 1e-6 * np.max(np.abs(f["acq"]))
    ei_truth = O.expected_improvement(f["mean_truth"], f["var_truth"], float(f["y_best"]), f["task"]) / float(f["cost"])
    assert_parity(acq[big], f["acq"][big], ei_truth[big], f"acq[{f['name']}]", rtol=1e-5, slack=8.0)
    assert np.isclose(res["best_val"], float(f["best_val"]), rtol=1e-5 + 8 * np.max(
        np.abs(f["acq"][big] - ei_truth[big]) / np.abs(ei_truth[big])), atol=1e-300)
    # evaluate() is the reference's method name: EI without the cost
    assert np.allclose(ei.evaluate(f["Xs"]) / float(f["cost"]), acq, rtol=1e-14, atol=0)


def test_set_data_refits(hip):
    f, g = load_fixture("toy_bo_d2"), load_fixture("toy_init_Z")
    m = make_model(hip, f)
    m2 = make_model(hip, load_fixture("complete_bo_d3"))      # different n and d on the same context
    sub = slice(0, 13)
    m.set_data(f["X"][sub], f["y"][sub])
    post = O.fit(f["X"][sub], f["y"][sub])
    mu, var = O.predict(post, f["Xs"])
    mean, v = m.predict(f["Xs"])
    assert np.allclose(mean, mu, rtol=1e-7, atol=1e-9) and np.allclose(v, var, rtol=1e-6)
    assert m.X.shape == (13, 2) and m.Y.shape == (13, 1)
    del m2


def test_not_positive_definite_raises(hip):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X = np.array([[0.0], [0.0], [1.0]])
    y = np.zeros((3, 1))
    with pytest.raises(np.linalg.LinAlgError, match="non-positive diagonal"):
        HipGaussianProcess(X, y, noise_var=-2.0)
    # indefinite with positive diagonal: five jitters of ~1e-6..1e-2 cannot repair a -0.5 shift
    with pytest.raises(np.linalg.LinAlgError, match="even with jitter"):
        HipGaussianProcess(X, y, noise_var=-0.5)
    with pytest.raises(np.linalg.LinAlgError):
        O.fit(X, y, noise_var=-0.5)


def test_find_next_y_point_and_selection_on_toy(hip):
    """BASELINE config 1 flow on the toy graph's two exploration sets: per-set sweep -> cross-set choice,
    against the oracle run on the same deterministic 200-point grids."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    fx, fz = load_fixture("toy_init_X"), load_fixture("toy_init_Z")
    es = ToyGraph.get_exploration_set("MIS")
    costs = ToyGraph.get_cost_structure(1)
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, costs, "min", [fx["X"], fz["X"]],
                              [fx["y"], fz["y"]], [ToyGraph.bounds(s) for s in es], grid_shapes=[[200], [200]])
    path.update_all_gaussian_processes()
    cur = {"X": [np.inf, float(fx["y"].min())], "Z": [np.inf, float(fz["y"].min())]}
    best = path.current_best_solution(cur)
    assert best == float(fz["y_best"])
    xs, ys = path.compute_best_acquisition_values(best)
    for s, f in enumerate((fx, fz)):
        assert xs[s].shape == (1, 1) and ys[s].shape == (1, 1)
        assert np.array_equal(xs[s][0], f["Xs"][int(f["best_idx"])])
        assert np.isclose(ys[s][0, 0], float(f["best_val"]), rtol=1e-5)
    chosen, idx = path.select_next_intervention(ys)
    assert idx == O.select_next_intervention([fx["best_val"], fz["best_val"]]) and chosen == es[idx]
    # refit only the chosen set after adding the new point (CBO.py:224-235 + Monitor.add_intervention_data)
    x_new = xs[idx]
    y_new = ToyGraph.target_do_z(x_new) if es[idx] == ["Z"] else ToyGraph.target_do_x(x_new)
    path.data_x[idx] = np.vstack([path.data_x[idx], x_new])
    path.data_y[idx] = np.vstack([path.data_y[idx], y_new])
    path.update_gaussian_process_of_last_intervention()
    post = O.fit(path.data_x[idx], path.data_y[idx])
    mu, var = O.predict(post, (fz if idx == 1 else fx)["Xs"])
    mean, v = path.models[idx].predict((fz if idx == 1 else fx)["Xs"])
    assert np.allclose(mean, mu, rtol=1e-5, atol=1e-7)


def test_variable_cost_reevaluation(hip):
    """type_cost 3: the batch cost sums |x| over the whole grid, the returned y uses the single point's
    cost (utils.py:36) -- reference quirk kept."""
    from cbo_with_oop_amd import GaussianProcessFactory, GaussianProcessType, find_next_y_point
    from cbo_with_oop_amd.graphs import CompleteGraph, meshgrid_candidates
    f = load_fixture("complete_bo_d3")
    es = ["B", "E", "D"]
    costs = CompleteGraph.get_cost_structure(3)
    m = GaussianProcessFactory.create(GaussianProcessType.NON_CAUSAL_GP, f["X"], f["y"], None, emukit_wrapper=True)
    y, x = find_next_y_point(None, m, float(f["y_best"]), es, costs, candidates=f["Xs"])
    post = O.fit(f["X"], f["y"])
    batch_cost = O.cost_of_batch(f["Xs"], [10, 20, 5], [True] * 3)
    acq, _, idx, _, _ = O.acquisition_sweep(post, f["Xs"], float(f["y_best"]), cost=batch_cost)
    assert np.array_equal(x[0], f["Xs"][idx])
    ei1, _, _, _, _ = O.acquisition_sweep(post, x, float(f["y_best"]), cost=O.cost_of_batch(x, [10, 20, 5], [True] * 3))
    assert np.isclose(y[0, 0], ei1[0, 0], rtol=1e-5)


def test_chunked_sweep_equals_unchunked(hip, monkeypatch):
    """Force a tiny V workspace so the candidate loop runs many chunks."""
    from cbo_with_oop_amd import _lib, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("coral_max_d3")
    m = make_model(hip, f)
    ref = CausalExpectedImprovement(float(f["y_best"]), "min", m).sweep(f["Xs"], cost=1.0, want_acq=True)
    monkeypatch.setenv("CBO_HIP_WORKSPACE_MB", "1")          # 1 MiB / (256 rows * 8 B) = 512 columns per chunk
    ctx2 = _lib.Context(0)
    m2 = HipGaussianProcess(f["X"], f["y"], context=ctx2)
    res = CausalExpectedImprovement(float(f["y_best"]), "min", m2).sweep(f["Xs"], cost=1.0, want_acq=True)
    assert res["best_idx"] == ref["best_idx"] and np.array_equal(res["acq"], ref["acq"])


# ---------------------------------------------------------------------------------- full size (C2)
def c2_problem(n=4096, grid=(32, 32, 16), seed=0):
    """BASELINE config 2: toy_graph-style box, d=3, N obs, regular candidate grid."""
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    box = [(-5.0, 5.0), (-5.0, 20.0), (-5.0, 5.0)]
    lo, hi = np.array([b[0] for b in box]), np.array([b[1] for b in box])
    X = np.random.default_rng(seed).uniform(lo, hi, (n, 3))
    y = (np.cos(np.exp(-X[:, 0] / 3)) - np.exp(-X[:, 1] / 20) + 0.3 * np.sin(X[:, 2])
         + 0.1 * np.random.default_rng(seed + 1).standard_normal(n))[:, None]
    return X, y, meshgrid_candidates(box, grid)


def test_full_size_c2_against_oracle(hip):
    """N=4096, M=16384, d=3, fp64: the whole sweep against the oracle (takes ~10-20 s of CPU)."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X, y, Xs = c2_problem()
    m = HipGaussianProcess(X, y)
    res = CausalExpectedImprovement(float(y.min()), "min", m).sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
    post = O.fit(X, y)
    acq, best_val, best_idx, mu, var = O.acquisition_sweep(post, Xs, float(y.min()), cost=3.0)
    assert m.jitter_tries == post.tries
    assert res["best_idx"] == best_idx
    assert np.max(np.abs(res["var"] - var) / var) < 1e-5
    assert np.max(np.abs(res["mean"] - mu)) < 1e-5 * np.max(np.abs(y))
    big = acq[:, 0] > 1e-6 * acq.max()
    assert np.max(np.abs(res["acq"][big] - acq[big]) / acq[big]) < 1e-4
    assert np.isclose(res["best_val"], best_val, rtol=1e-5)


def test_full_size_properties(hip):
    """Size-independent properties at N=4096 x M=16384 (no oracle involved)."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X, y, Xs = c2_problem(seed=3)
    m = HipGaussianProcess(X, y)
    ei = CausalExpectedImprovement(float(y.min()), "min", m)
    full = ei.sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
    # (1) interpolation: at the training inputs the posterior mean returns y to O(noise) and the
    #     variance collapses to O(diag) -- exercises K*, TRSM and epilogue with M = N
    mean_tr, var_tr = m.predict(X[:1024])
    _, alpha = m.posterior_state()
    # K alpha = y - (noise + 1e-8) alpha exactly, so the interpolation residual is 1.01e-8 * alpha
    assert np.allclose(mean_tr - y[:1024], -1.01e-8 * alpha[:1024], rtol=1e-3, atol=1e-9)
    assert np.max(var_tr) < 1e-6
    # (2) shard invariance: the global winner of 4 contiguous shards (index offsets) equals the unsharded one,
    #     and per-candidate results do not depend on which strip/chunk a candidate lands in
    from cbo_with_oop_amd.sharding import reduce_pairs, shard_bounds
    vals, idxs = [], []
    for r in range(4):
        b, e = shard_bounds(Xs.shape[0], 4, r)
        g = CandidateGrid(Xs[b:e], m, index_offset=b)
        res = ei.sweep(g, cost=3.0, want_acq=True)
        assert np.array_equal(res["acq"], full["acq"][b:e])
        vals.append(res["best_val"]); idxs.append(res["best_idx"])
    assert reduce_pairs(vals, idxs) == (full["best_val"], full["best_idx"])
    # (3) permutation of candidates permutes the outputs
    perm = np.random.default_rng(5).permutation(Xs.shape[0])
    p = ei.sweep(Xs[perm], cost=3.0, want_acq=True)
    assert np.array_equal(p["acq"], full["acq"][perm]) and perm[p["best_idx"]] == full["best_idx"]
    # (4) linearity of the posterior mean in y, variance independent of y
    y2 = np.sin(X[:, :1] * X[:, 1:2] / 10)
    ma, va = HipGaussianProcess(X, y2).predict(Xs[::16])
    mb, vb = HipGaussianProcess(X, y + y2).predict(Xs[::16])
    assert np.allclose(full["mean"][::16] + ma, mb, rtol=0, atol=1e-7 * np.max(np.abs(y)))
    assert np.array_equal(va, vb) and np.array_equal(va, full["var"][::16])
    # (5) variances are within [noise, prior]
    assert full["var"].min() >= 1e-10 and full["var"].max() <= 1.0 + 1e-10 + 1e-12
    # (6) refit + sweep as ONE overlapped call (what bench.py times) against the two calls above, full size:
    #     bit-identical (same operations per element, q and mu summed pair-wise in both schedules)
    fused = ei.sweep(Xs, cost=3.0, want_acq=True, want_posterior=True, refit=True)
    assert fused["best_idx"] == full["best_idx"] and fused["best_val"] == full["best_val"]
    for key in ("mean", "var", "acq"):
        assert np.array_equal(fused[key], full[key]), key
    if not any(os.environ.get(k) for k in ("CBO_HIP_OVERLAP", "CBO_HIP_PIPE_TAIL", "CBO_HIP_PIPE_GROUP")):
        from cbo_with_oop_amd import _lib
        assert last_schedule(_lib.Context.get(), 4096, 16384)[0] >= 0      # it WAS an overlapped call (-1: fit, then sweep)


# ---------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (2, 3, 2), (63, 65, 3), (64, 64, 1), (127, 129, 5), (128, 1, 8),
                                   (129, 200, 7), (300, 1000, 4)])
def test_ragged_sizes_and_dims(hip, n, m, d):
    """Sizes around the 64/128 padding boundaries, single points, every input dimension up to CBO_MAX_DIM."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(100 * n + m + d)
    X = rng.uniform(-3, 3, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.01 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-3, 3, (m, d))
    g = HipGaussianProcess(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-4)
    mean, var = g.predict(Xs)
    post = O.fit(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-4)
    mu, v = O.predict(post, Xs)
    assert np.allclose(mean, mu, rtol=1e-7, atol=1e-9) and np.allclose(var, v, rtol=1e-6)
    L, alpha = g.posterior_state()
    assert np.allclose(L, post.L, rtol=1e-9, atol=1e-12) and np.allclose(alpha, post.alpha, rtol=1e-6, atol=1e-9)


def test_argmax_ties_and_nan_like_numpy(hip):
    """Lowest index wins exact ties (candidates duplicated); a NaN score is maximal, as numpy.argmax has it."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("toy_bo_d2")
    m = make_model(hip, f)
    Xs = np.vstack([f["Xs"], f["Xs"], f["Xs"][::-1]])            # every candidate appears three times
    res = CausalExpectedImprovement(float(f["y_best"]), "min", m).sweep(Xs, cost=1.0, want_acq=True)
    assert res["best_idx"] == int(np.argmax(res["acq"][:, 0])) == int(f["best_idx"])
    # NaN: a causal model whose prior variance is negative at one candidate (sqrt -> NaN in CausalRBF.K)
    c = load_fixture("causal_d2")
    bad = 17
    vXs = c["vXs"].copy()
    vXs[bad] = -1.0
    lut = lambda tab_x, tab_v: {tuple(r): v for r, v in zip(map(tuple, tab_x), tab_v[:, 0])}
    lm = {**lut(c["X"], c["mX"]), **lut(c["Xs"], c["mXs"])}
    lv = {**lut(c["X"], c["vX"]), **lut(c["Xs"], vXs)}
    g = HipGaussianProcess(c["X"], c["y"], mean_function=lambda a: np.array([[lm[tuple(r)]] for r in a]),
                           variance_adjustment=lambda a: np.array([[lv[tuple(r)]] for r in a]))
    with np.errstate(invalid="ignore"):
        res = CausalExpectedImprovement(float(c["y_best"]), "min", g).sweep(c["Xs"], cost=1.0, want_acq=True)
        post = O.fit(c["X"], c["y"], c["mX"], c["vX"])
        acq, _, idx, _, _ = O.acquisition_sweep(post, c["Xs"], float(c["y_best"]), c["mXs"], vXs)
    assert np.isnan(acq[bad, 0]) and idx == bad
    assert np.isnan(res["acq"][bad, 0]) and res["best_idx"] == bad and np.isnan(res["best_val"])


def test_expected_improvement_over_the_whole_range_of_u(hip):
    """The EI arithmetic of the epilogue alone (cbo_device.h: square root and quotient from one reciprocal-root estimate, lean
    exponential, cephes ndtr in its three ranges, VOP3 selects) against scipy on the DEVICE's own mean and variance: the
    incumbent is moved so that u = (y_best - mean) / s sweeps -39 .. +39 over the candidates -- below sqrt(1/2) (erf), up to 1
    (1 - erf), the middle and the far rational functions of erfc, the underflow beyond 37.5 -- for both tasks.  u Phi(u) +
    phi(u) cancels in the lower tail (both terms ~ phi, the sum ~ phi / u^2), so the bound is on the TERMS: a few ulp times
    (1 + u^2) of s (|u| Phi + phi), for the device as for scipy."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    f = load_fixture("toy_bo_d2")
    m = make_model(hip, f)
    Xs = f["Xs"]
    base = CausalExpectedImprovement(float(f["y_best"]), "min", m).sweep(Xs, cost=1.0, want_acq=True, want_posterior=True)
    mean, var = base["mean"][:, 0], base["var"][:, 0]
    s = np.sqrt(var)
    eps = np.finfo(float).eps
    seen = set()
    for task in ("min", "max"):
        for shift in (-39.0, -20.0, -12.0, -8.0, -3.0, -1.2, -0.5, 0.0, 0.5, 1.2, 3.0, 8.0, 12.0, 20.0, 39.0):
            y_best = float(np.median(mean) + shift * np.median(s))
            res = CausalExpectedImprovement(y_best, task, m).sweep(Xs, cost=1.0, want_acq=True)
            acq = res["acq"][:, 0]
            ref = O.expected_improvement(mean, var, y_best, task)
            u = (y_best - mean) / s
            import scipy.stats
            terms = s * (np.abs(u) * scipy.stats.norm.cdf(u) + scipy.stats.norm.pdf(u))
            bound = 48 * eps * (1.0 + u * u) * terms + 1e-300
            assert np.all(np.abs(acq - ref) <= bound), (task, shift, float(np.max(np.abs(acq - ref) / bound)))
            # the winner: the device's arg-max of its own values, and among the oracle's best within the bound
            assert res["best_idx"] == int(np.argmax(acq)) and ref[res["best_idx"]] >= ref.max() - 2 * bound[res["best_idx"]]
            z = np.abs(u) * np.sqrt(0.5)
            seen |= {k for k, hit in (("centre", (z < np.sqrt(0.5)).any()), ("below 1", ((z >= np.sqrt(0.5)) & (z < 1)).any()),
                                      ("middle", ((z >= 1) & (z < 8)).any()), ("far", ((z >= 8) & (z * z <= 709.78)).any()),
                                      ("underflow", (z * z > 709.78).any())) if hit}
    assert seen == {"centre", "below 1", "middle", "far", "underflow"}, seen


def test_c3_size_against_oracle_subsample(hip):
    """BASELINE config 3 shape per GPU: N=8192 observations, a 32768-candidate shard (64x32x16 of the 64x32x32
    grid), complete-graph box.  The oracle checks a 512-candidate subsample (full sweep = minutes of CPU)."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph, meshgrid_candidates
    box = CompleteGraph.bounds(["B", "D", "E"])
    lo, hi = np.array([b[0] for b in box], float), np.array([b[1] for b in box], float)
    rng = np.random.default_rng(8192)
    X = rng.uniform(lo, hi, (8192, 3))
    y = (np.sin(X[:, 0]) * np.cos(X[:, 1] / 2) + 0.2 * X[:, 2] + 0.1 * rng.standard_normal(8192))[:, None]
    Xs = meshgrid_candidates(box, [64, 32, 32])[:32768]
    m = HipGaussianProcess(X, y)
    res = CausalExpectedImprovement(float(y.min()), "min", m).sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
    post = O.fit(X, y)
    assert m.jitter_tries == post.tries
    sub = np.unique(np.concatenate([np.arange(0, 32768, 67), [res["best_idx"]]]))
    mu, var = O.predict(post, Xs[sub])
    assert np.max(np.abs(res["var"][sub] - var) / var) < 1e-5
    assert np.max(np.abs(res["mean"][sub] - mu)) < 1e-5 * np.max(np.abs(y))
    acq = O.expected_improvement(mu, var, float(y.min())) / 3.0
    big = acq[:, 0] > 1e-6 * acq.max()
    assert np.max(np.abs(res["acq"][sub][big] - acq[big]) / acq[big]) < 1e-4
    assert int(np.argmax(res["acq"][:, 0])) == res["best_idx"]


def test_c3_bench_problem_against_the_oracle(hip):
    """BASELINE config 3 on the data ``bench.py --config c3`` benches (``bench.make_problem``: complete_graph (B, D, E)
    ranges, 8192 observations, the fixed 64x32x32 grid), one GPU: the one call the bench times, against the oracle on a
    512-candidate subsample plus the device's 64 best candidates -- variance and mean at the plain 1e-5, acquisition 1e-4
    where it is not negligible, the oracle's best of those candidates = the device's arg-max."""
    import bench
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X, y, Xs, grid, note = bench.make_problem(bench.CONFIGS["c3"], 1, "strong", False)
    assert X.shape == (8192, 3) and Xs.shape == (65536, 3) and tuple(grid) == (64, 32, 32)
    y_best, cost = float(y.min()), 3.0
    m = HipGaussianProcess(X, y, fit=False)                        # unfitted: the sweep below is the bench's one call
    res = CausalExpectedImprovement(y_best, "min", m).sweep(Xs, cost=cost, want_acq=True, want_posterior=True, refit=True)
    assert not m.stale and int(np.argmax(res["acq"][:, 0])) == res["best_idx"]
    post = O.fit(X, y)
    assert m.jitter_tries == post.tries
    top64 = np.argsort(-res["acq"][:, 0], kind="stable")[:64]
    sub = np.unique(np.concatenate([np.arange(0, 65536, 128), top64]))
    acq, _, _, mu, var = O.acquisition_sweep(post, Xs[sub], y_best, cost=cost)
    assert np.max(np.abs(res["var"][sub] - var) / var) < 1e-5
    assert np.max(np.abs(res["mean"][sub] - mu)) < 1e-5 * np.max(np.abs(y))
    big = acq[:, 0] > 1e-6 * acq.max()
    assert big.sum() >= 32                                         # (the top 64 are in: the column is not a comparison of zeros)
    # the improvement moves one for one with the mean (d EI / d mean = -Phi(u)): it inherits the mean's ABSOLUTE tolerance,
    # 1e-5 max|y| (/ cost), next to 1e-4 of its own value (measured: 5.6e-7 absolute on a value of 0.028, max 4.3)
    err = np.abs(res["acq"][sub][big] - acq[big])
    assert np.all(err <= 1e-4 * acq[big] + 1e-5 * np.max(np.abs(y)) / cost), float(np.max(err / acq[big]))
    assert np.max(err[acq[big] > 0.1 * acq.max()] / acq[big][acq[big] > 0.1 * acq.max()]) < 1e-5     # the candidates that matter
    assert int(sub[np.argmax(acq[:, 0])]) == res["best_idx"]
    m.close()


# ---------------------------------------------------------------------------------- do-calculus prior (f1)
def test_do_calculus_prior_matches_oracle(hip):
    """Graph-level GP (ARD RBF, noise 1e-2) -> do-calculus mean/variance closures -> causal GP -> sweep,
    against the oracle's row-by-row restatement of src/DoCalculus.py:34-89."""
    import warnings
    from cbo_with_oop_amd import (CausalExpectedImprovement, DoCalculus, GaussianProcessFactory, GaussianProcessType,
                                  do_prior_functions)
    from cbo_with_oop_amd.utils_functions import fit_gaussian_process
    rng = np.random.default_rng(77)
    n_obs = 120
    obs = {"B": rng.uniform(-5, 4, (n_obs, 1)), "D": rng.uniform(-5, 5, (n_obs, 1)), "C": rng.normal(0, 1, (n_obs, 1))}
    yobs = np.sin(obs["B"]) + 0.3 * obs["D"] ** 2 / 5 + 0.5 * obs["C"] + 0.05 * rng.standard_normal((n_obs, 1))
    deps = ["B", "D", "C"]                                  # graph GP inputs; we intervene on (B, D), C stays observed
    params = [np.array([1.2, 0.8, 1.5]), 1.4, 1e-2, True]   # [lengthscales, variance, noise, ARD]
    xin = np.hstack([obs[v] for v in deps])
    ggp = fit_gaussian_process(xin, yobs, params)           # includes gp.optimize() as in the reference
    assert ggp.noise_var == 1e-2 and ggp.fix_noise
    gpost = O.fit(xin, yobs, variance=ggp.variance, lengthscale=ggp.lengthscale, noise_var=1e-2)
    mean_fn, var_fn = do_prior_functions(ggp, xin, [0, 1, -1])
    vals = rng.uniform([-5, -5], [4, 5], (37, 2))
    m_ref = O.do_prior(gpost, xin, [0, 1, -1], vals, 0)
    v_ref = O.do_prior(gpost, xin, [0, 1, -1], vals, 1)
    assert np.allclose(mean_fn(vals), m_ref, rtol=1e-8, atol=1e-10) and mean_fn(vals).shape == (37, 1)
    assert np.allclose(var_fn(vals), v_ref, rtol=1e-7)

    # the reference-shaped class gives the same closures
    class G:
        fit_dependencies = [deps]
        @staticmethod
        def get_gp_name(iv): return "gp_" + "_".join(iv)
    class C:
        exploration_set = [["B", "D"]]; es_size = 1; measurements = obs; graph = G()
    fns = DoCalculus(C()).update_all_do_functions({"gp_B_D": ggp})
    assert np.array_equal(fns[0][0](vals), mean_fn(vals)) and np.array_equal(fns[1][0](vals), var_fn(vals))

    # causal GP on interventional data with that prior, 400-candidate sweep
    Xi = rng.uniform([-5, -5], [4, 5], (25, 2))
    yi = np.sin(Xi[:, :1]) + 0.3 * Xi[:, 1:] ** 2 / 5 + 0.02 * rng.standard_normal((25, 1))
    model = GaussianProcessFactory.create(GaussianProcessType.CAUSAL_GP, Xi, yi, [mean_fn, var_fn], emukit_wrapper=True)
    Xs = rng.uniform([-5, -5], [4, 5], (400, 2))
    res = CausalExpectedImprovement(float(yi.min()), "min", model).sweep(Xs, cost=2.0, want_acq=True, want_posterior=True)
    pm = lambda a: O.do_prior(gpost, xin, [0, 1, -1], a, 0)
    pv = lambda a: O.do_prior(gpost, xin, [0, 1, -1], a, 1)
    post = O.fit(Xi, yi, pm(Xi), pv(Xi))
    acq, bval, bidx, mu, var = O.acquisition_sweep(post, Xs, float(yi.min()), pm(Xs), pv(Xs), cost=2.0)
    assert res["best_idx"] == bidx
    assert np.allclose(res["mean"], mu, rtol=1e-6, atol=1e-8) and np.allclose(res["var"], var, rtol=1e-5)


# ---------------------------------------------------------------------------------- hyper-parameter MLE (f2)
def test_log_marginal_likelihood_matches_oracle(hip, golden):
    f = golden
    m = make_model(hip, f)
    post = O.fit(f["X"], f["y"], f["mX"], f["vX"], float(f["variance"]), f["lengthscale_arg"], float(f["noise_var"]))
    ref = O.log_marginal_likelihood(post)
    # r^T Ky^-1 r carries the eps*cond(Ky) error of any fp64 solve; logdet is benign
    tol = 1e-9 + 50 * np.max(np.abs(f["alpha"][:, 0] - f["alpha_truth"]) / np.abs(f["alpha_truth"]).clip(1e-300))
    assert np.isclose(m.log_likelihood(), ref, rtol=tol), (m.log_likelihood(), ref, golden["name"])


def test_optimize_reaches_the_oracle_optimum(hip):
    """model.optimize() (src/CBO.py:173): same objective and optimiser call on both sides."""
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory, GaussianProcessType
    rng = np.random.default_rng(5)
    X = rng.uniform(-4, 4, (60, 2))
    y = np.sin(1.3 * X[:, :1]) * np.cos(0.7 * X[:, 1:]) + 0.05 * rng.standard_normal((60, 1))
    m = GaussianProcessFactory.create(GaussianProcessType.NON_CAUSAL_GP, X, y, None, emukit_wrapper=True)
    l0 = m.log_likelihood()
    res = m.optimize()                       # paramz's call: L-BFGS-B on the Logexp-transformed parameters (the default)
    info = {}
    v, ls, nz, lml = O.optimize_hyperparameters(X, y, info=info)
    assert res.transform == "logexp" and res.success and info["warnflag"] == 0
    assert abs(res.nfev - info["funcalls"]) <= 5, (res.nfev, info)       # the same path to rounding of the gradients
    assert m.log_likelihood() > l0 + 1.0
    assert np.isclose(m.log_likelihood(), lml, rtol=1e-5, atol=1e-4)
    assert np.isclose(m.variance, v, rtol=2e-2) and np.allclose(m.lengthscale, ls, rtol=2e-2)
    mean, var = m.predict(X[:5])
    mu, vv = O.predict(O.fit(X, y, variance=m.variance, lengthscale=float(m.lengthscale[0]), noise_var=m.noise_var), X[:5])
    assert np.allclose(mean, mu, rtol=1e-6, atol=1e-8) and np.allclose(var, vv, rtol=1e-5)
    # rounds 1-4's parametrisation (theta = exp x) stays selectable: same stationary point
    m2 = GaussianProcessFactory.create(GaussianProcessType.NON_CAUSAL_GP, X, y, None, emukit_wrapper=True)
    assert m2.optimize(transform="log").transform == "log"
    v2, ls2, nz2, lml2 = O.optimize_hyperparameters(X, y, transform="log")
    assert np.isclose(m2.log_likelihood(), lml2, rtol=1e-5, atol=1e-4) and np.isclose(m2.log_likelihood(), lml, rtol=1e-5, atol=1e-4)
    assert np.isclose(m2.variance, v2, rtol=2e-2) and np.allclose(m2.lengthscale, ls2, rtol=2e-2)
    # graph-level GP: ARD lengthscales, noise fixed at 1e-2 (src/utils_functions/utils.py:40-45)
    Xg = rng.uniform(-2, 2, (80, 3))
    yg = (np.cos(Xg[:, 0]) + 0.5 * Xg[:, 1])[:, None] + 0.1 * rng.standard_normal((80, 1))
    g = GaussianProcessFactory.create(GaussianProcessType.GRAPH_GP, Xg, yg, [1.0, 1.0, 1e-2, True])
    g.optimize()
    v, ls, nz, lml = O.optimize_hyperparameters(Xg, yg, variance=1.0, lengthscale=np.ones(3), noise_var=1e-2,
                                                fix_noise=True)
    assert g.noise_var == 1e-2 and nz == 1e-2
    assert np.isclose(g.log_likelihood(), lml, rtol=1e-5, atol=1e-4)
    assert ls[2] > 3 * ls[0] and g.lengthscale[2] > 3 * g.lengthscale[0]      # the irrelevant input is switched off


# ---------------------------------------------------------------------------------- trajectories
def _toy_trajectory(fit_predict_sweep, n_trials=12):
    """The reference's intervene() loop on the toy graph (src/CBO.py:143-173 without the monitor): refit the
    GP(s), score each exploration set on its 200-point grid, pick the set (first max), evaluate the SEM target
    there, append the point.  `fit_predict_sweep(X, y, Xs, y_best)` -> (best_val, best_idx)."""
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    fx, fz = load_fixture("toy_init_X"), load_fixture("toy_init_Z")
    data_x, data_y = [fx["X"].copy(), fz["X"].copy()], [fx["y"].copy(), fz["y"].copy()]
    grids = [meshgrid_candidates(ToyGraph.bounds(["X"]), [200]), meshgrid_candidates(ToyGraph.bounds(["Z"]), [200])]
    target = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    best_y = {"X": [np.inf, float(data_y[0].min())], "Z": [np.inf, float(data_y[1].min())]}
    history = []
    for _ in range(n_trials):
        y_star = O.find_current_global(best_y, ["X", "Z"], "min")
        scores = [fit_predict_sweep(data_x[s], data_y[s], grids[s], y_star) for s in range(2)]
        s = O.select_next_intervention([np.array([[v]]) for v, _ in scores])
        idx = scores[s][1]
        x_new = grids[s][idx][None, :]
        y_new = target[s](x_new)
        data_x[s] = np.vstack([data_x[s], x_new])
        data_y[s] = np.vstack([data_y[s], y_new])
        best_y["XZ"[s]].append(float(y_new[0, 0]))
        history.append((s, idx, scores[s][0]))
    return history


def test_toy_graph_intervention_trajectory_matches_oracle(hip):
    """'identical intervention choices to the reference on toy_graph' (BASELINE.json north_star), trial after
    trial, against the oracle run through the same loop (the reference itself cannot run toy_graph)."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory, GaussianProcessType

    def hip_side(X, y, Xs, y_star):
        m = GaussianProcessFactory.create(GaussianProcessType.NON_CAUSAL_GP, X, y, None, emukit_wrapper=True)
        r = CausalExpectedImprovement(y_star, "min", m).sweep(Xs, cost=1.0)
        return r["best_val"], r["best_idx"]

    def oracle_side(X, y, Xs, y_star):
        _, val, idx, _, _ = O.acquisition_sweep(O.fit(X, y), Xs, y_star, cost=1.0)
        return val, idx

    h, o = _toy_trajectory(hip_side), _toy_trajectory(oracle_side)
    assert [(s, i) for s, i, _ in h] == [(s, i) for s, i, _ in o], (h, o)
    assert np.allclose([v for _, _, v in h], [v for _, _, v in o], rtol=1e-4)
    assert len({s for s, _, _ in h}) >= 1


def test_c4_size_chunked_workspace(hip, monkeypatch):
    """BASELINE config 4 shape per GPU: N=16384 observations, 32768 candidates (one 8th of the 64^3 grid), coral
    box -- with a 4 GiB cap the V workspace (4.3 GB) is processed in two chunks; with the default cap it is one
    chunk and the overlapped refit + sweep applies.  The oracle checks a 128-candidate subsample (fp64 dpotrf
    of a 16384^2 matrix on the host, ~0.5 min)."""
    from cbo_with_oop_amd import CausalExpectedImprovement, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CoralGraph, meshgrid_candidates
    box = CoralGraph.bounds(["N", "O", "C"])     # (the ranges this test has used since round 1)
    lo, hi = np.array([b[0] for b in box], float), np.array([b[1] for b in box], float)
    rng = np.random.default_rng(16384)
    X = rng.uniform(lo, hi, (16384, 3))
    y = (np.sin(X[:, 0]) + np.cos(3 * X[:, 1]) * X[:, 2] + 0.1 * rng.standard_normal(16384))[:, None]
    Xs = meshgrid_candidates(box, [64, 64, 64])[:32768]
    monkeypatch.setenv("CBO_HIP_WORKSPACE_MB", "4096")
    capped = _lib.Context(0)
    monkeypatch.delenv("CBO_HIP_WORKSPACE_MB")
    m = HipGaussianProcess(X, y, context=capped)
    res = CausalExpectedImprovement(float(y.min()), "min", m).sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
    assert int(np.argmax(res["acq"][:, 0])) == res["best_idx"]
    # one chunk on the default context, refit and sweep overlapped (64 panel pairs)
    m1 = HipGaussianProcess(X, y, fit=False)
    one = CausalExpectedImprovement(float(y.min()), "min", m1).sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
    assert not m1.stale and one["best_idx"] == res["best_idx"]
    assert np.array_equal(one["var"], res["var"]) and np.array_equal(one["mean"], res["mean"])
    m1.close()
    post = O.fit(X, y)
    assert m.jitter_tries == post.tries
    sub = np.unique(np.concatenate([np.arange(0, 32768, 257), [res["best_idx"]]]))
    mu, var = O.predict(post, Xs[sub])
    # 16384 observations in this small box leave posterior variances of 1e-10..1e-7: var = kss - q with
    # q = kss (1 - 1e-9) is a cancellation that no fp64 evaluation resolves to 1e-5 (both sides carry
    # ~N eps kss = 1e-14 absolute); hence rtol 1e-5 plus that absolute floor
    assert np.all(np.abs(res["var"][sub] - var) <= 1e-5 * var + 1e-13)
    assert np.max(np.abs(res["mean"][sub] - mu)) < 1e-5 * np.max(np.abs(y))
    m.close()
    capped.close()


def test_c4_bench_problem_against_oracle_and_arbiter(hip):
    """BASELINE config 4 ON THE DATA bench.py --config c4 TIMES (bench.make_problem(CONFIGS["c4"]): simplified_coral_graph
    (N, O, T) box, T in [2300, 2400], 16384 seeded observations, the rank's 1/8 shard = the first 32768 candidates of the 64^3
    grid), through the call the bench times (cbo_gp_fit_sweep; above 12288 rows it does not overlap).  The model is the one
    the reference builds at src/GaussianProcessFactory.py:57-60.  On this data Ky is not positive definite as assembled:
    jitchol's first retry is exercised on every fit (asserted).  The oracle (dpotrf of a 16384^2 matrix on the host, twice)
    checks a 257-candidate subsample plus the device's top candidates: mean, variance and acquisition by the arbiter rule of
    tests/conftest.py (device error <= 1e-5 + 8 x the oracle's own) with oracle/truth.py:refined_mean / refined_variance
    (exact kernel entries, iterative refinement with long-double residuals) as the arbiter --
    at T ~ 2350 GPy's |x|^2 + |x'|^2 - 2 x.x' loses 1e-9 of every entry, which jitchol's 1e-6 jitter under 16384 points
    turns into 1e-3 of the mean in oracle and device alike; identical arg-max, or a tie within 1e-12."""
    import bench
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from oracle.truth import refined_mean
    X, y, Xs, grid, note = bench.make_problem(bench.CONFIGS["c4"], 1, "strong", False)
    assert X.shape == (16384, 3) and Xs.shape == (32768, 3) and 2300.0 <= X[:, 2].min() and X[:, 2].max() <= 2400.0
    y_best, cost = float(y.min()), 3.0
    m = HipGaussianProcess(X, y, fit=False)                        # unfitted: the sweep below is the bench's one call
    res = CausalExpectedImprovement(y_best, "min", m).sweep(Xs, cost=cost, want_acq=True, want_posterior=True, refit=True)
    assert not m.stale and int(np.argmax(res["acq"][:, 0])) == res["best_idx"]
    if not any(os.environ.get(k) for k in ("CBO_HIP_OVERLAP", "CBO_HIP_PIPE_TAIL", "CBO_HIP_PIPE_GROUP")):
        from cbo_with_oop_amd import _lib
        assert last_schedule(_lib.Context.get(), 16384, 32768)[0] >= 0     # an overlapped call, its pipeline repeated by the retry
    post = O.fit(X, y)
    assert m.jitter_tries == post.tries and post.tries >= 1, (m.jitter_tries, post.tries)      # the retry IS exercised
    assert np.isclose(m.jitter, post.jitter, rtol=1e-12, atol=0.0), (m.jitter, post.jitter)
    top = np.argsort(-res["acq"][:, 0], kind="stable")[:64]
    sub = np.unique(np.concatenate([np.arange(0, 32768, 128), top]))
    acq, _, _, mu, var = O.acquisition_sweep(post, Xs[sub], y_best, cost=cost)
    problems = []
    # Variance.  Two faithful fp64 evaluations of GPy's formula differ here by far more than 1e-5: its |x|^2 + |x'|^2 - 2 x.x'
    # carries 1e-9 of absolute error per kernel entry at T ~ 2350 (which entry gets which error depends on the order of the
    # three coordinate products), and Ky^-1 has norm 1e6 under jitchol's 1e-6 jitter.  So the variance goes by the arbiter
    # rule too: on 16 candidates (the device's winner among them) the arbiter is the exact-entry kernel solved by iterative
    # refinement in long double (oracle/truth.py:refined_variance, pinned against the 80-bit restatement in
    # tests/test_oracle.py), and the device may be off by 1e-5 relative plus 8 x the oracle's own error; on the whole
    # subsample the device stays within 1e-5 relative + 16 x that measured error of the oracle (absolute).
    from oracle.truth import refined_variance
    arb = np.unique(np.concatenate([[int(np.searchsorted(sub, res["best_idx"]))], np.linspace(0, sub.size - 1, 15).astype(int)]))
    tv = refined_variance(post, Xs[sub[arb]])
    oracle_verr = np.max(np.abs(var[arb] - tv))
    dev_verr = np.max(np.abs(res["var"][sub[arb]] - tv))
    print(f"config-4 var: |oracle - arbiter| {oracle_verr:.3e}, |device - arbiter| {dev_verr:.3e}, |device - oracle| "
          f"{np.max(np.abs(res['var'][sub] - var)):.3e}, variances {np.min(var):.2e} .. {np.max(var):.2e}")
    if np.any(np.abs(res["var"][sub[arb]] - tv) > 1e-5 * tv + 8.0 * oracle_verr):
        problems.append(f"var: |device - arbiter| {dev_verr:.3e} > 1e-5 * var + 8 * {oracle_verr:.3e}")
    bad = np.abs(res["var"][sub] - var) > 1e-5 * var + 1e-13 + 16.0 * oracle_verr
    if np.any(bad):
        problems.append(f"var vs oracle: {int(bad.sum())} of {sub.size} beyond rtol 1e-5 + 16 * {oracle_verr:.3e}, worst "
                        f"{np.max(np.abs(res['var'][sub] - var)):.3e}")
    tm, _ = refined_mean(post, Xs[sub], exact_entries=True)
    scale = np.max(np.abs(y))
    oracle_err, dev_err = np.max(np.abs(mu - tm)), np.max(np.abs(res["mean"][sub] - tm))
    print(f"config-4 mean: |oracle - arbiter| {oracle_err:.3e}, |device - arbiter| {dev_err:.3e}, |device - oracle| "
          f"{np.max(np.abs(res['mean'][sub] - mu)):.3e}, max|y| {scale:.2f}; jitter tries {post.tries}, jitter {post.jitter:.3e}")
    if dev_err > 1e-5 * scale + 8.0 * oracle_err:
        problems.append(f"mean: |device - arbiter| {dev_err:.3e} > 1e-5 * {scale:.2f} + 8 * {oracle_err:.3e}")
    amax = np.max(np.abs(res["acq"]))
    # acquisition: from the arbiter's mean and, where it exists (the 16 candidates), the arbiter's variance
    var_t = var.copy()
    var_t[arb] = tv
    acq_t = O.expected_improvement(tm, var_t, y_best, "min", 0.0) / cost
    oracle_acq_err, dev_acq_err = np.max(np.abs(acq - acq_t)), np.max(np.abs(res["acq"][sub] - acq_t))
    print(f"config-4 acq: |oracle - arbiter| {oracle_acq_err:.3e}, |device - arbiter| {dev_acq_err:.3e}, max|acq| {amax:.3e}")
    if dev_acq_err > 1e-5 * amax + 8.0 * oracle_acq_err:
        problems.append(f"acq: |device - arbiter| {dev_acq_err:.3e} > 1e-5 * {amax:.3e} + 8 * {oracle_acq_err:.3e}")
    # arg-max: the oracle's best over (subsample + the device's 64 best) is the device's winner, or ties it to 1e-12
    o_best, o_val = int(sub[np.argmax(acq[:, 0])]), float(np.max(acq[:, 0]))
    if o_best != res["best_idx"] and abs(float(acq[list(sub).index(res["best_idx"]), 0]) - o_val) > 1e-12 * abs(o_val):
        problems.append(f"oracle prefers {o_best} ({o_val:.15e}) over the device's {res['best_idx']} ({res['best_val']:.15e})")
    assert not problems, "; ".join(problems)
    m.close()


def test_bitwise_reproducibility(hip):
    """Two fits and two sweeps of the same inputs give bit-identical factors and scores (fixed reduction orders,
    no atomics; a race in the LDS-DMA pipeline or the look-ahead streams would show up here)."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X, y, Xs = c2_problem(n=1536, grid=(16, 16, 8), seed=11)
    a, b = HipGaussianProcess(X, y), HipGaussianProcess(X, y)
    La, _ = a.posterior_state()
    Lb, _ = b.posterior_state()
    assert np.array_equal(La, Lb)
    ei = CausalExpectedImprovement(float(y.min()), "min", a)
    r1 = ei.sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
    for _ in range(3):
        a.set_data(X, y)                                      # refit in place, then sweep again
        r2 = ei.sweep(Xs, cost=3.0, want_acq=True, want_posterior=True)
        assert np.array_equal(r1["acq"], r2["acq"]) and np.array_equal(r1["var"], r2["var"])
        assert np.array_equal(r1["mean"], r2["mean"]) and r1["best_idx"] == r2["best_idx"]


def test_chain_launch_forms_give_the_same_bits(hip):
    """The factorisation's chain with the diagonal block and its row panel in ONE launch (the default: workgroup 0
    publishes row tiles, the strips follow through flags with coherent loads) against the same chain as separate
    launches (CBO_HIP_PANEL_FORM=2), each in a process of its own: identical factors, inverses-derived posteriors and
    sweeps, at sizes with one, several and many panels, with and without a jitchol retry."""
    import subprocess
    import sys
    from conftest import ROOT
    code = r"""
import hashlib, sys, warnings
import numpy as np
sys.path.insert(0, %r)
from cbo_with_oop_amd import CausalExpectedImprovement
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
h = hashlib.sha256()
for n, noise in ((130, 1e-2), (700, 1e-2), (2300, 1e-3), (1500, 1e-10)):
    rng = np.random.default_rng(n)
    X = rng.uniform([-5, -5, -5], [5, 20, 5], (n, 3))
    if noise == 1e-10:
        X[1::2] = X[::2][: len(X[1::2])]                      # duplicated rows: the first attempt is not positive definite
    y = np.sin(X).sum(1, keepdims=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = HipGaussianProcess(X, y, noise_var=noise)
    L, alpha = m.posterior_state()
    r = CausalExpectedImprovement(float(y.min()), "min", m).sweep(rng.uniform(-5, 5, (300, 3)), want_acq=True, want_posterior=True)
    for a in (L, alpha, r["acq"], r["var"], r["mean"]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(str((m.jitter_tries, r["best_idx"])).encode())
    # one appended observation: the single-vector forward solve (a chain of workgroups in one launch, or per-block launches)
    x_new = rng.uniform([-5, -5, -5], [5, 20, 5], (1, 3))
    appended = m.append(x_new, np.sin(x_new).sum(1, keepdims=True))
    L2, alpha2 = m.posterior_state()
    h.update(str(appended).encode())
    h.update(np.ascontiguousarray(L2).tobytes())
    h.update(np.ascontiguousarray(alpha2).tobytes())
    m.close()
print("DIGEST", h.hexdigest())
""" % ROOT
    digests = {}
    # "timeout": every poll of a launch-internal protocol gives up at once (CBO_HIP_FUSED_SPIN_LIMIT=-1: the strips of
    # the fused diagonal + panel launches, the workgroup chains of the single-vector solves): the host repeats the
    # factorisation with the separate-launch kernels / the solve with the per-block launches inside the same call -- no
    # error, same bits.  "per-block": the single-vector solves as one launch per block (CBO_HIP_VEC_SOLVE_FORM=1).
    # "split": the block as a one-workgroup launch and the strips as an LDS-free launch behind it (CBO_HIP_PANEL_FORM=5,
    # what large factorisations use beside their bulk updates), forced at every size.
    variants = (("4", {"CBO_HIP_PANEL_FORM": "4"}), ("2", {"CBO_HIP_PANEL_FORM": "2"}), ("split", {"CBO_HIP_PANEL_FORM": "5"}),
                ("timeout", {"CBO_HIP_FUSED_SPIN_LIMIT": "-1"}), ("per-block", {"CBO_HIP_VEC_SOLVE_FORM": "1"}))
    for form, env in variants:
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        digests[form] = [ln for ln in out.stdout.splitlines() if ln.startswith("DIGEST")][-1]
    assert len(set(digests.values())) == 1, digests


def test_chain_launch_forms_give_the_same_bits_at_full_sizes(hip):
    """The same comparison at BASELINE's sizes, by digest of the factor and of a sweep: 4096 observations (32 panels; also
    through the overlapped refit + sweep call) and 16384 observations (128 panels, the fused launch with up to 255
    strips) -- fused, separate launches, and the forced give-up + repeat."""
    import subprocess
    import sys
    from conftest import ROOT
    code = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from cbo_with_oop_amd import CausalExpectedImprovement
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
h = hashlib.sha256()
for n in (4096, 16384):
    rng = np.random.default_rng(n)
    X = rng.uniform([-5, -5, -5], [5, 20, 5], (n, 3))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform([-5, -5, -5], [5, 20, 5], (1024, 3))
    m = HipGaussianProcess(X, y)
    L, alpha = m.posterior_state()
    h.update(np.ascontiguousarray(L).tobytes())
    h.update(np.ascontiguousarray(alpha).tobytes())
    del L
    ei = CausalExpectedImprovement(float(y.min()), "min", m)
    r = ei.sweep(Xs, want_acq=True, want_posterior=True)
    f = ei.sweep(Xs, want_acq=True, want_posterior=True, refit=True)          # cbo_gp_fit_sweep (overlapped at 4096)
    for res in (r, f):
        for k in ("acq", "var", "mean"):
            h.update(np.ascontiguousarray(res[k]).tobytes())
        h.update(str((m.jitter_tries, res["best_idx"])).encode())
    m.close()
print("DIGEST", h.hexdigest())
""" % ROOT
    digests = {}
    for form, env in (("auto", {}), ("4", {"CBO_HIP_PANEL_FORM": "4"}), ("2", {"CBO_HIP_PANEL_FORM": "2"}),
                      ("split", {"CBO_HIP_PANEL_FORM": "5"}), ("timeout", {"CBO_HIP_FUSED_SPIN_LIMIT": "-1"}),
                      ("per-block", {"CBO_HIP_VEC_SOLVE_FORM": "1"}),
                      # the bulk trailing updates pair by pair (K = 256), in groups of two pairs only (K = 512), in groups of
                      # four wherever they fit (K = 1024; the default takes them above 10240 trailing rows) -- on the side
                      # stream, the next group's rows brought up to date on the chain: same bits by construction
                      ("pairs", {"CBO_HIP_BULK_GROUP": "1"}), ("groups of two", {"CBO_HIP_BULK_GROUP": "2"}),
                      ("groups of four", {"CBO_HIP_BULK_GROUP4_ROWS": "0"})):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        digests[form] = [ln for ln in out.stdout.splitlines() if ln.startswith("DIGEST")][-1]
    assert len(set(digests.values())) == 1, digests


def test_optimizer_class_and_quotient_mirror_the_reference_call_sequence(hip):
    """src/utils_functions/utils.py:29-37 written out with the mirrored classes gives find_next_y_point's answer."""
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost,
                                                  find_next_y_point)
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory, GaussianProcessType
    f = load_fixture("toy_init_Z")
    model = GaussianProcessFactory.create(GaussianProcessType.NON_CAUSAL_GP, f["X"], f["y"], None, emukit_wrapper=True)
    costs = ToyGraph.get_cost_structure(1)
    space = ToyGraph.bounds(["Z"])
    cost_acquisition = Cost(costs, ["Z"])
    optimizer = CausalGradientAcquisitionOptimizer(space, grid_shape=[200])
    acquisition = CausalExpectedImprovement(float(f["y_best"]), "min", model) / cost_acquisition
    x_new, _ = optimizer.optimize(acquisition)
    y_acquisition = acquisition.evaluate(x_new)
    y2, x2 = find_next_y_point(space, model, float(f["y_best"]), ["Z"], costs, grid_shape=[200])
    assert np.array_equal(x_new, x2) and np.array_equal(x_new[0], f["Xs"][int(f["best_idx"])])
    assert np.allclose(y_acquisition, y2, rtol=1e-14) and np.isclose(y2[0, 0], float(f["best_val"]), rtol=1e-5)


def test_uniform_anchor_mode_against_the_oracle_on_the_same_anchors(hip):
    """The reference's own optimiser mode (``anchors="uniform"``, src/utils_functions/causal_optimizer.py:19,52-65) on the
    device: the 100 anchors drawn from numpy's global generator are scored by ONE device sweep -- against the oracle's
    acquisition on the same anchors, same top anchor --, L-BFGS from it lands where the same scipy call on the oracle's
    function and gradient lands, and ``find_next_y_point(anchors="uniform")`` re-evaluates the acquisition at the point
    found (src/utils_functions/utils.py:33-36)."""
    from scipy.optimize import fmin_l_bfgs_b
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost,
                                                  find_next_y_point)
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(33)
    bounds = [(-5.0, 4.0), (-5.0, 5.0)]                              # complete_graph (B, D)
    X = rng.uniform([-5, -5], [4, 5], (60, 2))
    y = np.sin(X[:, :1]) + 0.1 * X[:, 1:] ** 2 + 0.05 * rng.standard_normal((60, 1))
    m = HipGaussianProcess(X, y, noise_var=1e-4)
    post = O.fit(X, y, noise_var=1e-4)
    y_best = float(y.min())
    costs = CompleteGraph.get_cost_structure(1)
    acquisition = CausalExpectedImprovement(y_best, "min", m) / Cost(costs, ["B", "D"])
    np.random.seed(9)
    anchors = np.hstack([np.random.uniform(low=lo, high=hi, size=(100, 1)) for lo, hi in bounds])
    np.random.seed(9)
    x_new, fx = CausalGradientAcquisitionOptimizer(bounds, anchors="uniform").optimize(acquisition)
    # the anchors' scores: device against oracle, same winner
    scores = acquisition.evaluate(anchors)[:, 0]
    ref = O.acquisition_sweep(post, anchors, y_best, cost=2.0)[0].reshape(-1)
    big = np.abs(ref) > 1e-6 * np.abs(ref).max()
    assert np.allclose(scores[big], ref[big], rtol=1e-6) and int(np.argmax(scores)) == int(np.argmax(ref))
    start = anchors[np.argsort(ref)[::-1][:1]]

    def f_df(v):
        f, df = O.expected_improvement_with_gradients(post, v[None, :], y_best)
        return -float(f[0, 0]) / 2.0, -df[0] / 2.0
    xo, fo, _ = fmin_l_bfgs_b(f_df, start.reshape(-1), bounds=bounds, maxfun=1000)
    assert np.allclose(x_new[0], xo, atol=2e-4) and np.isclose(fx[0, 0], -fo, rtol=1e-5)
    assert fx[0, 0] >= scores.max() * (1 - 1e-9)                     # L-BFGS improved on (or kept) the best anchor
    np.random.seed(9)
    y2, x2 = find_next_y_point(bounds, m, y_best, ["B", "D"], costs, anchors="uniform")
    assert np.array_equal(x2, x_new) and np.isclose(y2[0, 0], fx[0, 0], rtol=1e-9)
    m.close()


# ---------------------------------------------------------------------------------- gradients + refinement (f3)
def test_prediction_gradients_and_refinement(hip):
    """get_prediction_gradients / evaluate_with_gradients against the oracle, then the reference's second
    optimiser stage (L-BFGS from the best grid point) with the same scipy call on both sides."""
    from scipy.optimize import fmin_l_bfgs_b
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph
    rng = np.random.default_rng(21)
    X = rng.uniform([-5, -5], [4, 5], (150, 2))
    y = np.sin(X[:, :1]) + 0.1 * X[:, 1:] ** 2 + 0.05 * rng.standard_normal((150, 1))
    m = HipGaussianProcess(X, y, variance=1.2, lengthscale=1.1, noise_var=1e-3)
    post = O.fit(X, y, variance=1.2, lengthscale=1.1, noise_var=1e-3)
    xs = rng.uniform([-5, -5], [4, 5], (9, 2))
    dm, dv = m.get_prediction_gradients(xs)
    dmo, dvo = O.predict_gradients(post, xs)
    assert np.allclose(dm, dmo, rtol=1e-7, atol=1e-9) and np.allclose(dv, dvo, rtol=1e-6, atol=1e-9)
    ei = CausalExpectedImprovement(float(y.min()), "min", m)
    f, df = ei.evaluate_with_gradients(xs)
    fo, dfo = O.expected_improvement_with_gradients(post, xs, float(y.min()))
    assert np.allclose(f, fo, rtol=1e-6, atol=1e-12) and np.allclose(df, dfo, rtol=1e-5, atol=1e-10)
    # ARD + causal kernel: gradients use the stationary part only, the solve uses the full kernel
    c = load_fixture("causal_d2")
    g = make_model(hip, c)
    pts = c["Xs"][:5]
    dm, dv = g.get_prediction_gradients(pts)
    cpost = O.fit(c["X"], c["y"], c["mX"], c["vX"])
    dmo, dvo = O.predict_gradients(cpost, pts, c["vXs"][:5])
    assert np.allclose(dm, dmo, rtol=1e-6, atol=1e-9) and np.allclose(dv, dvo, rtol=1e-5, atol=1e-9)
    # refinement: grid arg-max, then L-BFGS-B within the bounds
    bounds = CompleteGraph.bounds(["B", "D"])
    opt = CausalGradientAcquisitionOptimizer(bounds, grid_shape=[24, 24])
    acq = ei / Cost(CompleteGraph.get_cost_structure(1), ["B", "D"])
    x0, f0 = opt.optimize(acq)
    x1, f1 = opt.optimize(acq, refine=True)
    assert f1[0, 0] >= f0[0, 0] and all(lo <= v <= hi for v, (lo, hi) in zip(x1[0], bounds))

    def f_df(v):
        fv, dfv = O.expected_improvement_with_gradients(post, v[None, :], float(y.min()))
        return -float(fv[0, 0]) / 2.0, -dfv[0] / 2.0
    xo, fxo, _ = fmin_l_bfgs_b(f_df, x0[0], bounds=bounds, maxfun=1000)
    assert np.isclose(f1[0, 0], -fxo, rtol=1e-5) and np.allclose(x1[0], xo, atol=1e-4)


def test_multi_start_refinement_in_lockstep(hip):
    """Top-k grid points refined at once: one batched device call per round for all k searches; every
    search ends at least as high as it started, the winner is at least the single-start result, and the values the
    searches report are the oracle's acquisition at the points they report.  A variable cost (summed |x| of the batch it
    is given) is charged per point, as k separate single-point calls would."""
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph
    rng = np.random.default_rng(33)
    X = rng.uniform([-5, -5], [4, 5], (120, 2))
    y = np.sin(1.7 * X[:, :1]) * np.cos(1.3 * X[:, 1:]) + 0.05 * rng.standard_normal((120, 1))
    m = HipGaussianProcess(X, y, variance=1.0, lengthscale=0.8, noise_var=1e-3)
    post = O.fit(X, y, variance=1.0, lengthscale=0.8, noise_var=1e-3)
    best = float(y.min())
    bounds = CompleteGraph.bounds(["B", "D"])
    ei = CausalExpectedImprovement(best, "min", m)
    calls = []
    predict = m.get_prediction_gradients
    m.get_prediction_gradients = lambda x: (calls.append(np.shape(x)[0]), predict(x))[1]
    for cost_kind, scale in ((1, lambda P: np.full(len(P), 2.0)), (3, None)):
        acq = ei / Cost(CompleteGraph.get_cost_structure(cost_kind), ["B", "D"])
        opt = CausalGradientAcquisitionOptimizer(bounds, grid_shape=[24, 24])
        x0, f0 = opt.optimize(acq)
        x1, f1 = opt.optimize(acq, refine=True)
        calls.clear()
        x8, f8 = opt.optimize(acq, refine=True, num_starts=8)
        assert calls and set(calls) == {8}, calls                       # every round is ONE batch of the 8 searches
        assert all(lo <= v <= hi for v, (lo, hi) in zip(x8[0], bounds))
        fixed = cost_kind == 1      # (a variable cost prices the grid as ONE batch: grid and point values differ in scale)
        if fixed:
            assert f8[0, 0] >= f0[0, 0] and f8[0, 0] >= f1[0, 0] - 1e-9 * abs(f1[0, 0])
        # the searches themselves, from the 8 best grid points
        res = acq.sweep(opt._grid, want_acq=True)
        a = np.asarray(res["acq"]).reshape(-1)
        top = np.argsort(-a, kind="stable")[:8]
        starts = opt._grid.points[top]
        pts, vals = opt.refine_batched(acq, starts)
        if fixed:
            assert np.all(vals >= a[top] - 1e-12) and np.isclose(vals.max(), f8[0, 0], rtol=1e-12)
        fo, _ = O.expected_improvement_with_gradients(post, pts, best)
        cost = np.array([float(acq.denominator.evaluate(pts[i:i + 1])) for i in range(8)])
        if scale is not None:
            assert np.allclose(cost, scale(pts))
        assert np.allclose(vals, fo[:, 0] / cost, rtol=1e-6, atol=1e-14)
    m.close()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_bench_exchange_over_rccl_single_rank(hip):
    """bench.py under the one-process-per-GPU launcher with one rank: the communicator is RCCL formed inside
    libcbo_hip.so (no PyTorch in the bench process) and the winner goes through ncclAllGather on the GPU; it must
    equal the winner of the plain run."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--post-steps", "0"]
    plain = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common, env=env, capture_output=True,
                           text=True, timeout=300, cwd=ROOT)
    assert plain.returncode == 0, plain.stderr[-2000:]
    launched = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                               os.path.join(ROOT, "bench.py")] + common, env=dict(env, CBO_BENCH_STRONG_AT_ONE="1"),
                              capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert launched.returncode == 0, launched.stderr[-2000:]
    a = json.loads([l for l in plain.stdout.splitlines() if l.startswith("{")][-1])
    b = json.loads([l for l in launched.stdout.splitlines() if l.startswith("{")][-1])
    assert a["winner"] == b["winner"]
    # the strong-scaling leg of the several-rank line (c2's one grid cut into shards, timed through the same exchange),
    # taken here with the one rank this box holds: one shard = the whole grid, so its winner is the line's winner
    assert "strong" not in a
    st = b["strong"]
    assert st["scaling"] == "strong" and st["shard_of_rank_0"] == [0, st["candidates_total"]] == [0, 16384]
    assert st["winner"]["index"] == b["winner"]["index"] and st["winner"]["acq"] == b["winner"]["acq"]
    assert st["ms_per_step"] > 0 and abs(st["value"] * st["ms_per_step"] * 1e-3 - 16384) < 1e-6 * 16384
    assert b["n_gpus"] == 1 and "RCCL" in b["config"]["exchange"] and "RCCL" not in a["config"]["exchange"]
    assert b["config"]["rccl_ranks"] == 1 and a["config"]["rccl_ranks"] == 0
    # the self-launch form (what a plain `python bench.py --gpus N` does for N > 1; CBO_BENCH_SELF_LAUNCH=1 takes that
    # path with the one rank a one-GPU box can hold): bench.py is its own launcher, the rank is its child
    own = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common,
                         env=dict(env, CBO_BENCH_SELF_LAUNCH="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert own.returncode == 0, own.stderr[-2000:]
    lines = [l for l in own.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    c = json.loads(lines[0])
    assert c["winner"] == a["winner"] and c["n_gpus"] == 1 and c["config"]["rccl_ranks"] == 1


def test_bench_lines_of_the_other_configs_carry_the_contract(hip):
    """bench.py --config c1 and --config c3 (a short run each): one JSON line with the contract's fields, the config's own
    workload string, a roofline object, and -- c1 -- the CPU oracle taking the same decision."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def line(*args):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True,
                             text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])

    c1 = line("--config", "c1", "--steps", "200")
    c3 = line("--config", "c3", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--post-steps", "1")
    for d, cfg in ((c1, "c1"), (c3, "c3")):
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                    "vs_baseline", "dtype", "data", "config", "roofline"):
            assert key in d, (cfg, key)
        assert d["config"]["config"] == cfg and d["unit"] == "acquisitions/s" and d["vs_baseline"] is None
        assert d["roofline"]["bound"] == "mfma" and d["roofline"]["peak"] == 78.6
    assert c1["config"]["candidates_total"] == 400 and c1["cpu_baseline"]["same_choice"] is True
    assert c3["scaling"] == "strong" and c3["config"]["candidates_total"] == 65536 and c3["config"]["n_obs"] == 8192
    assert 0.5 < c3["roofline"]["isolated"]["frac"] < 1.0


def test_bench_dump_outputs_are_what_the_timed_steps_computed(hip, tmp_path):
    """bench.py --dump-outputs DIR: the line reports the --steps it was given; c2 writes acq, mean, var of the 16384
    candidates (float64) whose arg-max is the line's winner, and the overlapped step writes the same bits as the two-call
    step of --sequential; c1 writes each set's point and value and the pick, agreeing with the line."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def line(*args):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True,
                             text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])

    common = ["--steps", "3", "--warmup", "1", "--cpu-sample", "0", "--post-steps", "0"]
    fused = line(*common, "--dump-outputs", str(tmp_path / "fused"))
    seq = line(*common, "--sequential", "--dump-outputs", str(tmp_path / "seq"))
    assert fused["steps"] == seq["steps"] == 3 and fused["ms_per_step"] > 0
    d = {k: np.load(tmp_path / "fused" / f"{k}.npy") for k in ("acq", "mean", "var", "winner_value", "winner_index")}
    assert all(a.dtype == np.float64 for a in d.values())
    assert d["acq"].shape == d["mean"].shape == d["var"].shape == (16384,) and np.all(d["var"] > 0)
    w = int(d["winner_index"][0])
    assert w == fused["winner"]["index"] == int(np.argmax(d["acq"])) and d["acq"][w] == d["winner_value"][0] == fused["winner"]["acq"]
    for k, a in d.items():
        assert np.array_equal(a, np.load(tmp_path / "seq" / f"{k}.npy")), k
    c1 = line("--config", "c1", "--steps", "5", "--cpu-sample", "0", "--dump-outputs", str(tmp_path / "c1"))
    assert c1["steps"] == 5
    pick = np.load(tmp_path / "c1" / "pick.npy")
    acq_sets = [np.load(tmp_path / "c1" / f"acq_set{s}.npy") for s in range(2)]
    assert int(pick[0]) == c1["winner"]["set"] and acq_sets[int(pick[0])][0, 0] == c1["winner"]["acq"]
    assert all(np.load(tmp_path / "c1" / f"x_new_set{s}.npy").shape == (1, 1) for s in range(2))


def test_a_factor_taken_in_row_slices_is_the_factor(hip):
    """The hand-over of ``cbo_comm_share_factor`` between ranks cannot run on a one-GPU box (with one rank nobody lacks
    the factor).  Everything around the transfers is pinned here: model A holds the factor at the level the data need,
    model B (same data) has failed at the level below; B takes A's factor in the row slices of 1, 3 and 7 owners
    (``factor_slice``'s uneven split: whole lda-rows and the 16x16 diagonal inverses of the same rows, device copies in
    the place of ncclRecv) and adopts it -- and B's posterior state, predictions and sweep are A's bit for bit, at a size
    of several row blocks and on the jitter fixture."""
    import warnings
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("jitter_ladder")
    rng = np.random.default_rng(77)
    Xb = np.linspace(-2.0, 2.0, 700)[:, None]                        # a dense 1-D set of six row blocks ...
    Xb[350:] = Xb[:350]                                              # ... with duplicate rows and the fixture's negative
    yb = np.sin(3.0 * Xb)                                            # effective diagonal: level 0 fails, level 1 goes through
    cases = [(f["X"], f["y"], dict(noise_var=float(f["noise_var"]), variance=float(f["variance"]), lengthscale=f["lengthscale_arg"])),
             (Xb, yb, dict(noise_var=-1e-8 - 1e-9))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for X, y, kw in cases:
            a = HipGaussianProcess(X, y, **kw)
            need = a.jitter_tries
            assert need >= 1
            Xs = rng.uniform(X.min(0), X.max(0), (300, X.shape[1]))
            ref_state = [np.array(v) for v in a.posterior_state()]
            ref_pred = a.predict(Xs)
            ref_sweep = CausalExpectedImprovement(float(y.min()), "min", a).sweep(Xs, cost=2.0, want_acq=True)
            for owners in (1, 3, 7):
                b = HipGaussianProcess(X, y, **kw, fit=False)
                assert b.fit_level(need - 1)[0] == 0                 # B tried the level below: not positive definite
                b.take_factor_slices(a, need, owners)
                assert (b.jitter_tries, b.jitter) == (need, a.jitter)
                for u, v in zip(b.posterior_state(), ref_state):
                    assert np.array_equal(np.array(u), v)
                mu, var = b.predict(Xs)
                assert np.array_equal(mu, ref_pred[0], equal_nan=True) and np.array_equal(var, ref_pred[1], equal_nan=True)
                res = CausalExpectedImprovement(float(y.min()), "min", b).sweep(Xs, cost=2.0, want_acq=True)
                # (the fixture's negative effective noise makes some variances negative: NaN acquisitions, in both alike)
                assert np.array_equal(res["acq"], ref_sweep["acq"], equal_nan=True) and res["best_idx"] == ref_sweep["best_idx"]
                b.close()
            # a source that does not hold the level is refused
            c = HipGaussianProcess(X, y, **kw, fit=False)
            with pytest.raises(Exception):
                c.take_factor_slices(a, need + 1, 2)
            c.close(); a.close()


def test_ladder_levels_one_at_a_time_equal_the_plain_fit(hip):
    """cbo_gp_fit_level tries ONE level of jitchol's ladder (what a rank does when the ranks walk the ladder side by side,
    sharding.fit_over_ranks): on the jitter fixture (duplicate rows, no noise) the levels below the one the plain fit
    needs report "not positive definite", that level gives the plain fit's factor, jitter and posterior bit for bit, and
    a level beyond the ladder is jitchol's error.  With one rank fit_over_ranks IS the sequential walk; the single-rank
    communicator's gather and factor hand-over go through RCCL's entry points."""
    import warnings
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.sharding import Communicator, fit_over_ranks
    f = load_fixture("jitter_ladder")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = HipGaussianProcess(f["X"], f["y"], noise_var=float(f["noise_var"]), variance=float(f["variance"]),
                                   lengthscale=f["lengthscale_arg"])
        need = plain.jitter_tries
        assert need >= 1
        ref = [np.array(a) for a in plain.posterior_state()]
        lvl = HipGaussianProcess(f["X"], f["y"], noise_var=float(f["noise_var"]), variance=float(f["variance"]),
                                 lengthscale=f["lengthscale_arg"], fit=False)
        for level in range(need):
            assert lvl.fit_level(level)[0] == 0
        outcome, jitter = lvl.fit_level(need)
        assert outcome == 1 and (lvl.jitter_tries, lvl.jitter) == (need, plain.jitter) and jitter == plain.jitter
        for a, b in zip(lvl.posterior_state(), ref):
            assert np.array_equal(np.array(a), b)
        with pytest.raises(np.linalg.LinAlgError):
            lvl.fit_level(6)
        # one rank, no communicator: the sequential walk, whatever level is expected
        for expected in (None, 0, need, 4):
            walk = HipGaussianProcess(f["X"], f["y"], noise_var=float(f["noise_var"]), variance=float(f["variance"]),
                                      lengthscale=f["lengthscale_arg"], fit=False)
            assert fit_over_ranks(walk, None, expected) == (need, plain.jitter)
            for a, b in zip(walk.posterior_state(), ref):
                assert np.array_equal(np.array(a), b)
            walk.close()
        # the same through a one-rank RCCL communicator: the outcome travels through ncclAllGather, nobody lacks the factor
        comm = Communicator.single(_lib.Context.get())
        assert comm.gather(-7) == [-7]
        walk = HipGaussianProcess(f["X"], f["y"], noise_var=float(f["noise_var"]), variance=float(f["variance"]),
                                  lengthscale=f["lengthscale_arg"], fit=False)
        assert fit_over_ranks(walk, comm, need) == (need, plain.jitter)
        comm.share_factor(walk, need, [0], [])                       # nobody needs it: no transfer
        with pytest.raises(_lib.CboHipError):
            comm.share_factor(walk, need + 1, [0], [])               # an owner must hold the factor at that level
        comm.close()
        walk.close(); lvl.close(); plain.close()


def test_communicator_through_the_c_abi(hip):
    """cbo_comm_* with one rank (all a one-GPU box can form): both ways of forming the communicator, the arg-max
    exchange, the max reduction, and the empty-shard sentinel."""
    import ctypes
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.sharding import NO_CANDIDATE, Communicator
    ctx = _lib.Context.get()
    comm = Communicator.single(ctx)
    assert (comm.world, comm.rank) == (1, 0)
    assert comm.argmax(0.25, 1234567890123) == (0.25, 1234567890123)
    v, i = comm.argmax(float("nan"), 7)
    assert np.isnan(v) and i == 7
    assert comm.max(3.5) == 3.5
    comm.barrier()
    with pytest.raises(_lib.CboHipError) as e:
        comm.argmax(-np.inf, NO_CANDIDATE)              # every shard empty: nothing to pick
    assert e.value.code == _lib.CBO_ERR_INVALID
    comm.close()
    # one process driving the devices: ncclCommInitAll + grouped collectives
    lib = _lib.load()
    ctxs = (ctypes.c_void_p * 1)(ctx.handle)
    comms = (ctypes.c_void_p * 1)()
    _lib.check(lib.cbo_comm_init_all(1, ctxs, comms))
    vals, idxs = (ctypes.c_double * 1)(1.5), (ctypes.c_int64 * 1)(42)
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    _lib.check(lib.cbo_comm_argmax_all(1, comms, vals, idxs, ctypes.byref(bv), ctypes.byref(bi)))
    assert (bv.value, bi.value) == (1.5, 42)
    lib.cbo_comm_destroy(comms[0])
    # a bad library name surfaces as CBO_ERR_COMM in a fresh process (the library is opened once per process)
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from cbo_with_oop_amd import _lib\n"
            "from cbo_with_oop_amd.sharding import Communicator\n"
            "try:\n    Communicator.unique_id()\nexcept _lib.CboHipError as e:\n    print('code', e.code)\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CBO_HIP_RCCL_LIB="/nonexistent/librccl.so"),
                         capture_output=True, text=True, timeout=120)
    assert "code -8" in out.stdout, (out.stdout, out.stderr[-500:])          # CBO_ERR_COMM


def last_schedule(ctx, rows, candidates):
    """(pairs, group) the last cbo_gp_fit_sweep call of the shape ran, from cbo_schedule_report (pairs = -1: the plain
    sequence, fit then sweep)."""
    import re
    _, text = ctx.schedule_report()
    line = next(l for l in text.splitlines() if l.startswith(f"rows {rows} candidates {candidates}:"))
    m = re.search(r"last call ran pairs (-?\d+) group (\d+)", line)
    return int(m.group(1)), int(m.group(2))


def test_pair_blocks_and_128_row_blocks_give_the_same_bits(hip):
    """trsm_pair_kernel (256-row pair blocks: the default wherever the padded row count is a multiple of 256) against
    trsm_strip8_kernel (128-row blocks, CBO_HIP_STRIP_FORM=8; the form is read once per process, hence one process per form):
    digests of posterior mean, variance, acquisition, winner and prediction gradients -- the kernel's SWEEP and plain
    instantiations, forward and reversed factor -- at a two-pair, an ill-conditioned 1-D and a six-pair shape."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "strip_form_bits.py"), "500x4096x3", "1000x2048x1", "1500x4096x2"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.count("same bits") == 3 and "DIFFERENT" not in out.stdout, (out.stdout[-1500:], out.stderr[-800:])


def forced_context(monkeypatch, **env):
    """A fresh context whose schedule knobs are pinned (they are read when the context is created)."""
    from cbo_with_oop_amd import _lib
    for k, val in env.items():
        monkeypatch.setenv(k, str(val))
    ctx = _lib.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


@pytest.mark.parametrize("n,m,d", [(100, 300, 2), (128, 64, 1), (129, 1000, 3), (257, 777, 3), (640, 2048, 3),
                                   (1500, 4100, 4), (2100, 20000, 3)])
def test_three_schedules_give_the_same_bits(hip, monkeypatch, n, m, d):
    """The substitution V = L^-1 K* has three schedules: the left-looking strip kernel, the right-looking
    pair-by-pair pipeline on a finished factor (chosen for column counts that would leave CUs idle), and the same
    pipeline overlapped with the refit (cbo_gp_fit_sweep).  Each V element sees the same operations in the same
    order and q, mu are summed pair-wise in all three, so mean, variance and acquisition are bit-identical --
    schedule selection never shows in the results.  Against the oracle at the path's tolerance."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(n + m)
    X = rng.uniform(-3, 3, (n, d))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-3, 3, (m, d))
    left = forced_context(monkeypatch, CBO_HIP_SWEEP=0, CBO_HIP_OVERLAP=0)
    right = forced_context(monkeypatch, CBO_HIP_SWEEP=1, CBO_HIP_OVERLAP=1)
    out = []
    for ctx, refit in ((left, False), (right, False), (right, True)):
        model = HipGaussianProcess(X, y, lengthscale=1.3, noise_var=1e-2, context=ctx)
        grid = CandidateGrid(Xs, model, context=ctx)
        ei = CausalExpectedImprovement(float(y.min()), "min", model)
        out.append(ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True, refit=refit))
        if refit:
            # the model left behind is a fitted one, with the factor the plain fit produces
            again = ei.sweep(grid, cost=2.0, want_acq=True)
            assert np.array_equal(again["acq"], out[0]["acq"])
            L_overlapped = model.posterior_state()[0]
        else:
            L_plain = model.posterior_state()[0]
        grid.close(); model.close()
    assert np.array_equal(L_overlapped, L_plain)
    for other in out[1:]:
        assert other["best_idx"] == out[0]["best_idx"] and other["best_val"] == out[0]["best_val"]
        for key in ("mean", "var", "acq"):
            assert np.array_equal(other[key], out[0][key]), key
    left.close(); right.close()
    post = O.fit(X, y, lengthscale=1.3, noise_var=1e-2)
    mu, var = O.predict(post, Xs)
    np.testing.assert_allclose(out[2]["mean"], mu, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(out[2]["var"], var, rtol=1e-5, atol=1e-10)


def test_grouped_pipeline_gives_the_same_bits_at_the_headline_shape(hip):
    """BASELINE config 2's shape (4096 observations, 16384 candidates) through cbo_gp_fit_sweep with the pipelined sweep's
    updates pair by pair (CBO_HIP_PIPE_GROUP=1), in groups of two pairs (the automatic choice there: K = 512 on the bulk
    stream), of three and of four pairs, with an odd split (a remainder pair behind the groups), with pairs going alone ahead of
    the first group (CBO_HIP_PIPE_LEAD), and as the two plain calls
    (no overlap, left-looking): the update kernel accumulates into V sequentially, so every grouping gives the same bits."""
    import subprocess
    import sys
    from conftest import ROOT
    code = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
rng = np.random.default_rng(42)
X = rng.uniform([-5, -5, -5], [5, 20, 5], (4096, 3))
y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((4096, 1))
Xs = rng.uniform([-5, -5, -5], [5, 20, 5], (16384, 3))
m = HipGaussianProcess(X, y, fit=False)
g = CandidateGrid(Xs, m)
r = CausalExpectedImprovement(float(y.min()), "min", m).sweep(g, cost=1.5, want_acq=True, want_posterior=True, refit=True)
h = hashlib.sha256()
for k in ("acq", "var", "mean"):
    h.update(np.ascontiguousarray(r[k]).tobytes())
h.update(str(r["best_idx"]).encode())
h.update(np.ascontiguousarray(m.posterior_state()[0]).tobytes())
print("DIGEST", h.hexdigest())
""" % ROOT
    digests = {}
    for name, env in (("first call", {}), ("quarter", {"CBO_HIP_OVERLAP": "1"}), ("pairs", {"CBO_HIP_PIPE_GROUP": "1"}),
                      ("three", {"CBO_HIP_PIPE_GROUP": "3"}), ("four", {"CBO_HIP_PIPE_GROUP": "4"}),
                      ("odd split", {"CBO_HIP_PIPE_TAIL": "0.6875"}), ("all pipelined", {"CBO_HIP_PIPE_TAIL": "0"}),
                      # pairs that go alone AHEAD of the first group (what the measured schedule runs for a pair count that
                      # does not fill its groups): {0},{1,2}; {0},{1,2},{3,4}; {0},{1},{2,3,4}
                      ("one ahead, three pairs", {"CBO_HIP_PIPE_TAIL": "0.8125", "CBO_HIP_PIPE_LEAD": "1"}),
                      ("one ahead, five pairs", {"CBO_HIP_PIPE_TAIL": "0.6875", "CBO_HIP_PIPE_LEAD": "1"}),
                      ("two ahead, a group of three", {"CBO_HIP_PIPE_TAIL": "0.6875", "CBO_HIP_PIPE_GROUP": "3", "CBO_HIP_PIPE_LEAD": "2"}),
                      ("two calls", {"CBO_HIP_OVERLAP": "0"})):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        digests[name] = [ln for ln in out.stdout.splitlines() if ln.startswith("DIGEST")][-1]
    assert len(set(digests.values())) == 1, digests


def test_measured_schedule_settles_and_every_call_on_the_way_gives_the_same_bits(hip, monkeypatch):
    """cbo_gp_fit_sweep picks its schedule by timing the calls it is given (cbo_api.hip, schedule_choose): the plain
    sequence first, then neighbouring splits between the pipeline and the closing launch, groupings included.  Whatever
    it tries, the results are the same bits; it settles within its call budget and says what it chose."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    for knob in ("CBO_HIP_OVERLAP", "CBO_HIP_PIPE_TAIL", "CBO_HIP_PIPE_GROUP", "CBO_HIP_SCHEDULE_TUNE"):
        monkeypatch.delenv(knob, raising=False)
    ctx = forced_context(monkeypatch)
    rng = np.random.default_rng(5)
    X = rng.uniform(-4, 4, (1500, 2)); y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((1500, 1))
    model = HipGaussianProcess(X, y, noise_var=1e-2, fit=False, context=ctx)
    grid = CandidateGrid(rng.uniform(-4, 4, (16384, 2)), model, context=ctx)
    ei = CausalExpectedImprovement(float(y.min()), "min", model)
    first = ei.sweep(grid, refit=True)
    states, calls = set(), 1
    while True:
        exploring, text = ctx.schedule_report()
        assert "rows 1536 candidates 16384" in text
        states.add(text.split(": ")[1].split(" ")[0])
        if exploring == 0:
            break
        r = ei.sweep(grid, refit=True)
        calls += 1
        assert (r["best_val"], r["best_idx"]) == (first["best_val"], first["best_idx"])
        assert calls <= 110, text                       # (the tuner itself gives up after 96 sampled calls)
    assert "settled" in states and len(states) >= 3, (states, text)
    full = ei.sweep(grid, refit=True, want_acq=True, want_posterior=True)       # (outputs requested: the settled schedule)
    mu, var = model.predict(grid.points[:64])
    assert np.array_equal(np.ravel(full["mean"])[:64], mu[:, 0]) and full["best_idx"] == first["best_idx"]
    grid.close(); model.close(); ctx.close()


def test_first_call_of_a_fresh_context_is_overlapped_whatever_outputs_it_asks_for(hip, monkeypatch):
    """Round 4's tuner ran the plain sequence (fit, then sweep) on every call that could not be sampled -- every call that
    asked for the per-candidate outputs, every call under the profiling timers -- as long as the shape was cold: a caller of
    CausalExpectedImprovement.evaluate() on a stale model never left it.  Now the first call of a shape runs the analytic
    split, outputs or not, profiling or not, and the calls with outputs take part in the measurement.  At the headline
    shape: the first call of a fresh context, with every output requested, reports a pipelined schedule and returns the bits
    of the two calls; so does a fresh context that is never sampled (profiling on)."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    for knob in ("CBO_HIP_OVERLAP", "CBO_HIP_PIPE_TAIL", "CBO_HIP_PIPE_GROUP", "CBO_HIP_SCHEDULE_TUNE"):
        monkeypatch.delenv(knob, raising=False)
    rng = np.random.default_rng(11)
    X = rng.uniform([-5, -5, -5], [5, 20, 5], (4096, 3))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((4096, 1))
    Xs = rng.uniform([-5, -5, -5], [5, 20, 5], (16384, 3))
    ref_ctx = forced_context(monkeypatch, CBO_HIP_OVERLAP=0)                       # the two calls
    m0 = HipGaussianProcess(X, y, context=ref_ctx)
    g0 = CandidateGrid(Xs, m0, context=ref_ctx)
    two = CausalExpectedImprovement(float(y.min()), "min", m0).sweep(g0, cost=3.0, want_acq=True, want_posterior=True)
    for profiling in (False, True):
        ctx = forced_context(monkeypatch)
        ctx.set_profiling(profiling)
        model = HipGaussianProcess(X, y, fit=False, context=ctx)
        grid = CandidateGrid(Xs, model, context=ctx)
        ei = CausalExpectedImprovement(float(y.min()), "min", model)
        for call in range(3 if profiling else 1):
            one = ei.sweep(grid, cost=3.0, want_acq=True, want_posterior=True, refit=True)
            pairs, group = last_schedule(ctx, 4096, 16384)
            assert 1 <= pairs < 16, (profiling, call, pairs, group)              # some pairs pipelined, then the closing launch
            assert one["best_idx"] == two["best_idx"] and one["best_val"] == two["best_val"]
            for key in ("mean", "var", "acq"):
                assert np.array_equal(one[key], two[key]), (profiling, call, key)
        ctx.set_profiling(False)
        grid.close(); model.close(); ctx.close()
    g0.close(); m0.close(); ref_ctx.close()


def test_schedule_selection(hip):
    """Automatic choice: few strips at a large N go right-looking, full rounds of strips stay left-looking
    (checked through the launch count the timers report)."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    if os.environ.get("CBO_HIP_SWEEP") is not None:
        pytest.skip("the schedule is pinned by CBO_HIP_SWEEP")
    rng = np.random.default_rng(2)
    X = rng.uniform(-3, 3, (1100, 2)); y = np.cos(X[:, :1])
    model = HipGaussianProcess(X, y, noise_var=1e-2)
    ctx = _lib.Context.get()
    ei = CausalExpectedImprovement(0.0, "min", model)
    counts = {}
    for m in (1000, 16384):
        grid = CandidateGrid(rng.uniform(-3, 3, (m, 2)), model)
        ctx.set_profiling(True); ctx.reset_timers()
        ei.sweep(grid)
        counts[m] = ctx.timers()["n_trsm_launches"]
        ctx.set_profiling(False)
        grid.close()
    assert counts[16384] == 1 and counts[1000] > 1, counts


def test_overlapped_refit_sweep_jitter_ladder_and_chunking(hip, monkeypatch):
    """The overlapped call walks the same jitchol ladder (duplicate rows, no noise) and falls back to the plain
    sequence when the candidates do not fit one workspace."""
    import warnings
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("jitter_ladder")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model = make_model(hip, f)
        tries_seq, jit_seq = model.jitter_tries, model.jitter
        ei = CausalExpectedImprovement(float(f["y_best"]), "min", model)
        a = ei.sweep(f["Xs"], want_acq=True)
        b = ei.sweep(f["Xs"], want_acq=True, refit=True)
    assert tries_seq >= 1 and (model.jitter_tries, model.jitter) == (tries_seq, jit_seq)
    assert np.array_equal(b["acq"], a["acq"]) and b["best_idx"] == a["best_idx"]
    # candidates that need several workspace chunks: the call degrades to fit-then-sweep, bit-identical to it
    from cbo_with_oop_amd import _lib
    g = load_fixture("coral_max_d3")
    monkeypatch.setenv("CBO_HIP_WORKSPACE_MB", "1")
    small = _lib.Context(0)
    m2 = HipGaussianProcess(g["X"], g["y"], context=small)
    ei2 = CausalExpectedImprovement(float(g["y_best"]), "min", m2)
    two = ei2.sweep(g["Xs"], want_acq=True)
    one = ei2.sweep(g["Xs"], want_acq=True, refit=True)
    assert np.array_equal(one["acq"], two["acq"]) and one["best_idx"] == two["best_idx"]
    small.close()


def test_overlapped_refit_sweep_repeats_a_failed_attempt(hip, monkeypatch):
    """cbo_gp_fit_sweep at a size where it really overlaps (1152 observations), on a matrix whose first attempt is not
    positive definite (duplicate rows, a slightly negative effective diagonal add): the acquisition epilogue is queued
    behind the closing launch before the host has seen the factorisation's status, so the failed attempt's epilogue runs on
    garbage and must leave nothing behind -- the call repeats with jitchol's jitter and returns what fit + sweep return."""
    import warnings
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(77)
    X = rng.uniform(-3, 3, (576, 2))
    X = np.vstack([X, X])                                    # exact duplicates -> singular K
    y = np.sin(X.sum(1, keepdims=True)) + 0.01 * rng.standard_normal((len(X), 1))
    Xs = rng.uniform(-3, 3, (3000, 2))
    ctx = forced_context(monkeypatch, CBO_HIP_OVERLAP=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = HipGaussianProcess(X, y, noise_var=-1e-8 - 1e-9, context=ctx)
        assert plain.jitter_tries >= 1
        a = CausalExpectedImprovement(float(y.min()), "min", plain).sweep(Xs, want_acq=True, want_posterior=True)
        lazy = HipGaussianProcess(X, y, noise_var=-1e-8 - 1e-9, context=ctx, fit=False)
        grid = CandidateGrid(Xs, lazy, context=ctx)
        ei = CausalExpectedImprovement(float(y.min()), "min", lazy)
        b = ei.sweep(grid, want_acq=True, want_posterior=True, refit=True)
        c = ei.sweep(grid, want_acq=True, want_posterior=True)            # the unchanged model: from the cached q, mu
    assert (lazy.jitter_tries, lazy.jitter) == (plain.jitter_tries, plain.jitter)
    for r in (b, c):
        assert r["best_idx"] == a["best_idx"] and r["best_val"] == a["best_val"]
        for key in ("acq", "mean", "var"):
            assert np.array_equal(r[key], a[key]), key
    grid.close(); lazy.close(); plain.close(); ctx.close()


def test_deferred_refit_is_transparent(hip):
    """set_data(fit=False) / create(fit=False): the next sweep refits overlapped, any other consumer fits first;
    results equal the eager path; a not-PD model raises at that use."""
    from cbo_with_oop_amd import CausalExpectedImprovement, GaussianProcessFactory, GaussianProcessType
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(11)
    X = rng.uniform(-2, 2, (300, 2)); y = np.cos(X[:, :1]) + 0.05 * rng.standard_normal((300, 1))
    X2 = np.vstack([X, rng.uniform(-2, 2, (5, 2))]); y2 = np.vstack([y, rng.standard_normal((5, 1))])
    Xs = rng.uniform(-2, 2, (500, 2))
    eager = HipGaussianProcess(X, y, noise_var=1e-3)
    eager.set_data(X2, y2)
    lazy = HipGaussianProcess(X, y, noise_var=1e-3)
    lazy.set_data(X2, y2, fit=False)
    assert lazy.stale
    a = CausalExpectedImprovement(0.0, "min", eager).sweep(Xs, want_acq=True)
    b = CausalExpectedImprovement(0.0, "min", lazy).sweep(Xs, want_acq=True)
    assert not lazy.stale and b["best_idx"] == a["best_idx"] and np.array_equal(b["acq"], a["acq"])
    lazy.set_data(X, y, fit=False)
    mu_l, var_l = lazy.predict(Xs)                      # a consumer other than the sweep fits first
    mu_e, var_e = HipGaussianProcess(X, y, noise_var=1e-3).predict(Xs)
    assert not lazy.stale and np.array_equal(mu_l, mu_e) and np.array_equal(var_l, var_e)
    # construction without a fit, then the error of a hopeless matrix at first use
    bad_x = np.zeros((8, 1)); bad_y = np.zeros((8, 1))
    m = GaussianProcessFactory.create(GaussianProcessType.CAUSAL_GP, bad_x, bad_y,
                                      [lambda a: np.zeros((len(a), 1)), lambda a: -2.0 * np.ones((len(a), 1))], fit=False)
    with pytest.raises(np.linalg.LinAlgError):
        CausalExpectedImprovement(0.0, "min", m).sweep(np.ones((4, 1)))


def test_path_with_deferred_refit_takes_the_same_decisions(hip):
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    rng = np.random.default_rng(3)
    es = ToyGraph.get_exploration_set("MIS")
    picks = []
    for lazy in (False, True):
        xs = [rng.uniform(-5, 5, (40, 1)), rng.uniform(-5, 20, (40, 1))] if not picks else [x.copy() for x in xs0]
        xs0 = [x.copy() for x in xs]
        ys = [ToyGraph.target_do_x(xs[0]), ToyGraph.target_do_z(xs[1])]
        path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, ToyGraph.get_cost_structure(1), "min", xs, ys,
                                  [ToyGraph.bounds(s) for s in es], grid_shapes=[[300], [300]])
        path.update_all_gaussian_processes()
        best = min(float(ys[0].min()), float(ys[1].min()))
        trace = []
        for _ in range(4):
            xn, yn = path.compute_best_acquisition_values(best)
            _, s = path.select_next_intervention(yn)
            target = ToyGraph.target_do_x if s == 0 else ToyGraph.target_do_z
            path.data_x[s] = np.vstack([path.data_x[s], xn[s]]); path.data_y[s] = np.vstack([path.data_y[s], target(xn[s])])
            best = min(best, float(path.data_y[s][-1, 0]))
            path.update_gaussian_process_of_last_intervention(fit=not lazy)
            trace.append((s, float(xn[s][0, 0])))
        picks.append(trace)
    assert [t[0] for t in picks[0]] == [t[0] for t in picks[1]]
    np.testing.assert_allclose([t[1] for t in picks[0]], [t[1] for t in picks[1]], rtol=0, atol=1e-12)


@pytest.mark.parametrize("n,d,ard,causal", [(60, 1, False, False), (200, 3, False, False), (333, 4, True, False),
                                            (1100, 3, False, True), (1500, 2, True, False)])
def test_likelihood_gradients_match_the_restatement(hip, n, d, ard, causal):
    """cbo_gp_lml_gradients (Ky^-1 = L^-T L^-1 by the sweep and GEMM kernels, contraction on the device) against the
    oracle's analytic gradients; n >= 1024 exercises the right-looking inverse and several panel pairs."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(n + d)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X[:, :1]) + 0.2 * X[:, -1:] + 0.05 * rng.standard_normal((n, 1))
    ls = np.linspace(0.7, 1.6, d) if ard else 0.9
    kw = dict(variance=1.2, lengthscale=ls, noise_var=0.04)
    okw = dict(kw)
    if causal:
        mean_fn = lambda a: 0.1 * a[:, :1]
        var_fn = lambda a: 0.2 + 0.1 * np.cos(a[:, 1:2]) ** 2
        kw.update(mean_function=mean_fn, variance_adjustment=var_fn)
        okw.update(mX=mean_fn(X), vX=var_fn(X))
    m = HipGaussianProcess(X, y, ard=ard, **kw)
    dv, dls, dn = m.log_likelihood_gradients()
    post = O.fit(X, y, **okw)
    o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
    scale = max(abs(o_dv), np.max(np.abs(o_dls)), abs(o_dn))
    assert m._last_lml == pytest.approx(O.log_marginal_likelihood(post), rel=1e-9)
    assert dv == pytest.approx(o_dv, rel=1e-6, abs=1e-8 * scale)
    assert dn == pytest.approx(o_dn, rel=1e-6, abs=1e-8 * scale)
    np.testing.assert_allclose(dls, o_dls, rtol=1e-6, atol=1e-8 * scale)
    # the sweep state is untouched by the gradient call: a sweep afterwards equals one before
    from cbo_with_oop_amd import CausalExpectedImprovement
    Xs = rng.uniform(-2, 2, (130, d))
    a = CausalExpectedImprovement(0.0, "min", m).sweep(Xs, want_acq=True)
    m.log_likelihood_gradients()
    b = CausalExpectedImprovement(0.0, "min", m).sweep(Xs, want_acq=True)
    assert np.array_equal(a["acq"], b["acq"])


@pytest.mark.parametrize("n,d,ard,causal", [(10, 1, False, False), (50, 2, False, False), (100, 3, True, False),
                                            (128, 3, False, True), (17, 4, True, True), (33, 8, False, False)])
def test_small_model_likelihood_gradients_in_one_launch(hip, n, d, ard, causal):
    """Models of at most 128 observations: likelihood and gradients straight from the data and the hyper-parameters
    (one workgroup, no fit before, none left behind) against the oracle; after new hyper-parameters again; the model
    still answers a sweep afterwards (it fits itself then)."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(7 * n + d)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X[:, :1]) + 0.2 * X[:, -1:] + 0.05 * rng.standard_normal((n, 1))
    prior = {}
    if causal:
        mean_fn = lambda a: 0.1 * a[:, :1]
        var_fn = lambda a: 0.2 + 0.1 * np.cos(a[:, -1:]) ** 2
        prior = dict(mean_function=mean_fn, variance_adjustment=var_fn)
    m = HipGaussianProcess(X, y, ard=ard, variance=1.2, lengthscale=np.linspace(0.7, 1.6, d) if ard else 0.9,
                           noise_var=0.04, fit=False, **prior)
    assert m.small and m.stale
    for variance, ls, noise in ((1.2, np.linspace(0.7, 1.6, d) if ard else 0.9, 0.04),
                                (0.6, np.linspace(1.3, 0.8, d) if ard else 1.4, 0.3)):
        m.set_hyperparameters(variance, ls, noise, fit=False)
        dv, dls, dn = m.log_likelihood_gradients()
        assert m.stale                                             # nothing was fitted on the way
        okw = dict(variance=variance, lengthscale=ls, noise_var=noise)
        if causal:
            okw.update(mX=mean_fn(X), vX=var_fn(X))
        post = O.fit(X, y, **okw)
        o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
        scale = max(abs(o_dv), np.max(np.abs(o_dls)), abs(o_dn))
        assert m._last_lml == pytest.approx(O.log_marginal_likelihood(post), rel=1e-10)
        assert dv == pytest.approx(o_dv, rel=1e-8, abs=1e-10 * scale)
        assert dn == pytest.approx(o_dn, rel=1e-8, abs=1e-10 * scale)
        np.testing.assert_allclose(dls, o_dls, rtol=1e-8, atol=1e-10 * scale)
    Xs = rng.uniform(-2, 2, (70, d))
    res = CausalExpectedImprovement(0.0, "min", m).sweep(Xs, want_acq=True)
    acq, _, idx, _, _ = O.acquisition_sweep(post, Xs, 0.0, vXs=var_fn(Xs) if causal else None,
                                            mXs=mean_fn(Xs) if causal else None)
    assert res["best_idx"] == idx
    m.close()


def test_small_model_likelihood_falls_back_when_not_positive_definite(hip):
    """Ky not positive definite as assembled (duplicated points, the reference's 1e-10 noise): the one-launch path
    declines, the model is fitted with the jitchol ladder and the general path answers -- the oracle's numbers with
    the same jitter."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    c = load_fixture("jitter_ladder")
    import warnings
    m = HipGaussianProcess(c["X"], c["y"], variance=float(c["variance"]), lengthscale=c["lengthscale_arg"],
                           noise_var=float(c["noise_var"]), fit=False)
    assert m.small and m.stale
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        dv, dls, dn = m.log_likelihood_gradients()
    post = O.fit(c["X"], c["y"], variance=float(c["variance"]), lengthscale=c["lengthscale_arg"],
                 noise_var=float(c["noise_var"]))
    assert post.tries >= 1
    o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
    assert m._last_lml == pytest.approx(O.log_marginal_likelihood(post), rel=1e-6)
    assert dv == pytest.approx(o_dv, rel=1e-4) and dn == pytest.approx(o_dn, rel=1e-4)
    m.close()


def test_complete_graph_trial_loop_end_to_end(hip):
    """The whole mirrored stack on the reference's complete graph, trial after trial: per-set GPs
    (GaussianProcessFactory), grid acquisition per set (find_next_y_point), set selection, the Monte-Carlo target
    of the chosen intervention on the device (compute_interventions, 20 000 draws of the reference's noise stream),
    data append and deferred refit -- against the same loop on the CPU restatements.  Same sets, same grid points,
    same targets."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import CompleteGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import graph_functions as G
    from oracle import sem_oracle as S
    es = CompleteGraph.get_exploration_set("MIS")
    bounds = [CompleteGraph.bounds(s) for s in es]
    shapes = [[40] if len(s) == 1 else [12, 12] for s in es]
    costs = CompleteGraph.get_cost_structure(1)
    draws = 20000
    sem_dev, sem_cpu = CompleteGraph.define_sem(), S.complete_graph_sem()
    rng = np.random.default_rng(9)
    x0 = [np.array([[rng.uniform(lo, hi) for lo, hi in b] for _ in range(4)]) for b in bounds]

    def target_dev(s, x):
        return G.compute_interventions(sem_dev, {n: "" for n in es[s]}, x, num_samples=draws)

    def target_cpu(s, x):
        return np.array([[S.compute_interventions(sem_cpu, dict(zip(es[s], row)), num_samples=draws)] for row in x])

    y0 = [target_cpu(s, x0[s]) for s in range(len(es))]
    y0_dev = [target_dev(s, x0[s]) for s in range(len(es))]
    for a, b in zip(y0, y0_dev):
        np.testing.assert_allclose(b, a, rtol=1e-12)

    def run(device):
        xs, ys = [x.copy() for x in x0], [y.copy() for y in y0]
        best = min(float(y.min()) for y in ys)
        trace = []
        if device:
            path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, costs, "min", xs, ys, bounds, grid_shapes=shapes)
            path.update_all_gaussian_processes()
        grids = [meshgrid_candidates(bounds[s], shapes[s]) for s in range(len(es))]
        for _ in range(6):
            if device:
                x_new, y_acq = path.compute_best_acquisition_values(best)
                _, s = path.select_next_intervention(y_acq)
                x_pick = x_new[s]
            else:
                vals, idxs = [], []
                for s in range(len(es)):
                    _, val, idx, _, _ = O.acquisition_sweep(O.fit(xs[s], ys[s]), grids[s], best, cost=float(len(es[s])))
                    vals.append(val); idxs.append(idx)
                s = O.select_next_intervention([np.array([[v]]) for v in vals])
                x_pick = grids[s][idxs[s]][None, :]
            y_new = target_dev(s, x_pick) if device else target_cpu(s, x_pick)
            xs[s] = np.vstack([xs[s], x_pick]); ys[s] = np.vstack([ys[s], y_new])
            best = min(best, float(y_new[0, 0]))
            if device:
                path.data_x[s], path.data_y[s] = xs[s], ys[s]
                path.update_gaussian_process_of_last_intervention()
            trace.append((s, tuple(np.round(x_pick[0], 12)), float(y_new[0, 0])))
        return trace

    dev, cpu = run(True), run(False)
    assert [(s, x) for s, x, _ in dev] == [(s, x) for s, x, _ in cpu], (dev, cpu)
    np.testing.assert_allclose([y for _, _, y in dev], [y for _, _, y in cpu], rtol=1e-12)


def test_unchanged_model_resweeps_from_cached_q_mu(hip, monkeypatch):
    """Between refits only the incumbent (and the cost) change: a candidate set keeps q = sum V^2 and mu = V^T z of
    its last sweep, stamped with the model's fit, and the next sweep of the unchanged model recomputes EI / cost /
    arg-max from them without touching the substitution.  Same bits as a cold sweep; a refit invalidates."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(77)
    X = rng.uniform(-2, 2, (700, 2)); y = np.cos(X[:, :1]) * X[:, 1:2] + 0.05 * rng.standard_normal((700, 1))
    Xs = rng.uniform(-2, 2, (3000, 2))
    ctx = _lib.Context.get()
    model = HipGaussianProcess(X, y, noise_var=1e-3)
    grid = CandidateGrid(Xs, model)
    first = CausalExpectedImprovement(0.3, "min", model).sweep(grid, cost=1.0, want_acq=True, want_posterior=True)
    ctx.set_profiling(True); ctx.reset_timers()
    warm = CausalExpectedImprovement(-0.2, "max", model).sweep(grid, cost=2.5, want_acq=True, want_posterior=True)
    launches = ctx.timers()["n_trsm_launches"]
    ctx.set_profiling(False)
    assert launches == 0
    cold_ctx = forced_context(monkeypatch, CBO_HIP_SWEEP_CACHE=0)
    cold_model = HipGaussianProcess(X, y, noise_var=1e-3, context=cold_ctx)
    cold = CausalExpectedImprovement(-0.2, "max", cold_model).sweep(CandidateGrid(Xs, cold_model, context=cold_ctx), cost=2.5,
                                                                    want_acq=True, want_posterior=True)
    for key in ("acq", "mean", "var"):
        assert np.array_equal(warm[key], cold[key]), key
    assert warm["best_idx"] == cold["best_idx"] and np.array_equal(warm["mean"], first["mean"])
    # new data -> new fit stamp -> the substitution runs again
    X2 = np.vstack([X, [[0.1, 0.2]]]); y2 = np.vstack([y, [[1.5]]])
    model.set_data(X2, y2)
    ctx.set_profiling(True); ctx.reset_timers()
    after = CausalExpectedImprovement(-0.2, "max", model).sweep(grid, cost=2.5, want_posterior=True)
    assert ctx.timers()["n_trsm_launches"] >= 1
    ctx.set_profiling(False)
    mu, var = O.predict(O.fit(X2, y2, noise_var=1e-3), Xs)
    np.testing.assert_allclose(after["mean"], mu, rtol=1e-6, atol=1e-9)
    cold_model.close(); cold_ctx.close()


def test_overlapped_call_retries_with_jitter_and_handles_causal_ard(hip, monkeypatch):
    """The pipelined schedule itself (n_pad >= 1024, so no fallback) on the awkward inputs: (1) duplicated rows
    without noise -> the first factorisation fails while sweep kernels are already in flight; the whole pipeline
    (K* included) is redone along GPy's jitter ladder and ends where the two calls end; (2) a causal kernel
    (prior mean / variance on observations and candidates) with ARD lengthscales."""
    import warnings
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(5)
    base = rng.uniform(-2, 2, (600, 2))
    X = np.vstack([base, base])                              # every row twice ...
    y = np.vstack([np.sin(base[:, :1]), np.sin(base[:, :1])])
    Xs = rng.uniform(-2, 2, (5000, 2))
    kw = dict(noise_var=-1e-8 - 1e-9)                       # ... and a 'noise' that cancels GPy's 1e-8: singular Ky
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eager = HipGaussianProcess(X, y, **kw)
        assert eager.jitter_tries >= 1
        two = CausalExpectedImprovement(0.0, "min", eager).sweep(Xs, want_acq=True, want_posterior=True)
        lazy = HipGaussianProcess(X, y, fit=False, **kw)
        one = CausalExpectedImprovement(0.0, "min", lazy).sweep(Xs, want_acq=True, want_posterior=True)
    assert (lazy.jitter_tries, lazy.jitter) == (eager.jitter_tries, eager.jitter)
    for key in ("acq", "mean", "var"):
        assert np.array_equal(one[key], two[key]), key
    # causal + ARD through the pipeline, against the oracle
    n, d = 1300, 3
    X = rng.uniform(-2, 2, (n, d)); y = np.cos(X[:, :1]) + 0.3 * X[:, 1:2] + 0.05 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2, 2, (2500, d))
    mean_fn = lambda a: 0.2 * a[:, :1]
    var_fn = lambda a: 0.1 + 0.05 * np.sin(a[:, 2:3]) ** 2
    ls = np.array([0.8, 1.2, 1.7])
    m = HipGaussianProcess(X, y, variance=1.1, lengthscale=ls, ard=True, noise_var=1e-2, mean_function=mean_fn,
                           variance_adjustment=var_fn, fit=False)
    res = CausalExpectedImprovement(float(y.min()), "min", m).sweep(CandidateGrid(Xs, m), cost=2.0, want_posterior=True)
    post = O.fit(X, y, mean_fn(X), var_fn(X), 1.1, ls, 1e-2)
    mu, var = O.predict(post, Xs, mean_fn(Xs), var_fn(Xs))
    np.testing.assert_allclose(res["mean"], mu, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(res["var"], var, rtol=1e-6, atol=1e-10)


@pytest.mark.parametrize("n0,d,causal", [(40, 1, False), (250, 2, False), (1100, 3, False), (300, 2, True)])
def test_append_only_trial_step_matches_full_refit(hip, n0, d, causal):
    """Appending one observation at a time (cbo_gp_append + one new row of the resident V) against refitting and
    re-sweeping from scratch: factor, alpha, mean, variance and acquisition agree to rounding, the winner is the
    same, trial after trial -- including the appends that cross a 16-row tile and (n0 = 250) the 128-row padding
    boundary, where the shortcut declines and the full path takes over."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(n0 + d)
    f = lambda a: np.sin(a[:, :1]) + 0.3 * np.cos(2 * a[:, -1:])
    X = rng.uniform(-2, 2, (n0, d)); y = f(X) + 0.05 * rng.standard_normal((n0, 1))
    Xs = rng.uniform(-2, 2, (1500, d))
    kw = dict(noise_var=1e-2, lengthscale=0.9)
    if causal:
        kw.update(mean_function=lambda a: 0.1 * a[:, :1], variance_adjustment=lambda a: 0.2 + 0.1 * np.cos(a[:, 1:2]) ** 2)
    inc = HipGaussianProcess(X, y, **kw)
    grid = CandidateGrid(Xs, inc, keep_solution=True)
    CausalExpectedImprovement(float(y.min()), "min", inc).sweep(grid)
    appended = 0
    for step in range(9):
        x_new = rng.uniform(-2, 2, (1, d)); y_new = f(x_new) + 0.05 * rng.standard_normal((1, 1))
        X = np.vstack([X, x_new]); y = np.vstack([y, y_new])
        ok = inc.append(x_new, y_new)
        appended += int(ok)
        if not ok:
            inc.set_data(X, y)
        best = float(y.min())
        a = CausalExpectedImprovement(best, "min", inc).sweep(grid, cost=2.0, want_acq=True, want_posterior=True)
        ref_model = HipGaussianProcess(X, y, **kw)
        b = CausalExpectedImprovement(best, "min", ref_model).sweep(Xs, cost=2.0, want_acq=True, want_posterior=True)
        np.testing.assert_allclose(a["mean"], b["mean"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(a["var"], b["var"], rtol=1e-8, atol=1e-13)
        big = b["acq"][:, 0] > 1e-6 * b["acq"].max()
        np.testing.assert_allclose(a["acq"][big], b["acq"][big], rtol=1e-6)
        assert a["best_idx"] == b["best_idx"], step
        La, alpha_a = inc.posterior_state()
        Lb, alpha_b = ref_model.posterior_state()
        np.testing.assert_allclose(La, Lb, rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(alpha_a, alpha_b, rtol=1e-7, atol=1e-9)
        assert inc.log_likelihood() == pytest.approx(ref_model.log_likelihood(), rel=1e-10)
        assert np.array_equal(inc.X, X) and np.array_equal(inc.Y, y)
        ref_model.close()
    assert appended >= (6 if n0 == 250 else 9)       # 250 + 6 = 256: the padded size runs out once
    # a full refit of the grown model reproduces itself (the resident data are complete)
    inc.set_data(X, y)
    c = CausalExpectedImprovement(best, "min", inc).sweep(grid, cost=2.0, want_acq=True)
    np.testing.assert_allclose(c["acq"][big], b["acq"][big], rtol=1e-9)


# ------------------------------------------------------------------------- every set of a trial in one launch
def _per_set_reference(hip, models, grids, y_best, task, costs):
    """The general path, set by set (cbo_acq_sweep after a fit)."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    out = []
    for m, g, c in zip(models, grids, costs):
        m.ensure_fitted()
        r = CausalExpectedImprovement(y_best, task, m).sweep(g, cost=c)
        out.append((r["best_val"], r["best_idx"]))
    return out


def _sweep_sets(models, grids, y_best, task, costs):
    import ctypes
    from cbo_with_oop_amd import _lib
    s = len(models)
    gps = (ctypes.c_void_p * s)(*[m._handle for m in models])
    cds = (ctypes.c_void_p * s)(*[g._handle for g in grids])
    yb, cs = np.full(s, float(y_best)), np.asarray(costs, dtype=np.float64)
    vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
    _lib.check(_lib.load().cbo_acq_sweep_sets(s, gps, cds, _lib.dptr(yb), _lib.TASK_CODE[task], 0.0, _lib.dptr(cs),
                                              _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)))
    return list(zip(vals.tolist(), idxs.tolist()))


def test_sweep_sets_small_models_equal_the_per_set_path(hip):
    """cbo_acq_sweep_sets on the reference's own model sizes (10..50 observations, src/ArgumentParser.py:18,25): one
    launch for all sets, UNFITTED models included, must give the per-set general path's winners -- same device
    functions, same summation orders, so the same bits."""
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import CompleteGraph, ToyGraph, meshgrid_candidates
    fx, fz, fc = load_fixture("toy_init_X"), load_fixture("toy_init_Z"), load_fixture("toy_c1_Z50")
    rng = np.random.default_rng(5)
    models, grids, costs = [], [], []
    for f in (fx, fz, fc):
        models.append(HipGaussianProcess(f["X"], f["y"], fit=False))           # never fitted before the launch
        grids.append(CandidateGrid(f["Xs"], models[-1]))
        costs.append(float(f["cost"]))
    # complete-graph sets: d = 1 and d = 2, 17 and 100 points, an index offset and a ragged candidate count
    for names, n, shape in ((("B",), 17, (333,)), (("B", "D"), 100, (25, 21)), (("D", "E"), 128, (40, 40))):
        box = CompleteGraph.bounds(list(names))
        lo, hi = np.array([b[0] for b in box], float), np.array([b[1] for b in box], float)
        X = rng.uniform(lo, hi, (n, len(box)))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
        models.append(HipGaussianProcess(X, y, fit=False))
        grids.append(CandidateGrid(meshgrid_candidates(box, shape), models[-1], index_offset=1000 * len(models)))
        costs.append(float(len(names)))
    y_best = -0.7
    for task in ("min", "max"):
        got = _sweep_sets(models, grids, y_best, task, costs)
        assert all(m.stale for m in models)                                    # the launch left the models alone
        ref_models = [HipGaussianProcess(m.X, m.Y) for m in models]
        ref_grids = [CandidateGrid(g.points, rm, index_offset=g.index_offset) for g, rm in zip(grids, ref_models)]
        want = _per_set_reference(hip, ref_models, ref_grids, y_best, task, costs)
        assert got == want, (task, got, want)
    # against the oracle on the toy fixtures (the fixtures' own incumbent and task)
    for f, m, g in zip((fx, fz, fc), models, grids):
        (val, idx), = _sweep_sets([m], [g], float(f["y_best"]), f["task"], [float(f["cost"])])
        assert idx == int(f["best_idx"]), f["note"]


def test_sweep_sets_on_both_sides_of_the_two_launch_split(hip):
    """cbo_acq_sweep_sets with 13 candidate blocks per set (two launches: one workgroup per set factors, the sweep reads
    the factor back) and, the first set's candidates cut to 700, with 11 (one launch: every workgroup factors): a
    non-causal d = 1 model of 17 observations (one ragged tile) and a causal d = 3 model of 128 whose second workgroup
    holds one live candidate.  Winners and values are cbo_gp_fit_sweep's on twin models, bit for bit."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(13)
    mean_f = lambda a: 0.3 * np.sin(a).sum(1, keepdims=True)                   # noqa: E731
    var_f = lambda a: 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2       # noqa: E731
    kws = [dict(noise_var=1e-3), dict(variance=1.3, lengthscale=0.9, noise_var=1e-3, mean_function=mean_f,
                                      variance_adjustment=var_f)]
    data, cand = [], []
    for n, m, d in ((17, 800, 1), (128, 65, 3)):
        X = rng.uniform(-2.0, 2.0, (n, d))
        data.append((X, np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))))
        cand.append(rng.uniform(-2.5, 2.5, (m, d)))
    y_best, costs = 0.2, [1.0, 3.0]
    for m0 in (800, 700):
        pts = [cand[0][:m0], cand[1]]
        assert (max(len(p) for p in pts) + 63) // 64 == (13 if m0 == 800 else 11)
        models = [HipGaussianProcess(X, y, fit=False, **kw) for (X, y), kw in zip(data, kws)]
        grids = [CandidateGrid(p, m, index_offset=100 * i) for i, (p, m) in enumerate(zip(pts, models))]
        got = _sweep_sets(models, grids, y_best, "min", costs)
        assert all(m.stale for m in models)
        twins = [HipGaussianProcess(X, y, fit=False, **kw) for (X, y), kw in zip(data, kws)]
        want = []
        for i, (p, t) in enumerate(zip(pts, twins)):
            r = CausalExpectedImprovement(y_best, "min", t).sweep(CandidateGrid(p, t, index_offset=100 * i), cost=costs[i],
                                                                  refit=True)
            want.append((r["best_val"], r["best_idx"]))
        assert got == want, (m0, got, want)


def test_sweep_sets_twenty_five_sets_in_one_call(hip):
    """The coral graph's count of exploration sets (S = 25, src/graphs/impl/CoralGraph.py:162-175) in ONE call: more
    sets than travel as kernel arguments, so the descriptors are read from the pinned array; dimensions 1..3, ragged
    sizes and grids, against the per-set general path (same bits) and the oracle's arg-max."""
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    rng = np.random.default_rng(25)
    models, grids, costs, boxes = [], [], [], []
    for sidx in range(25):
        d = 1 + sidx % 3
        n = 8 + (7 * sidx) % 60
        box = [(-1.0 - 0.1 * sidx, 2.0 + 0.05 * sidx)] * d
        X = rng.uniform(box[0][0], box[0][1], (n, d))
        y = np.cos(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
        models.append(HipGaussianProcess(X, y, noise_var=1e-3, fit=False))
        shape = [(150,), (17, 13), (7, 6, 5)][d - 1]
        grids.append(CandidateGrid(meshgrid_candidates(box, shape), models[-1]))
        costs.append(float(d))
        boxes.append((box, shape))
    y_best = 0.1
    got = _sweep_sets(models, grids, y_best, "min", costs)
    ref_models = [HipGaussianProcess(m.X, m.Y, noise_var=1e-3) for m in models]
    ref_grids = [CandidateGrid(g.points, rm) for g, rm in zip(grids, ref_models)]
    want = _per_set_reference(hip, ref_models, ref_grids, y_best, "min", costs)
    assert got == want
    for m, g, c, (val, idx) in zip(models, grids, costs, got):
        _, o_val, o_idx, _, _ = O.acquisition_sweep(O.fit(m.X, m.Y, noise_var=1e-3), g.points, y_best, cost=c)
        assert idx == o_idx and np.isclose(val, o_val, rtol=1e-6, atol=1e-300)


def test_sweep_sets_mixed_sizes_causal_and_jitter(hip):
    """One call over: a causal small model, a small model whose K needs jitchol's jitter (duplicate rows: the general
    path takes over for that set), a model beyond 128 observations, an fp32 model."""
    import warnings
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    fcausal, fj, fbig = load_fixture("causal_d2"), load_fixture("jitter_ladder"), load_fixture("complete_bo_d3")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mc = make_model(hip, fcausal)
        mj = HipGaussianProcess(fj["X"], fj["y"], noise_var=float(fj["noise_var"]), fit=False)
        rng = np.random.default_rng(3)
        Xb = rng.uniform(-3, 3, (300, 3))
        yb = np.cos(Xb).sum(1, keepdims=True)
        mb = HipGaussianProcess(Xb, yb, fit=False)
        m32 = HipGaussianProcess(Xb[:200], yb[:200], noise_var=1e-2, dtype="f32")
        models = [mc, mj, mb, m32]
        grids = [CandidateGrid(fcausal["Xs"], mc), CandidateGrid(fj["Xs"], mj), CandidateGrid(fbig["Xs"], mb),
                 CandidateGrid(fbig["Xs"], m32)]
        costs = [2.0, 1.0, 3.0, 3.0]
        got = _sweep_sets(models, grids, 0.1, "min", costs)
        refs = [make_model(hip, fcausal), make_model(hip, fj), HipGaussianProcess(Xb, yb),
                HipGaussianProcess(Xb[:200], yb[:200], noise_var=1e-2, dtype="f32")]
        want = _per_set_reference(hip, refs, [CandidateGrid(g.points, r) for g, r in zip(grids, refs)], 0.1, "min", costs)
    assert got == want, (got, want)
    assert refs[1].jitter_tries >= 1                                           # that set did need the ladder


def test_sweep_sets_switch_and_path_integration(hip, monkeypatch):
    """CBO_HIP_SMALL_SETS=0 sends everything through the general path (same answers), and CBOAcquisitionPath's
    compute_best_acquisition_values is the multi-set call."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    rng = np.random.default_rng(0)
    es = ToyGraph.get_exploration_set("MIS")
    xs = [rng.uniform(-5, 5, (50, 1)), rng.uniform(-5, 20, (50, 1))]
    ys = [ToyGraph.target_do_x(xs[0]), ToyGraph.target_do_z(xs[1])]

    def run():
        path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, ToyGraph.get_cost_structure(1), "min", xs, ys,
                                  [ToyGraph.bounds(s) for s in es], grid_shapes=[[200], [200]])
        path.update_all_gaussian_processes()
        best = min(float(ys[0].min()), float(ys[1].min()))
        path.last_intervention = 1
        path.update_gaussian_process_of_last_intervention()
        pts, vals = path.compute_best_acquisition_values(best)
        choice = path.select_next_intervention(vals)
        return [p.tolist() for p in pts], [v.tolist() for v in vals], choice

    from cbo_with_oop_amd import _lib
    one_launch = run()
    ctx = forced_context(monkeypatch, CBO_HIP_SMALL_SETS=0)
    monkeypatch.setattr(_lib.Context, "get", classmethod(lambda cls, device_id=None: ctx))
    assert run() == one_launch


def test_trial_step_is_the_three_calls_in_one(hip):
    """CBOAcquisitionPath.trial_step = ONE cbo_trial_step call for what CBO.intervene() does between two observations
    (src/CBO.py:143-173): the rebuilt model of the set intervened on last, the sweep of every set, the pick.  Over a short
    trajectory on the toy graph (data of the chosen set growing by one observation per trial) it must return exactly what
    the three calls return on a twin path -- same device functions, same bits -- and pick what the oracle picks."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    rng = np.random.default_rng(4)
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]

    def fresh():
        xs = [rng0.uniform(-5, 5, (12, 1)), rng0.uniform(-5, 20, (12, 1))]
        ys = [targets[0](xs[0]), targets[1](xs[1])]
        path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, ToyGraph.get_cost_structure(1), "min", xs, ys,
                                  [ToyGraph.bounds(s) for s in es], grid_shapes=[[200], [200]], comm=None)
        path.update_all_gaussian_processes()
        return path, xs, ys

    rng0 = np.random.default_rng(4)
    one, xs1, ys1 = fresh()
    rng0 = np.random.default_rng(4)
    three, xs3, ys3 = fresh()
    grids = [meshgrid_candidates(ToyGraph.bounds(s), [200]) for s in es]
    for trial in range(8):
        best = min(float(ys1[0].min()), float(ys1[1].min()))
        a_x, a_y, (a_set, a_idx) = one.trial_step(best)
        if three.last_intervention is not None:
            three.update_gaussian_process_of_last_intervention()
        b_x, b_y = three.compute_best_acquisition_values(best)
        b_set, b_idx = three.select_next_intervention(b_y)
        assert a_idx == b_idx and a_set == b_set
        assert all(np.array_equal(p, q) for p, q in zip(a_x, b_x)) and all(np.array_equal(p, q) for p, q in zip(a_y, b_y))
        # the oracle's pick on the same data and grids
        vals = [O.acquisition_sweep(O.fit(xs1[s], ys1[s]), grids[s], best, cost=1.0)[1] for s in range(2)]
        assert O.select_next_intervention([np.array([[v]]) for v in vals]) == a_idx
        # intervene: the chosen set gains the point (both paths share the arrays' contents, not the objects)
        for xs, ys in ((xs1, ys1), (xs3, ys3)):
            xs[a_idx] = np.vstack([xs[a_idx], a_x[a_idx]])
            ys[a_idx] = np.vstack([ys[a_idx], targets[a_idx](a_x[a_idx])])
        assert one.last_intervention == a_idx
    # from the second trial on the one-call form was taken (the first builds the handle arrays through the three calls)
    assert one._call_cache.get("sweep_sets") is not None and one.models[a_idx].small


@pytest.mark.parametrize("causal,ard", [(False, False), (True, False), (False, True), (True, True)])
def test_trial_step_with_the_upload_folded_in_equals_the_three_calls(hip, causal, ard):
    """cbo_trial_step hands the refitted model's NEW data to the sweep's one launch through the staging buffer (every
    workgroup of the set prepares the points itself, the first one also fills the resident copies).  Against the explicit
    sequence cbo_gp_upload_data + cbo_acq_sweep_sets + cbo_argmax_sets on twin models: same winners, same values, same
    pick, bit for bit -- with prior closures (causal GP: prior mean and variance travel too), with per-dimension
    lengthscales (the points are scaled on the way), d = 3, and a model that grows across a 16-row tile boundary (63 -> 66
    observations).  Afterwards the resident copies serve a plain fit + predict exactly as uploaded data do."""
    import ctypes
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    rng = np.random.default_rng(17)
    d, sizes, cand_sizes = 3, [40, 63, 100], [200, 130, 300]
    mean_f = (lambda x: 0.3 * np.sin(x[:, :1]) + 0.1 * x[:, 1:2]) if causal else None
    var_f = (lambda x: 0.05 + 0.02 * np.cos(x[:, 2:3]) ** 2) if causal else None
    ls = np.array([0.8, 1.7, 1.2]) if ard else 1.3
    f = lambda x: np.sin(x).sum(1, keepdims=True) + 0.05 * rng.standard_normal((x.shape[0], 1))
    data = [rng.uniform(-3, 3, (n, d)) for n in sizes]
    obs = [f(x) for x in data]

    def build():
        models = [HipGaussianProcess(x, y, variance=1.4, lengthscale=ls, ard=ard, noise_var=1e-3, mean_function=mean_f,
                                     variance_adjustment=var_f, fit=False) for x, y in zip(data, obs)]
        grids = [CandidateGrid(g, m) for g, m in zip(cand_points, models)]
        return models, grids
    cand_points = [rng.uniform(-3, 3, (m, d)) for m in cand_sizes]
    one, one_grids = build()
    three, three_grids = build()
    S = len(sizes)
    arr = lambda objs: (ctypes.c_void_p * S)(*[o._handle for o in objs])
    y_best = np.full(S, min(float(y.min()) for y in obs))
    costs = np.array([1.0, 2.0, 3.0])
    for trial in range(5):
        r = 1 if trial < 3 else trial % S                       # set 1 grows 63 -> 64 -> 65 -> 66, then the others
        x_new = rng.uniform(-3, 3, (1, d))
        data[r] = np.vstack([data[r], x_new]); obs[r] = np.vstack([obs[r], f(x_new)])
        results = []
        for models, grids, fused in ((one, one_grids, True), (three, three_grids, False)):
            m = models[r]
            m._set_arrays(data[r], obs[r])
            pm, pv = m._prior(m.X)
            vals, idxs, chosen = np.empty(S), np.empty(S, dtype=np.int64), ctypes.c_int(-1)
            if fused:
                _lib.check(lib.cbo_trial_step(S, arr(models), arr(grids), r, m.X.shape[0], _lib.dptr(m.X), _lib.dptr(m._y_flat),
                                              _lib.dptr(pm), _lib.dptr(pv), _lib.dptr(y_best), 0, 0.0, _lib.dptr(costs),
                                              _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p), ctypes.byref(chosen)))
            else:
                _lib.check(lib.cbo_gp_upload_data(m._handle, m.X.shape[0], _lib.dptr(m.X), _lib.dptr(m._y_flat),
                                                  _lib.dptr(pm), _lib.dptr(pv)))
                _lib.check(lib.cbo_acq_sweep_sets(S, arr(models), arr(grids), _lib.dptr(y_best), 0, 0.0, _lib.dptr(costs),
                                                  _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)))
                _lib.check(lib.cbo_argmax_sets(_lib.dptr(vals), S, ctypes.byref(chosen)))
            m.stale = True
            results.append((vals.copy(), idxs.copy(), chosen.value))
        (va, ia, ca), (vb, ib, cb) = results
        assert np.array_equal(va, vb) and np.array_equal(ia, ib) and ca == cb, (trial, va, vb, ia, ib)
        # the oracle's winners on the same data
        for s in range(S):
            post = O.fit(data[s], obs[s], None if not causal else mean_f(data[s]), None if not causal else var_f(data[s]),
                         1.4, ls, 1e-3)
            _, val, idx, _, _ = O.acquisition_sweep(post, cand_points[s], float(y_best[s]),
                                                    None if not causal else mean_f(cand_points[s]),
                                                    None if not causal else var_f(cand_points[s]), "min", float(costs[s]))
            assert idx == ia[s] and np.isclose(val, va[s], rtol=1e-6, atol=1e-12), (trial, s, idx, ia[s], val, va[s])
    # a call the sweep would refuse is refused before the model's state moves to the new data
    m = one[0]
    n_before = lib.cbo_gp_n(m._handle)
    bigger = np.vstack([data[0], rng.uniform(-3, 3, (1, d))])
    pm_b, pv_b = (mean_f(bigger), var_f(bigger)) if causal else (None, None)
    vals, idxs, chosen = np.empty(S), np.empty(S, dtype=np.int64), ctypes.c_int(-1)
    rc = lib.cbo_trial_step(S, arr(one), arr(one_grids), 0, bigger.shape[0], _lib.dptr(bigger), _lib.dptr(np.zeros(bigger.shape[0])),
                            _lib.dptr(None if pm_b is None else np.ascontiguousarray(pm_b[:, 0])),
                            _lib.dptr(None if pv_b is None else np.ascontiguousarray(pv_b[:, 0])), _lib.dptr(y_best), 7, 0.0,
                            _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p), ctypes.byref(chosen))
    assert rc == _lib.CBO_ERR_INVALID
    assert lib.cbo_gp_n(m._handle) == n_before == data[0].shape[0]
    # the resident copies the launch filled: a plain fit + predict from them equals the uploaded twin's
    probe = rng.uniform(-3, 3, (9, d))
    for a, b in zip(one, three):
        (ma, sa), (mb, sb) = a.predict(probe), b.predict(probe)
        assert np.array_equal(ma, mb) and np.array_equal(sa, sb)
    for o in one_grids + three_grids + one + three:
        o.close()


def test_trial_step_at_the_edges_of_the_one_launch_path(hip):
    """cbo_trial_step where the folded-in upload does not apply or barely does: no set to refit (refit_set = -1), a model
    of one observation growing to two, and a model growing 127 -> 128 -> 129 observations -- the last step leaves the
    one-launch path (padded size 256: a plain upload, the general path for that set).  Always the three calls' answer."""
    import ctypes
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    rng = np.random.default_rng(23)
    f = lambda x: np.cos(x).sum(1, keepdims=True) + 0.05 * rng.standard_normal((x.shape[0], 1))
    for start, steps in ((1, 1), (127, 2)):
        data = [rng.uniform(-3, 3, (start, 2)), rng.uniform(-3, 3, (30, 2))]
        obs = [f(x) for x in data]
        cand = [rng.uniform(-3, 3, (150, 2)), rng.uniform(-3, 3, (70, 2))]
        twins = []
        for _ in range(2):
            models = [HipGaussianProcess(x, y, noise_var=1e-3, fit=False) for x, y in zip(data, obs)]
            twins.append((models, [CandidateGrid(c, m) for c, m in zip(cand, models)]))
        arr = lambda objs: (ctypes.c_void_p * 2)(*[o._handle for o in objs])
        y_best, costs = np.full(2, min(float(y.min()) for y in obs)), np.array([1.0, 2.0])

        def run(models, grids, fused, refit):
            vals, idxs, chosen = np.empty(2), np.empty(2, dtype=np.int64), ctypes.c_int(-1)
            m = models[0]
            if fused:
                _lib.check(lib.cbo_trial_step(2, arr(models), arr(grids), 0 if refit else -1, m.X.shape[0], _lib.dptr(m.X),
                                              _lib.dptr(m._y_flat), None, None, _lib.dptr(y_best), 0, 0.0, _lib.dptr(costs),
                                              _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p), ctypes.byref(chosen)))
            else:
                if refit:
                    _lib.check(lib.cbo_gp_upload_data(m._handle, m.X.shape[0], _lib.dptr(m.X), _lib.dptr(m._y_flat), None, None))
                _lib.check(lib.cbo_acq_sweep_sets(2, arr(models), arr(grids), _lib.dptr(y_best), 0, 0.0, _lib.dptr(costs),
                                                  _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)))
                _lib.check(lib.cbo_argmax_sets(_lib.dptr(vals), 2, ctypes.byref(chosen)))
            return vals, idxs, chosen.value

        for step in range(steps + 1):
            refit = step > 0
            if refit:
                x_new = rng.uniform(-3, 3, (1, 2))
                data[0] = np.vstack([data[0], x_new]); obs[0] = np.vstack([obs[0], f(x_new)])
                for models, _ in twins:
                    models[0]._set_arrays(data[0], obs[0])
            (va, ia, ca), (vb, ib, cb) = run(*twins[0], True, refit), run(*twins[1], False, refit)
            assert np.array_equal(va, vb) and np.array_equal(ia, ib) and ca == cb, (start, step, va, vb)
            assert lib.cbo_gp_n(twins[0][0][0]._handle) == data[0].shape[0]
            for s in range(2):
                _, val, idx, _, _ = O.acquisition_sweep(O.fit(data[s], obs[s], None, None, 1.0, 1.0, 1e-3), cand[s],
                                                        float(y_best[s]), None, None, "min", float(costs[s]))
                assert idx == ia[s] and np.isclose(val, va[s], rtol=1e-5, atol=1e-12), (start, step, s)
        for models, grids in twins:
            for o in grids + models:
                o.close()


def test_path_rebuilds_between_sweeps_never_reuse_destroyed_handles(hip):
    """A set rebuilt twice without a sweep in between (two observe trials in a row with one set, or closures that
    change twice): the multi-set call must be handed the handles of the objects that are alive now.  The cache of the
    handle arrays holds the models and grids themselves and is dropped on every rebuild; each round is checked against
    the oracle on that round's data."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    rng = np.random.default_rng(5)
    es = [["Z"]]
    xs = [rng.uniform(-5, 20, (30, 1))]
    ys = [ToyGraph.target_do_z(xs[0])]
    closures = [lambda x: np.zeros((x.shape[0], 1)), lambda x: np.zeros((x.shape[0], 1))]
    path = CBOAcquisitionPath(GaussianProcessType.CAUSAL_GP, es, ToyGraph.get_cost_structure(1), "min", xs, ys,
                              [ToyGraph.bounds(s) for s in es], mean_functions=[closures[0]], var_functions=[closures[1]],
                              grid_shapes=[[200]], comm=None)
    path.update_all_gaussian_processes()
    grid = meshgrid_candidates(ToyGraph.bounds(es[0]), [200])
    for rnd in range(6):
        best = float(path.data_y[0].min())
        pts, vals = path.compute_best_acquisition_values(best)
        _, val, idx, _, _ = O.acquisition_sweep(O.fit(path.data_x[0], path.data_y[0]), grid, best, cost=1.0)
        assert np.allclose(pts[0], grid[idx][None, :]) and np.isclose(vals[0][0, 0], val, rtol=1e-5, atol=1e-300)
        cached = path._call_cache["sweep_sets"]
        assert cached["models"][0] is path.models[0] and cached["handles"][0] == path.models[0]._handle.value
        # two rebuilds, no sweep between them: new closures force new model and grid objects each time
        for _ in range(2):
            x_add = rng.uniform(-5, 20, (1, 1))
            path.data_x[0] = np.vstack([path.data_x[0], x_add])
            path.data_y[0] = np.vstack([path.data_y[0], ToyGraph.target_do_z(x_add)])
            path.mean_functions[0] = lambda x: np.zeros((x.shape[0], 1))
            path.var_functions[0] = lambda x: np.zeros((x.shape[0], 1))
            path.last_intervention = 0
            if rnd % 2:
                path.update_gaussian_process_of_last_intervention()
            else:
                path.update_all_gaussian_processes()
            assert "sweep_sets" not in path._call_cache


class _RecordingComm:
    """Stand-in for sharding.Communicator in a single process: phase "record" keeps what this rank would contribute to
    each exchange; phase "replay" answers each exchange with the reduction over all ranks' recorded contributions."""

    def __init__(self, world, rank, records=None):
        self.world, self.rank, self.records, self.mine, self.calls = world, rank, records, [], 0

    def argmax(self, val, idx):
        from cbo_with_oop_amd.sharding import NO_CANDIDATE, reduce_pairs
        self.mine.append((val, idx))
        if self.records is None:
            return (val, idx) if idx != NO_CANDIDATE else (0.0, 0)
        pairs = [r[self.calls] for r in self.records]
        self.calls += 1
        pairs = [p for p in pairs if p[1] != NO_CANDIDATE]
        return reduce_pairs([p[0] for p in pairs], [p[1] for p in pairs])


@pytest.mark.parametrize("world", [2, 3, 8])
def test_path_placement_over_ranks_equals_single_process(hip, world):
    """CBOAcquisitionPath under a communicator: sets placed on ranks (6 complete-graph sets over 2 or 3 ranks) or
    candidate blocks of every set (8 ranks > 6 sets, some blocks ragged), one exchange per set -- every rank must end
    up with the single-process answer.  The ranks run one after the other in this process; the exchange is replayed
    from their recorded contributions (the real one is cbo_comm_argmax, test_communicator_through_the_c_abi)."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import CompleteGraph
    rng = np.random.default_rng(11)
    es = CompleteGraph.get_exploration_set("MIS")
    xs, ys = [], []
    for s in es:
        box = CompleteGraph.bounds(s)
        lo, hi = np.array([b[0] for b in box], float), np.array([b[1] for b in box], float)
        X = rng.uniform(lo, hi, (30 + 7 * len(xs), len(box)))
        xs.append(X)
        ys.append(np.sin(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((X.shape[0], 1)))
    shapes = [[37] if len(s) == 1 else [9, 7] for s in es]
    costs = CompleteGraph.get_cost_structure(3)                     # variable costs: the batch cost is the whole grid's
    best = min(float(y.min()) for y in ys)

    def run(comm):
        path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, costs, "min", xs, ys,
                                  [CompleteGraph.bounds(s) for s in es], grid_shapes=shapes, comm=comm)
        path.update_all_gaussian_processes()
        pts, vals = path.compute_best_acquisition_values(best)
        return [p.tolist() for p in pts], [float(v[0, 0]) for v in vals], path.placement()[0]

    single_pts, single_vals, mode = run(None)
    assert mode == "single"
    recorders = [_RecordingComm(world, r) for r in range(world)]
    for c in recorders:
        run(c)
    records = [c.mine for c in recorders]
    assert all(len(r) == len(es) for r in records)
    for r in range(world):
        pts, vals, mode = run(_RecordingComm(world, r, records))
        assert mode == ("sets" if len(es) >= world else "candidates")
        assert pts == single_pts
        assert np.allclose(vals, single_vals, rtol=1e-13, atol=0)


def test_path_failure_on_one_rank_reaches_every_rank(hip, monkeypatch):
    """Multi-rank CBOAcquisitionPath: a rank whose sweep raises still takes part in every exchange of the trial (with an
    error record) and re-raises afterwards; a rank that sees another rank's error record raises too -- nobody is left
    blocked in the all-gather."""
    from cbo_with_oop_amd import CBO as cbo_module, CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.sharding import ERROR_CANDIDATE
    rng = np.random.default_rng(2)
    es = ToyGraph.get_exploration_set("MIS")
    xs = [rng.uniform(-5, 5, (20, 1)), rng.uniform(-5, 20, (20, 1))]
    ys = [ToyGraph.target_do_x(xs[0]), ToyGraph.target_do_z(xs[1])]

    class Comm:
        def __init__(self, world, rank, poisoned=False):
            self.world, self.rank, self.poisoned, self.calls = world, rank, poisoned, []

        def argmax(self, val, idx):
            self.calls.append((val, idx))
            return (float("nan"), ERROR_CANDIDATE) if self.poisoned else (val, idx)

    class FlagComm(Comm):                       # a sharding.Communicator has max(): the failure travels as its own flag
        def __init__(self, world, rank, poisoned=False):
            super().__init__(world, rank, poisoned)
            self.flags = []

        def max(self, value):
            self.flags.append(value)
            return 1.0 if self.poisoned else value

    def make(comm):
        path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, ToyGraph.get_cost_structure(1), "min", xs, ys,
                                  [ToyGraph.bounds(s) for s in es], grid_shapes=[[64], [64]], comm=comm)
        path.update_all_gaussian_processes()
        return path

    # this rank fails: both exchanges still happen, with the error record, then the original exception surfaces
    comm = Comm(2, 0)
    path = make(comm)

    def boom(*a, **k):
        raise ValueError("sweep failed on this rank")
    monkeypatch.setattr(cbo_module, "find_next_y_points", boom)
    with pytest.raises(ValueError, match="sweep failed on this rank"):
        path.compute_best_acquisition_values(0.0)
    assert len(comm.calls) == len(es) and all(i == ERROR_CANDIDATE and np.isnan(v) for v, i in comm.calls)
    monkeypatch.undo()
    # another rank failed: this rank's own sweep is fine, the exchange returns the error record
    comm = Comm(2, 0, poisoned=True)
    path = make(comm)
    with pytest.raises(RuntimeError, match="another rank failed"):
        path.compute_best_acquisition_values(0.0)
    assert len(comm.calls) == len(es)
    # with the explicit flag (the real communicator): ONE flag exchange, then every rank raises before any arg-max exchange
    # -- a healthy rank's genuine NaN acquisition can no longer outvote an error record
    comm = FlagComm(2, 0)
    path = make(comm)
    monkeypatch.setattr(cbo_module, "find_next_y_points", boom)
    with pytest.raises(ValueError, match="sweep failed on this rank"):
        path.compute_best_acquisition_values(0.0)
    assert comm.flags == [1.0] and comm.calls == []
    monkeypatch.undo()
    comm = FlagComm(2, 0, poisoned=True)
    path = make(comm)
    with pytest.raises(RuntimeError, match="another rank failed"):
        path.compute_best_acquisition_values(0.0)
    assert comm.flags == [0.0] and comm.calls == []
    class HealthyComm(FlagComm):                # (the other rank's sets come back with a valid winner)
        def argmax(self, val, idx):
            from cbo_with_oop_amd.sharding import NO_CANDIDATE
            self.calls.append((val, idx))
            return (val, idx) if idx != NO_CANDIDATE else (0.0, 0)

    comm = HealthyComm(2, 0)                    # nobody failed: the flag exchange, then one arg-max exchange per set
    path = make(comm)
    path.compute_best_acquisition_values(0.0)
    assert comm.flags == [0.0] and len(comm.calls) == len(es)


def test_prediction_gradients_for_a_whole_grid(hip, monkeypatch):
    """cbo_gp_predict_gradients at M = 20480 points (forward sweep + backward substitution through the same strip kernel
    on the reversed factor), ARD lengthscales, against the oracle; then the same with the workspace cut into chunks."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(8)
    n, d, M = 500, 3, 20480
    X = rng.uniform(-4, 4, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))
    ls = np.array([1.3, 0.8, 2.0])
    kw = dict(variance=1.5, lengthscale=ls, ard=True, noise_var=1e-3)
    m = HipGaussianProcess(X, y, **kw)
    post = O.fit(X, y, variance=1.5, lengthscale=ls, noise_var=1e-3)
    Xs = rng.uniform(-4, 4, (M, d))
    dm, dv = m.get_prediction_gradients(Xs)
    scale_m, scale_v = None, None
    for a in range(0, M, 4096):
        dmo, dvo = O.predict_gradients(post, Xs[a:a + 4096])
        scale_m = max(scale_m or 0.0, np.max(np.abs(dmo)))
        scale_v = max(scale_v or 0.0, np.max(np.abs(dvo)))
        assert np.max(np.abs(dm[a:a + 4096] - dmo)) <= 1e-8 * scale_m
        assert np.max(np.abs(dv[a:a + 4096] - dvo)) <= 1e-7 * scale_v
    ctx2 = forced_context(monkeypatch, CBO_HIP_WORKSPACE_MB=16)       # 2 x 8 MiB workspaces: 2048-column chunks
    m2 = HipGaussianProcess(X, y, context=ctx2, **kw)
    dm2, dv2 = m2.get_prediction_gradients(Xs)
    assert np.array_equal(dm2, dm) and np.array_equal(dv2, dv)
    m2.close()
    ctx2.close()


def test_do_calculus_inputs_built_on_the_device(hip):
    """cbo_gp_predict_do (observed rows + candidate values expanded on the device) equals predict_grouped on the
    host-expanded (M * N_obs, d) array bit for bit, at a size where that array is a million rows."""
    from cbo_with_oop_amd.DoCalculus import intervened_inputs
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory, GaussianProcessType
    rng = np.random.default_rng(4)
    n_obs, d, m = 256, 3, 4096
    obs = rng.normal(size=(n_obs, d))
    yy = np.sin(obs).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n_obs, 1))
    gp = GaussianProcessFactory.create(GaussianProcessType.GRAPH_GP, obs, yy, [1.0, 1.0, 10.0, False])
    values = rng.uniform(-2, 2, (m, 2))
    index = [1, -1, 0]                                   # column 0 <- values[:, 1], column 2 <- values[:, 0]
    mean, var = gp.predict_do(obs, index, values)
    x = intervened_inputs(obs, index, values)
    assert x.shape == (m * n_obs, d)
    mean_h, var_h = gp.predict_grouped(x, n_obs)
    assert np.array_equal(mean, mean_h) and np.array_equal(var, var_h)
    post = O.fit(obs, yy, noise_var=1e-2)
    mo, vo = O.predict(post, x[:64 * n_obs])
    assert np.allclose(mean[:64, 0], mo.reshape(64, n_obs).mean(1), rtol=1e-9, atol=1e-12)
    assert np.allclose(var[:64, 0], vo.reshape(64, n_obs).mean(1), rtol=1e-7, atol=0)
    with pytest.raises(Exception):
        gp.predict_do(obs, [2, -1, 0], values)          # index beyond the columns of values
