"""GPU tests of the hyper-parameter-marginalised causal EI (cbo_acq_sweep_hyper, kernels_hyper.hip).

The contract is stated against the device's own per-sample route: acq_out = (((0 + a_0) + a_1) + ...) / H bit for bit, a_h
being what cbo_acq_sweep writes for a fresh model with sample h's hyper-parameters.  Accuracy is judged by
conftest.assert_parity against the mean over the samples of the fp64 oracle, the oracle's own error measured by the 80-bit
arbiter (the form tests/test_parity_gpu.py uses for cbo_acq_sweep's acq_out).

Shapes: n in {10, 17, 64, 128} (17: two tiles, a ragged last one; 128: a full block), m in {1, 64, 65, 200} (65 leaves a
workgroup one candidate) and 800 (13 candidate blocks: from 12 on the samples are factored by a first launch), d in {1, 3},
ARD and not, causal and plain, both tasks, an index offset, H in {1, 2, 3, 10}."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import assert_parity, load_fixture
from oracle import gp_oracle as O
from oracle.truth import truth_predict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def prior_mean(x):
    return 0.3 * np.sum(x, axis=1, keepdims=True)


def prior_var(x):
    return 0.2 + 0.1 * np.square(x[:, :1])


def problem(n, m, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.0, 2.0, (m, d))
    return X, y, Xs


def samples_for(d, ard, H, seed, own_first=False):
    """H rows of (variance, lengthscale x L, noise) spread by a factor of about 2 around (1.3, 0.8.., 2e-2); noise >= 1e-2."""
    rng = np.random.default_rng(1000 + seed)
    L = d if ard else 1
    base = np.concatenate([[1.3], np.linspace(0.8, 1.1, L), [2e-2]])
    rows = base * 2.0 ** rng.uniform(-1.0, 1.0, (H, L + 2))
    rows[:, -1] = np.maximum(rows[:, -1], 1e-2)
    if own_first:
        rows[0] = base
    return np.ascontiguousarray(rows)


def make_model(X, y, row, ard, causal, fit=True):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    kw = dict(variance=float(row[0]), lengthscale=row[1:-1].copy() if ard else float(row[1]), ard=ard,
              noise_var=float(row[-1]), fit=fit)
    if causal:
        kw.update(mean_function=prior_mean, variance_adjustment=prior_var)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def integrated(hip, model, rows, y_best, task):
    return hip.IntegratedHyperParameterAcquisition(
        model, lambda mdl: hip.CausalExpectedImprovement(y_best, task, mdl), samples=rows)


def per_sample_route(hip, X, y, Xs, rows, ard, causal, y_best, task, cost):
    """The loop the single call replaces, on the device: a fresh model per sample, its sweep, the sum in sample order."""
    total = np.zeros(Xs.shape[0])
    tries = []
    for row in rows:
        mh = make_model(X, y, row, ard, causal)
        tries.append(mh.jitter_tries)
        with np.errstate(invalid="ignore"):
            total = total + hip.CausalExpectedImprovement(y_best, task, mh).sweep(Xs, cost=cost, want_acq=True)["acq"][:, 0]
        mh.close()
    return total / rows.shape[0], tries


def first_argmax(v):
    """numpy.argmax: the first maximum, NaN maximal."""
    return int(np.argmax(v))


# (n, m, d, ard, causal, task, H, index_offset)
CASES = [
    (10, 1, 1, False, False, "min", 1, 0),
    (17, 65, 3, True, True, "min", 2, 1000),
    (64, 64, 1, False, True, "max", 10, 0),
    (128, 200, 3, True, False, "min", 2, 7),
    (17, 200, 3, False, False, "max", 10, 0),
    (128, 65, 1, True, True, "min", 10, 0),
    (50, 800, 3, True, True, "min", 3, 5),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n{}-m{}-d{}-{}-{}-{}-H{}-off{}".format(
    c[0], c[1], c[2], "ard" if c[3] else "iso", "causal" if c[4] else "plain", c[5], c[6], c[7]))
def test_equals_the_per_sample_route_bit_for_bit(hip, case):
    n, m, d, ard, causal, task, H, offset = case
    X, y, Xs = problem(n, m, d, seed=n + m)
    rows = samples_for(d, ard, H, seed=n)
    y_best, cost = float(y.min() if task == "min" else y.max()), 3.0
    want, _ = per_sample_route(hip, X, y, Xs, rows, ard, causal, y_best, task, cost)
    model = make_model(X, y, rows[0], ard, causal, fit=False)
    grid = hip.CandidateGrid(Xs, model, index_offset=offset)
    res = integrated(hip, model, rows, y_best, task).sweep(grid, cost=cost, want_acq=True)
    assert np.array_equal(res["acq"][:, 0], want)
    assert res["best_idx"] == first_argmax(want) + offset
    assert res["best_val"] == want[first_argmax(want)]
    # the winner alone (acq_out NULL) and determinism: the same bits again
    again = integrated(hip, model, rows, y_best, task).sweep(grid, cost=cost)
    assert again["acq"] is None and (again["best_val"], again["best_idx"]) == (res["best_val"], res["best_idx"])
    third = integrated(hip, model, rows, y_best, task).sweep(grid, cost=cost, want_acq=True)
    assert np.array_equal(third["acq"], res["acq"])
    grid.close(); model.close()


@pytest.mark.parametrize("case", [(10, 1, 1, False, False, "min"), (17, 65, 3, True, True, "max"),
                                  (128, 200, 3, True, False, "min"), (64, 800, 1, False, True, "min")],
                         ids=lambda c: "n{}-m{}-d{}".format(*c[:3]))
def test_one_sample_at_the_models_own_hyper_parameters_is_the_plain_sweep(hip, case):
    from cbo_with_oop_amd import _lib
    n, m, d, ard, causal, task = case
    X, y, Xs = problem(n, m, d, seed=3 * n + m)
    rows = samples_for(d, ard, 1, seed=n, own_first=True)
    y_best, cost = float(np.median(y)), 2.0
    model = make_model(X, y, rows[0], ard, causal)
    grid = hip.CandidateGrid(Xs, model, index_offset=11)
    plain = hip.CausalExpectedImprovement(y_best, task, model).sweep(grid, cost=cost, want_acq=True)
    res = integrated(hip, model, rows, y_best, task).sweep(grid, cost=cost, want_acq=True)
    assert np.array_equal(res["acq"], plain["acq"])
    assert (res["best_val"], res["best_idx"]) == (plain["best_val"], plain["best_idx"])
    # ... and cbo_acq_sweep_sets' winner (the LDS launch this kernel shares its device functions with)
    vals, idxs = np.empty(1), np.empty(1, dtype=np.int64)
    _lib.check(_lib.load().cbo_acq_sweep_sets(
        1, (ctypes.c_void_p * 1)(model._handle), (ctypes.c_void_p * 1)(grid._handle), _lib.dptr(np.array([y_best])),
        _lib.TASK_CODE[task], 0.0, _lib.dptr(np.array([cost])), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)))
    assert (res["best_val"], res["best_idx"]) == (vals[0], idxs[0])
    grid.close(); model.close()


@pytest.mark.parametrize("case", [(17, 65, 3, True, True, "min", 10), (64, 200, 1, False, False, "max", 2),
                                  (128, 64, 3, False, True, "min", 2)], ids=lambda c: "n{}-m{}-d{}-H{}".format(*c[:3], c[6]))
def test_against_the_mean_of_the_oracles_sweeps(hip, case):
    n, m, d, ard, causal, task, H = case
    X, y, Xs = problem(n, m, d, seed=7 * n + m)
    rows = samples_for(d, ard, H, seed=n + 1)
    y_best, cost = float(y.min() if task == "min" else y.max()), 3.0
    mX, vX, mXs, vXs = (prior_mean(X), prior_var(X), prior_mean(Xs), prior_var(Xs)) if causal else (None,) * 4
    oracle, truth = np.zeros(m), np.zeros(m)
    for row in rows:
        ls = row[1:-1] if ard else float(row[1])
        post = O.fit(X, y, mX, vX, variance=float(row[0]), lengthscale=ls, noise_var=float(row[-1]))
        assert post.tries == 0                                     # (noise >= 1e-2: the oracle itself is well conditioned)
        oracle += O.acquisition_sweep(post, Xs, y_best, mXs, vXs, task=task, cost=cost)[0][:, 0]
        mt, vt, _ = truth_predict(X, y, Xs, mX, vX, mXs, vXs, float(row[0]), ls, diag_add=float(row[-1]) + 1e-8,
                                  noise_var=float(row[-1]))
        truth += O.expected_improvement(mt, vt, y_best, task)[:, 0] / cost
    oracle, truth = oracle / H, truth / H
    model = make_model(X, y, rows[0], ard, causal, fit=False)
    res = integrated(hip, model, rows, y_best, task).sweep(Xs, cost=cost, want_acq=True)
    acq = res["acq"][:, 0]
    # EI inherits the posterior's error amplified by |u| when s is tiny; compare where EI is not negligible
    big = np.abs(oracle) > 1e-6 * np.max(np.abs(oracle))
    assert big.sum() >= 1
    assert_parity(acq[big], oracle[big], truth[big], f"marginalised acq {case}", rtol=1e-5, slack=8.0)
    assert res["best_idx"] == first_argmax(acq)
    model.close()


def test_nothing_of_a_small_model_or_its_candidates_is_touched(hip):
    from cbo_with_oop_amd import _lib
    n, m, d = 40, 130, 3
    X, y, Xs = problem(n, m, d, seed=5)
    rows = samples_for(d, True, 3, seed=2)
    own = samples_for(d, True, 1, seed=9)[0]
    y_best = float(y.min())
    # an unfitted model stays unfitted
    cold = make_model(X, y, own, True, True, fit=False)
    grid = hip.CandidateGrid(Xs, cold)
    res = integrated(hip, cold, rows, y_best, "min").sweep(grid, want_acq=True)
    assert cold.stale and np.all(np.isfinite(res["acq"]))
    rc = _lib.load().cbo_acq_sweep(cold._handle, grid._handle, y_best, 0, 0.0, 1.0, None, None, None,
                                   ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int64()))
    assert rc == _lib.CBO_ERR_NOT_FITTED
    grid.close(); cold.close()
    # a fitted one: sweep, posterior state and the kept solution are what they were; a twin that never saw the call agrees
    outs = []
    for call in (True, False):
        model = make_model(X, y, own, True, True)
        grid = hip.CandidateGrid(Xs, model, keep_solution=True)
        ei = hip.CausalExpectedImprovement(y_best, "min", model)
        before = ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True)
        state = [np.array(v) for v in model.posterior_state()]
        if call:
            integrated(hip, model, rows, y_best, "min").sweep(grid, cost=2.0, want_acq=True)
        after = ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True)
        for key in ("acq", "mean", "var"):
            assert np.array_equal(after[key], before[key])
        assert (after["best_val"], after["best_idx"]) == (before["best_val"], before["best_idx"])
        for u, v in zip(model.posterior_state(), state):
            assert np.array_equal(np.array(u), v)
        assert not model.stale
        assert model.append(np.array([0.25, -0.5, 1.0]), 0.7)          # the kept solution grows by one row
        outs.append(ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True))
        grid.close(); model.close()
    for key in ("acq", "mean", "var"):
        assert np.array_equal(outs[0][key], outs[1][key])


def test_the_general_path_answers_larger_models_and_restores_them(hip):
    n, m, d, ard, causal = 130, 130, 3, True, True
    X, y, Xs = problem(n, m, d, seed=21)
    rows = samples_for(d, ard, 2, seed=4)
    own = samples_for(d, ard, 1, seed=8)[0]
    y_best, cost = float(y.min()), 3.0
    want, _ = per_sample_route(hip, X, y, Xs, rows, ard, causal, y_best, "min", cost)
    model = make_model(X, y, own, ard, causal)
    grid = hip.CandidateGrid(Xs, model, index_offset=3)
    ei = hip.CausalExpectedImprovement(y_best, "min", model)
    before = ei.sweep(grid, cost=cost, want_acq=True, want_posterior=True)
    state = [np.array(v) for v in model.posterior_state()]
    res = integrated(hip, model, rows, y_best, "min").sweep(grid, cost=cost, want_acq=True)
    assert np.allclose(res["acq"][:, 0], want, rtol=1e-9, atol=0)
    assert res["best_idx"] == first_argmax(res["acq"][:, 0]) + 3
    assert res["best_val"] == res["acq"][res["best_idx"] - 3, 0]
    # hyper-parameters restored, fitted again (the sweep below would be refused otherwise): the same factor
    after = ei.sweep(grid, cost=cost, want_acq=True, want_posterior=True)
    for key in ("acq", "mean", "var"):
        assert np.array_equal(after[key], before[key])
    for u, v in zip(model.posterior_state(), state):
        assert np.array_equal(np.array(u), v)
    # an unfitted large model is answered too and stays unfitted
    cold = make_model(X, y, own, ard, causal, fit=False)
    res2 = integrated(hip, cold, rows, y_best, "min").sweep(Xs, cost=cost, want_acq=True)
    assert np.array_equal(res2["acq"], res["acq"]) and cold.stale
    grid.close(); model.close(); cold.close()


def test_a_sample_that_is_not_positive_definite_as_assembled_takes_the_general_path(hip):
    """The jitter fixture's duplicate rows under a sample whose variance (1e12) puts the rounding of the factorisation above
    the 1e-8 on the diagonal: the LDS launch meets a non-positive pivot and declines, the general path's jitchol ladder
    answers -- what a fresh model with that sample's hyper-parameters does on its own (its jitter_tries says so)."""
    f = load_fixture("jitter_ladder")
    X, y, Xs = f["X"], f["y"], f["Xs"]
    rows = np.array([[1.0, 1.0, 1e-2], [1e12, 1.0, 0.0]])
    y_best = float(f["y_best"])
    want, tries = per_sample_route(hip, X, y, Xs, rows, False, False, y_best, "min", 1.0)
    assert tries[0] == 0 and tries[1] >= 1
    model = make_model(X, y, rows[0], False, False)
    with np.errstate(invalid="ignore"):
        res = integrated(hip, model, rows, y_best, "min").sweep(Xs, want_acq=True)
    assert np.allclose(res["acq"][:, 0], want, rtol=1e-9, atol=0, equal_nan=True)
    assert res["best_idx"] == first_argmax(res["acq"][:, 0])
    assert not model.stale
    model.close()


def test_error_returns(hip):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    X, y, Xs = problem(12, 20, 2, seed=1)
    model = make_model(X, y, np.array([1.0, 1.0, 1e-2]), False, False, fit=False)
    grid = hip.CandidateGrid(Xs, model)
    other = hip.CandidateGrid(np.zeros((4, 3)))
    good = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 0.0]])
    acq = np.empty(20)
    bv, bi = ctypes.c_double(), ctypes.c_int64()

    def call(rows=good, n=None, cands=grid, task=0, cost=1.0, acq_out=acq, val=bv, idx=bi, gp=model):
        return lib.cbo_acq_sweep_hyper(gp._handle if gp is not None else None, cands._handle,
                                       rows.shape[0] if n is None else n, _lib.dptr(rows) if rows is not None else None,
                                       0.0, task, 0.0, cost, _lib.dptr(acq_out) if acq_out is not None else None,
                                       ctypes.byref(val) if val is not None else None,
                                       ctypes.byref(idx) if idx is not None else None)

    assert call() == _lib.CBO_OK
    assert call(acq_out=None) == _lib.CBO_OK and call(val=None, idx=None) == _lib.CBO_OK
    invalid = _lib.CBO_ERR_INVALID
    assert call(gp=None) == invalid and call(cands=other) == invalid and call(task=2) == invalid     # check_sweep_args
    assert call(n=0) == invalid and call(n=-1) == invalid
    assert call(rows=np.tile(good[:1], (257, 1))) == invalid and call(rows=np.tile(good[:1], (256, 1))) == _lib.CBO_OK
    assert call(rows=None, n=2) == invalid
    assert call(acq_out=None, val=None) == invalid and call(acq_out=None, idx=None) == invalid
    for cost in (0.0, -1.0, float("nan")):
        assert call(cost=cost) == invalid
    for col in (0, 1):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rows = good.copy()
            rows[1, col] = bad
            assert call(rows=rows) == invalid, (col, bad)
    for bad in (-1e-12, float("nan"), float("inf")):
        rows = good.copy()
        rows[0, 2] = bad
        assert call(rows=rows) == invalid, bad
    assert model.stale and call() == _lib.CBO_OK                   # never CBO_ERR_NOT_FITTED; the refusals left nothing behind
    grid.close(); other.close(); model.close()


def test_generate_hyperparameters_samples(hip):
    X, y, Xs = problem(20, 30, 1, seed=13)
    model = make_model(X, y, np.array([1.0, 1.0, 1e-2]), False, False)
    np.random.seed(5)
    samples = model.generate_hyperparameters_samples(n_samples=4, n_burnin=6, subsample_interval=2, step_size=0.05,
                                                     leapfrog_steps=4)
    assert samples.shape == (4, 3) and np.all(np.isfinite(samples)) and np.all(samples > 0)
    assert model.stale                                              # left at the chain's last state, unfitted
    acq = integrated(hip, model, samples, float(y.min()), "min").evaluate(Xs)
    assert acq.shape == (30, 1) and np.all(np.isfinite(acq)) and model.stale
    mean, var = model.predict(Xs)                                   # usable afterwards: the next use refits it
    assert np.all(np.isfinite(mean)) and np.all(var > 0) and not model.stale
    model.close()


def test_find_next_y_point_with_hyper_samples(hip):
    n, d = 17, 3
    X, y, Xs = problem(n, 65, d, seed=33)
    rows = samples_for(d, False, 3, seed=6)
    model = make_model(X, y, rows[0], False, True)
    y_best = float(y.min())
    costs = {"A": lambda col: 2.0, "B": lambda col: 1.0, "C": lambda col: 4.0}
    y_new, x_new = hip.find_next_y_point(None, model, y_best, ["A", "B", "C"], costs, candidates=Xs, hyper_samples=rows)
    res = integrated(hip, model, rows, y_best, "min").sweep(Xs, cost=7.0, want_acq=True)
    assert y_new.shape == (1, 1) and x_new.shape == (1, d)
    assert np.array_equal(x_new[0], Xs[res["best_idx"]]) and y_new[0, 0] == res["best_val"]
    model.close()
