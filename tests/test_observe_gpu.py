"""GPU tests of the observe step: the batched likelihood + gradients of many small models (one launch), the lockstep
hyper-parameter MLE of every graph-level GP, and the whole agent (``CBO.run``)."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def _model(rng, n, d, ard, noise=0.04, dup=False):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X = rng.uniform(-2, 2, (n, d))
    if dup:
        X[n // 2:] = X[:n - n // 2]                  # duplicated rows: Ky singular up to the noise
    y = np.sin(X[:, :1]) + 0.2 * X[:, -1:] + 0.05 * rng.standard_normal((n, 1))
    ls = np.linspace(0.7, 1.6, d) if ard else 0.9
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = HipGaussianProcess(X, y, ard=ard, variance=1.2, lengthscale=ls, noise_var=noise, fit=n > 128)
    return m, X, y, ls, noise


def _single(m):
    """cbo_gp_lml_gradients on the model alone: (lml, dv, dls, dn) or None (not positive definite)."""
    try:
        dv, dls, dn = m.log_likelihood_gradients()
    except np.linalg.LinAlgError:
        return None
    return m._last_lml, dv, dls, dn


def _unfitted(m):
    from cbo_with_oop_amd import _lib
    out = ctypes.c_double(0.0)
    return _lib.load().cbo_gp_log_marginal(m._handle, ctypes.byref(out)) == _lib.CBO_ERR_NOT_FITTED


def _bitwise(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3], (a, b)
    np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("k", [1, 8, 15, 21])
def test_batch_small_models_equal_one_model_alone(hip, k):
    """K small models of mixed n, d (1..8) and ARD in ONE launch: every model's outputs are the bits of
    cbo_gp_lml_gradients on it alone, within the oracle bar, and no model is fitted on the way."""
    from cbo_with_oop_amd.GaussianProcessFactory import lml_gradients_batch
    rng = np.random.default_rng(100 + k)
    specs = [(int(rng.integers(8, 129)), 1 + i % 8, i % 3 == 1) for i in range(k)]
    made = [_model(rng, n, d, ard) for n, d, ard in specs]
    models = [m for m, *_ in made]
    batch = lml_gradients_batch(models)
    assert all(_unfitted(m) and m.stale for m in models)
    for (m, X, y, ls, noise), got in zip(made, batch):
        _bitwise(got, _single(m))
        post = O.fit(X, y, variance=1.2, lengthscale=ls, noise_var=noise)
        o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
        scale = max(abs(o_dv), np.max(np.abs(o_dls)), abs(o_dn))
        assert got[0] == pytest.approx(O.log_marginal_likelihood(post), rel=1e-10)
        assert got[1] == pytest.approx(o_dv, rel=1e-8, abs=1e-10 * scale)
        assert got[3] == pytest.approx(o_dn, rel=1e-8, abs=1e-10 * scale)
        np.testing.assert_allclose(got[2], o_dls, rtol=1e-8, atol=1e-10 * scale)
    assert all(_unfitted(m) for m in models)
    for m in models:
        m.close()


def test_batch_mixed_large_and_not_positive_definite(hip):
    """In one batch with small models: a model above 256 observations (general path, fitted beforehand), a small
    model whose Ky is not positive definite as assembled but is after the jitchol ladder's first jitter (duplicated
    rows, noise -1e-6: an eigenvalue of about -1e-6), and one that no jitter of the ladder rescues (noise -0.5).  Each
    is answered as it would be alone, and the small ones keep their one-launch bits, unfitted."""
    from cbo_with_oop_amd.GaussianProcessFactory import lml_gradients_batch
    rng = np.random.default_rng(5)
    small = [_model(rng, 40 + 10 * i, 1 + i, i % 2 == 1) for i in range(4)]
    big = _model(rng, 300, 3, False)
    jittered = _model(rng, 60, 2, False, noise=-1e-6, dup=True)
    hopeless = _model(rng, 50, 2, False, noise=-0.5)
    made = small[:2] + [big, jittered] + small[2:] + [hopeless]
    models = [m for m, *_ in made]
    batch = lml_gradients_batch(models)
    assert not _unfitted(jittered[0])            # the one-launch factorisation failed: the ladder fitted the model
    assert batch[models.index(jittered[0])] is not None
    assert batch[models.index(hopeless[0])] is None
    assert all(_unfitted(m) for m, *_ in small)
    singles = [_single(m) for m in models]
    for got, want in zip(batch, singles):
        assert (got is None) == (want is None)
        if got is not None:
            _bitwise(got, want)
    m, X, y, ls, noise = big
    post = O.fit(X, y, variance=1.2, lengthscale=ls, noise_var=noise)
    assert batch[models.index(m)][0] == pytest.approx(O.log_marginal_likelihood(post), rel=1e-8)
    for m in models:
        m.close()


@pytest.mark.parametrize("k", [1, 6, 11])
def test_batch_two_block_models_against_oracle(hip, k):
    """Models of 128 < n <= 256 (mixed d and ARD, some with small ones in the same launch) go through the kernel's
    two-block form: likelihood and gradients within 1e-8 of the oracle, and no fit happened (the models are still
    unfitted afterwards)."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess, lml_gradients_batch
    rng = np.random.default_rng(300 + k)
    made = []
    for i in range(k):
        n = [129, 256, 200, 144, 177, 240][i % 6] if i % 4 != 3 else int(rng.integers(20, 129))
        d, ard = 1 + (2 * i) % 8, i % 2 == 0
        X = rng.uniform(-2, 2, (n, d))
        y = np.sin(X[:, :1]) + 0.2 * X[:, -1:] + 0.05 * rng.standard_normal((n, 1))
        ls = np.linspace(0.7, 1.6, d) if ard else 0.9
        m = HipGaussianProcess(X, y, ard=ard, variance=1.2, lengthscale=ls, noise_var=0.04, fit=False)
        made.append((m, X, y, ls))
    models = [m for m, *_ in made]
    batch = lml_gradients_batch(models)
    assert all(_unfitted(m) for m in models)
    for (m, X, y, ls), got in zip(made, batch):
        post = O.fit(X, y, variance=1.2, lengthscale=ls, noise_var=0.04)
        o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
        scale = max(abs(o_dv), np.max(np.abs(o_dls)), abs(o_dn))
        assert got[0] == pytest.approx(O.log_marginal_likelihood(post), rel=1e-8)
        assert got[1] == pytest.approx(o_dv, rel=1e-8, abs=1e-10 * scale)
        assert got[3] == pytest.approx(o_dn, rel=1e-8, abs=1e-10 * scale)
        np.testing.assert_allclose(got[2], o_dls, rtol=1e-8, atol=1e-10 * scale)
    for m in models:
        m.close()


def _observations(graph, n, seed):
    """n observational rows drawn from the graph's SEM with a fixed seed (a dict of columns)."""
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model
    sem = graph.define_sem()
    rng = np.random.default_rng(seed)
    rows = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(n)]
    return {v: np.array([r[v] for r in rows]) for v in rows[0] if not v.startswith("U")}


def _coral_like(n, seed):
    """Columns for the coral graphs' variables (their SEM is fitted to data this package does not load): smooth
    functions of a few latent draws, on the scales of the coral ranges."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 4))
    cols = {"N": z[:, 0], "L": np.abs(z[:, 1]) + 0.5, "TE": 0.3 * z[:, 1] + 0.1 * z[:, 2], "S": 0.5 * z[:, 2]}
    cols["C"] = 0.5 + 0.1 * np.tanh(cols["N"] + cols["L"])
    cols["T"] = 2.0 * cols["S"] + 0.3 * z[:, 3]
    cols["D"] = -1.0 * cols["S"] + 0.2 * z[:, 3]
    cols["O"] = 3.0 + 0.3 * np.sin(cols["T"]) + 0.1 * cols["D"]
    cols["Y"] = np.cos(cols["N"]) + 0.5 * cols["O"] - 0.2 * cols["C"] + 0.05 * z[:, 0] * z[:, 3]
    return cols


def _same_fits(a, b):
    assert list(a) == list(b)
    for name in a:
        ra, rb = a[name].optimization_result, b[name].optimization_result
        assert ra.nfev == rb.nfev and ra.nit == rb.nit and ra.status == rb.status, name
        np.testing.assert_array_equal(ra.x, rb.x, err_msg=name)
        assert ra.fun == rb.fun, name
        assert a[name].variance == b[name].variance, name
        np.testing.assert_array_equal(a[name].lengthscale, b[name].lengthscale, err_msg=name)


@pytest.mark.parametrize("n", [100, 200])
def test_fit_all_complete_graph_lockstep_equals_sequential(hip, n):
    """The complete graph's ten graph GPs: the lockstep fit gives every GP the hyper-parameters, evaluation count and
    likelihood of fitting it alone (``fit_gaussian_process`` one after another)."""
    from cbo_with_oop_amd.graphs import CompleteGraph
    g = CompleteGraph(_observations(CompleteGraph, n, seed=n))
    assert len(g.fit_dependencies) == 10
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lock = g.fit_all_gaussian_processes()
        seq = g.fit_all_gaussian_processes(lockstep=False)
    if n == 100:
        _same_fits(lock, seq)
    else:
        # above 128 rows the lockstep evaluations come from the two-block kernel, the sequential ones from a refit and
        # the general path: the same optimum to rounding
        for name in lock:
            assert lock[name].optimization_result.fun == pytest.approx(seq[name].optimization_result.fun, rel=1e-8)
            assert _unfitted(lock[name])                # evaluated without refits
    if n == 200:
        data = g.measurements
        for (name, m), deps, outp in zip(lock.items(), g.fit_dependencies, ["C"] + ["Y"] * 9):
            X = np.hstack([data[v] for v in deps])
            _, _, _, lml = O.optimize_hyperparameters(X, data[outp], variance=1.0, lengthscale=1.0, noise_var=1e-2,
                                                      fix_noise=True)
            assert -m.optimization_result.fun == pytest.approx(lml, rel=1e-5, abs=1e-5), name


def test_fit_all_coral_shapes(hip):
    """The coral graphs' fifteen dependency shapes (d up to 8, ARD on the first ones) at n = 100: lockstep equals
    sequential bit for bit, and every likelihood is the oracle MLE's within 1e-5."""
    from cbo_with_oop_amd.graphs import CoralGraph
    g = CoralGraph(_coral_like(100, seed=3))
    assert len(g.fit_dependencies) == 15
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lock = g.fit_all_gaussian_processes()
        seq = g.fit_all_gaussian_processes(lockstep=False)
    _same_fits(lock, seq)
    data = g.measurements
    for (name, m), deps, p in zip(lock.items(), g.fit_dependencies, g.fit_parameters):
        X = np.hstack([data[v] for v in deps])
        _, _, _, lml = O.optimize_hyperparameters(X, data["Y"], variance=1.0,
                                                  lengthscale=np.ones(X.shape[1]) if p[3] else 1.0, noise_var=1e-2,
                                                  fix_noise=True)
        assert -m.optimization_result.fun == pytest.approx(lml, rel=1e-5, abs=1e-5), name


def _agent(lockstep, causal_prior=False, sets="MIS"):
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import compute_interventions
    obs = _observations(CompleteGraph, 200, seed=11)
    init = {k: v[:100] for k, v in obs.items()}
    sem = CompleteGraph.define_sem()
    rng = np.random.default_rng(2)
    es = CompleteGraph.get_exploration_set(sets) if isinstance(sets, str) else sets
    data = []
    for s in es:
        lo, hi = np.array(CompleteGraph.bounds(s)).T
        x = rng.uniform(lo, hi, (5, len(s)))
        y = compute_interventions(sem, {v: "" for v in s}, x, target_variable="Y")
        data.append((x, y))
    grid = [[64] if len(s) == 1 else [24, 24] for s in es]
    return CBO(CompleteGraph, init, obs, data, exploration_set=sets, num_trials=12, initial_num_obs_samples=100,
               causal_prior=causal_prior, grid_shapes=grid, lockstep=lockstep)


def test_cbo_run_complete_graph_same_choices_as_sequential_fits(hip):
    """A seeded 12-trial run of the whole agent on the complete graph observes and intervenes, and makes the same
    choices (trial kinds, sets, values, best values, costs) as the same run with the graph GPs fitted one by one."""
    runs = []
    for lockstep in (True, False):
        np.random.seed(9)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            agent = _agent(lockstep)
            mon = agent.run()
        runs.append(mon)
    a, b = runs
    assert len(a.type_trial) == 12
    assert 0 in a.type_trial and 1 in a.type_trial
    assert a.type_trial == b.type_trial
    assert a.global_opt == b.global_opt and a.current_cost == b.current_cost
    for ca, cb in zip(a.chosen, b.chosen):
        assert (ca is None) == (cb is None)
        if ca is not None:
            assert ca[0] == cb[0]
            np.testing.assert_array_equal(ca[1], cb[1])


def test_causal_prior_names_the_missing_graph_gp(hip):
    """The complete graph fits no GP for the exploration set ['D']: the causal prior cannot be built, and the agent
    says which GP is missing before it changes anything."""
    with pytest.raises(KeyError, match="gp_D"):
        _agent(True, causal_prior=True)


def test_cbo_run_causal_prior_lockstep_and_sequential_fits_agree(hip):
    """With the causal prior on a set whose graph GP exists (['B'] -> gp_B), the do-calculus prior built on the
    observe step's graph GPs drives every acquisition: the seeded run with lockstep fits makes the choices of the run
    with sequential fits."""
    runs = []
    for lockstep in (True, False):
        np.random.seed(9)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            agent = _agent(lockstep, causal_prior=True, sets=[["B"]])
            mon = agent.run()
        assert agent.models[0].causal
        runs.append(mon)
    a, b = runs
    assert 0 in a.type_trial and 1 in a.type_trial
    assert a.type_trial == b.type_trial
    for ca, cb in zip(a.chosen, b.chosen):
        assert (ca is None) == (cb is None)
        if ca is not None:
            assert ca[0] == cb[0]
            np.testing.assert_allclose(ca[1], cb[1], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(a.global_opt, b.global_opt, rtol=1e-6, atol=1e-9)
