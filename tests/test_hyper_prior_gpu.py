"""GPU tests of the hyper-parameter priors: ``cbo_gp_log_prior_batch`` against the host form, the stage
inside ``cbo_gp_hmc_sets`` / ``cbo_gp_mle_sets`` bit for bit against the likelihood call plus the prior call, the device
chain and search against the host references on the model's own ``_objective`` (one launch per evaluation, prior included),
the routes, and the agent.  Models have 1..50 observations in 1..3 dimensions; chains are 8 samples of 5 leapfrog steps,
searches at most 40 rounds.  The small-model generators, the host references and their perturbation are the ones of
tests/test_hmc_sets_gpu.py and tests/test_mle_sets_gpu.py; the rounding bar is tests/test_hyper_prior_host.py's."""
import ctypes
import warnings

import numpy as np
import pytest

import test_hmc_sets_gpu as H
import test_hyper_prior_host as HP
import test_mle_sets_gpu as M

pytestmark = pytest.mark.gpu

ROUNDS, NUM, ITERS, STEP = 40, 8, 5, 0.05
EPS = 2.0 ** -52
bits = M.bits


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def P_():
    from cbo_with_oop_amd.utils_functions import priors
    return priors


# (n, d, ard, causal, fixed noise) and the priors each model carries: every kind, both noise modes, ARD and causal
CASES = [(1, 1, False, False, False), (10, 1, False, False, False), (17, 3, True, True, False), (50, 2, True, False, True),
         (10, 2, False, False, True)]
case_id = M.case_id


def priors_of(case):
    pr = P_()
    table = {
        CASES[0]: {"variance": pr.Gamma.from_EV(1.0, 10.0), "lengthscale": pr.Gamma.from_EV(1.0, 10.0),
                   "noise_var": pr.Gamma.from_EV(1.0, 10.0)},
        CASES[1]: {"variance": pr.Gaussian(1.0, 1.0), "lengthscale": pr.LogGaussian(0.0, 1.0), "noise_var": pr.InverseGamma(3.0, 0.2)},
        CASES[2]: {"variance": pr.Gamma(2.0, 1.5), "lengthscale": pr.LogGaussian(0.2, 0.8)},
        CASES[3]: {"variance": pr.InverseGamma(2.5, 2.0), "lengthscale": pr.Gamma(3.0, 2.0)},
        CASES[4]: {"lengthscale": pr.Gaussian(1.0, 0.5)},
    }
    return table[case]


def make_model(case, priors=True, **kw):
    model = M.make_model(case, **kw)
    for name, prior in (priors_of(case) if priors is True else (priors or {})).items():
        model.set_prior(name, prior)
    return model


def start_of(case):
    n, d, ard, causal, fixed = case
    ls = np.linspace(0.7, 1.6, d) if ard else np.array([0.9])
    return np.concatenate([[1.2], ls, [] if fixed else [0.04]])


def draws_of(case, num=NUM):
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
    np.random.seed(2000 + case[0] + case[1])
    return hmc_draws(start_of(case).size, num)


def prior_at(model, theta):
    from cbo_with_oop_amd.GaussianProcessFactory import log_prior_batch
    return log_prior_batch([model], [theta])[0]


def device_priors(model):
    from cbo_with_oop_amd import _lib
    n = 2 + model.lengthscale.size
    out = (_lib.CboHyperPrior * n)()
    _lib.check(_lib.load().cbo_gp_get_priors(model._handle, n, out))
    return [(d.kind, d.p0, d.p1, d.constant) for d in out]


def row_terms(model, theta):
    """Per row entry: S of tests/test_hyper_prior_host.py's bar (0 where there is no prior)."""
    row = P_().per_parameter(model.priors, model.lengthscale.size, not model.fix_noise)
    return row, np.array([0.0 if p is None else float(HP.abs_terms(p, t) + HP.jac_terms(t)) for p, t in zip(row, theta)])


# ---- 5. the prior call ----------------------------------------------------------------------------------------------------
def test_the_prior_call_agrees_with_the_host_form_and_does_not_depend_on_the_other_models(hip):
    """Against ``log_prior_host`` (numpy's log / expm1) within 8 ulp of S: the device's log and expm1 are within 1 ulp as
    glibc's are, the arithmetic is the same -- the host test's derivation holds unchanged.  The gradient: 8 ulp of the sum of
    the absolute values of its terms, bounded here by |density gradient| + |Jacobian gradient| + the cancelling pair of the
    Gamma kinds ((a - 1) / theta and b; b / theta^2 and (a + 1) / theta) and of the LogGaussian (log theta and mu)."""
    from cbo_with_oop_amd.GaussianProcessFactory import log_prior_batch
    pr = P_()
    cases = CASES + CASES[:4]
    models = [make_model(c) for c in cases]
    rng = np.random.default_rng(12)
    thetas = [np.exp(rng.uniform(-3.0, 3.0, start_of(c).size)) for c in cases]
    thetas[1][0] = 40.0                                                       # above the Jacobian's limit
    alone = [log_prior_batch([m], [t])[0] for m, t in zip(models, thetas)]
    for m, t, (lp, grad) in zip(models, thetas, alone):
        row, S = row_terms(m, t)
        want, gwant = pr.log_prior_host(row, t)
        assert abs(lp - want) <= HP.BAR_ULPS * EPS * S.sum(), (lp, want)
        for k, p in enumerate(row):
            if p is None:
                assert grad[k] == 0.0 and not np.signbit(grad[k])
                continue
            cancel = {pr.Gamma: abs(p.p0 - 1.0) / t[k] + p.p1, pr.InverseGamma: p.p1 / t[k] ** 2 + (p.p0 + 1.0) / t[k],
                      pr.LogGaussian: ((abs(np.log(t[k])) + abs(p.p0)) / p.p1 ** 2 + 1.0) / t[k]}.get(type(p), 0.0)
            terms = abs(float(p.lnpdf_grad(t[k]))) + abs(float(pr.log_jacobian_grad(t[k]))) + cancel
            assert abs(grad[k] - gwant[k]) <= HP.BAR_ULPS * EPS * terms, (k, grad[k], gwant[k])
    three, nine = log_prior_batch(models[1:4], thetas[1:4]), log_prior_batch(models, thetas)
    for got, want in list(zip(three, alone[1:4])) + list(zip(nine, alone)):
        assert bits(got[0]) == bits(want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    # the model's own parameters where no row is given; a model without priors answers 0 and zeros
    own = log_prior_batch([models[1], models[3]])
    assert bits(own[0][0]) == bits(log_prior_batch([models[1]], [start_of(CASES[1])])[0][0])
    assert bits(models[1].log_prior()) == bits(own[0][0]) and np.array_equal(models[3].log_prior_gradients(), own[1][1])
    bare = make_model(CASES[1], priors=False)
    mixed = log_prior_batch([bare, models[2], bare], [None, thetas[2], thetas[1]])
    assert mixed[0][0] == 0.0 and not mixed[0][1].any() and mixed[2][0] == 0.0 and not mixed[2][1].any()
    assert bits(mixed[1][0]) == bits(alone[2][0]) and bare.log_prior() == 0.0
    lik = models[1].log_likelihood()
    assert models[1].objective_function() == -lik - models[1].log_prior() and bare.objective_function() == -bare.log_likelihood()
    for m in models + [bare]:
        m.close()


# ---- 6. the final states, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_final_states_are_the_likelihood_call_plus_the_prior_call_bit_for_bit(hip, case):
    model = make_model(case)
    chain = H.device_chains([model], [start_of(case)], [draws_of(case)], ITERS, STEP)[0]
    rng = np.random.default_rng(5)
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f
    starts = np.vstack([start_of(case)[None], logexp_f(rng.standard_normal((2, start_of(case).size)))])
    runs = M.device_runs([model], [starts], ROUNDS)[0]
    ends = [("chain", chain["theta"], chain["lml"], chain["grad"])]
    ends += [(f"run {s}", runs["theta"][s], runs["lml"][s], runs["grad"][s]) for s in range(3)]
    for what, theta, post, grad in ends:
        lml, dl = M.likelihood_at(model, case, theta)
        lp, dlp = prior_at(model, theta)
        assert bits(post) == bits(lml + lp), (what, post, lml, lp)
        assert np.array_equal(bits(grad), bits(dl + dlp)), (what, grad, dl, dlp)
        assert lp != 0.0 and np.any(dlp != 0.0)
    model.close()


# ---- 7. the trajectories ----------------------------------------------------------------------------------------------------
_CHAINS, _SEARCHES = {}, {}


def chain_reference(case):
    if case not in _CHAINS:
        model = make_model(case)
        theta0, draws = start_of(case), draws_of(case)
        rows, flags, ks = H.host_chain(model, theta0, draws, ITERS, STEP)
        worst = 0.0
        for seed in (1, 2, 3):
            moved, moved_flags, _ = H.host_chain(model, theta0, draws, ITERS, STEP, perturb=np.random.RandomState(seed))
            assert np.array_equal(moved_flags, flags), "a perturbed reference chain changed a decision: other draws for this case"
            worst = max(worst, float(np.max(np.abs(moved - rows) / np.abs(rows))))
        model.close()
        _CHAINS[case] = (rows, flags, ks, worst)
    return _CHAINS[case]


def search_reference(case):
    if case not in _SEARCHES:
        model = make_model(case)
        theta0 = start_of(case)
        ref = M.host_search(model, theta0, ROUNDS)
        worst, stable = 0.0, True
        for seed in (1, 2, 3):
            moved = M.host_search(model, theta0, ROUNDS, perturb=np.random.RandomState(seed))
            stable = stable and moved["decisions"] == ref["decisions"] and moved["status"] == ref["status"]
            worst = max(worst, float(np.max(np.abs(moved["theta"] - ref["theta"]) / np.abs(ref["theta"]))),
                        abs(moved["lml"] - ref["lml"]) / max(1.0, abs(ref["lml"])))
        model.close()
        _SEARCHES[case] = (ref, worst, stable)
    return _SEARCHES[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_device_chain_decides_as_the_reference_chain_on_the_posterior(hip, case):
    """tests/test_hmc_sets_gpu.py's bar: 64 times the largest relative deviation of the reference's rows under a 4-ulp
    perturbation of every position (three seeds), not below 1e-12; measured from the reference, never from the kernel."""
    from cbo_with_oop_amd import _lib
    rows, flags, ks, measured = chain_reference(case)
    u = draws_of(case)[1]
    assert np.all(np.abs(u - ks) >= 1e-3), np.min(np.abs(u - ks))            # a condition of the comparison, not a skip
    model = make_model(case)
    out = H.device_chains([model], [start_of(case)], [draws_of(case)], ITERS, STEP)[0]
    bare = make_model(case, priors=False)
    plain = H.device_chains([bare], [start_of(case)], [draws_of(case)], ITERS, STEP)[0]
    model.close(); bare.close()
    assert out["status"] == _lib.HMC_OK and np.array_equal(out["accept"], flags)
    bar = max(64.0 * measured, 1e-12)
    dev = float(np.max(np.abs(out["rows"] - rows) / np.abs(rows)))
    print(f"{case_id(case)}: perturbed reference {measured:.3e}, bar {bar:.3e}, device {dev:.3e}, accepted {int(flags.sum())}, "
          f"min|u-k| {np.min(np.abs(u - ks)):.3e}")
    assert dev <= bar, (dev, bar)
    assert not np.array_equal(out["rows"], plain["rows"])                     # the prior moved the chain


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_device_search_decides_as_the_reference_search_on_the_posterior(hip, case):
    """tests/test_mle_sets_gpu.py's bar, measured the same way."""
    ref, measured, stable = search_reference(case)
    assert stable, "a perturbed reference run changed a decision: choose another start for this case"
    model = make_model(case)
    out = M.device_runs([model], [start_of(case)], ROUNDS)[0]
    model.close()
    bar = max(64.0 * measured, 1e-12)
    dev_theta = float(np.max(np.abs(out["theta"][0] - ref["theta"]) / np.abs(ref["theta"])))
    dev_lml = abs(out["lml"][0] - ref["lml"]) / max(1.0, abs(ref["lml"]))
    print(f"{case_id(case)}: reference rounds {ref['rounds']} status {ref['status']} accepted {sum(ref['decisions'])}, "
          f"device rounds {out['rounds'][0]} status {out['status'][0]}, perturbed reference {measured:.3e}, bar {bar:.3e}, "
          f"device theta {dev_theta:.3e} posterior {dev_lml:.3e}, posterior {ref['lml']:.6f}")
    assert (int(out["rounds"][0]), int(out["status"][0])) == (ref["rounds"], ref["status"])
    assert dev_theta <= bar and dev_lml <= bar, (dev_theta, dev_lml, bar)


# ---- 8. what holds whatever the trajectory ------------------------------------------------------------------------------------
def test_a_search_never_ends_below_its_start_and_a_pgtol_end_has_a_small_posterior_gradient(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_gradfactor
    for case in CASES:
        model = make_model(case)
        theta0 = start_of(case)
        start = M.device_runs([model], [theta0], 0)[0]
        assert (int(start["status"][0]), int(start["rounds"][0])) == (_lib.REFINE_MAX_ROUNDS, 0)
        out = M.device_runs([model], [theta0], ROUNDS)[0]
        assert out["lml"][0] >= start["lml"][0] and 0 <= out["rounds"][0] <= ROUNDS
        if out["status"][0] == _lib.REFINE_PGTOL:
            _, dl = M.likelihood_at(model, case, out["theta"][0])
            _, dlp = prior_at(model, out["theta"][0])
            assert np.max(np.abs((dl + dlp) * logexp_gradfactor(out["theta"][0]))) <= 1e-5
        model.close()


def test_three_points_under_a_gamma_prior_have_a_map(hip):
    """Three observations and a free noise: the likelihood alone has flat directions, the posterior under Gamma.from_EV(1, 10)
    on all three parameters has a maximum the search reaches."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X = np.array([[-1.0], [0.2], [1.3]])
    y = np.array([[0.3], [-0.1], [0.4]])
    model = HipGaussianProcess(X, y, variance=1.0, lengthscale=1.0, noise_var=0.1, fit=False)
    for name in ("variance", "lengthscale", "noise_var"):
        model.set_prior(name, P_().Gamma.from_EV(1.0, 10.0))
    out = M.device_runs([model], [np.array([1.0, 1.0, 0.1])], ROUNDS)[0]
    print(f"three points: status {out['status'][0]} rounds {out['rounds'][0]} theta {out['theta'][0]} posterior {out['lml'][0]:.6f}")
    assert out["status"][0] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL)
    assert np.all(np.isfinite(out["theta"][0])) and np.all(out["theta"][0] > 0.0) and np.isfinite(out["lml"][0])
    model.close()


# ---- 9. no priors: today's bits ------------------------------------------------------------------------------------------------
def test_a_model_whose_priors_were_unset_gives_the_bits_of_one_that_never_had_any(hip):
    cases = [CASES[1], CASES[2], CASES[3]]
    for case in cases:
        touched, twin = make_model(case), make_model(case, priors=False)
        with_priors = M.device_runs([touched], [start_of(case)], ROUNDS)[0]
        touched.unset_priors()
        assert touched.priors == {} and all(d[0] == 0 for d in device_priors(touched))
        a, b = M.device_runs([touched], [start_of(case)], ROUNDS)[0], M.device_runs([twin], [start_of(case)], ROUNDS)[0]
        assert M.same_bits(a, b) and not M.same_bits(a, with_priors)
        ca = H.device_chains([touched], [start_of(case)], [draws_of(case)], ITERS, STEP)[0]
        cb = H.device_chains([twin], [start_of(case)], [draws_of(case)], ITERS, STEP)[0]
        for k in ("rows", "theta", "grad"):
            assert np.array_equal(bits(ca[k]), bits(cb[k]))
        assert bits(ca["lml"]) == bits(cb["lml"]) and np.array_equal(ca["accept"], cb["accept"])
        # ... and one name alone
        touched.set_prior("variance", P_().Gamma(2.0, 1.0))
        touched.set_prior("lengthscale", P_().Gamma(2.0, 1.0))
        touched.unset_priors("lengthscale")
        assert list(touched.priors) == ["variance"]
        touched.close(); twin.close()


def test_a_call_that_mixes_models_with_and_without_priors_answers_each_as_alone(hip):
    cases = [CASES[1], CASES[1], CASES[2], CASES[3], CASES[3], CASES[4], CASES[0], CASES[2], CASES[4]]   # nine: beyond kSmallByValue
    flags = [True, False, True, False, True, True, True, False, False]
    models = [make_model(c, priors=f) for c, f in zip(cases, flags)]
    theta0s = [start_of(c) for c in cases]
    draws = [draws_of(c) for c in cases]
    alone = [M.device_runs([m], [t], ROUNDS)[0] for m, t in zip(models, theta0s)]
    for got, want in list(zip(M.device_runs(models, theta0s, ROUNDS), alone)) + list(zip(M.device_runs(models[:3], theta0s[:3], ROUNDS), alone)):
        assert M.same_bits(got, want)
    chains_alone = [H.device_chains([m], [t], [d], ITERS, STEP)[0] for m, t, d in zip(models, theta0s, draws)]
    for got, want in zip(H.device_chains(models, theta0s, draws, ITERS, STEP), chains_alone):
        assert np.array_equal(bits(got["rows"]), bits(want["rows"])) and bits(got["lml"]) == bits(want["lml"])
    assert not M.same_bits(alone[0], alone[1]) and not M.same_bits(alone[3], alone[4])
    for m in models:
        m.close()


# ---- 10. the routes ------------------------------------------------------------------------------------------------------------
def test_larger_and_fp32_models_with_priors_take_the_host_route_with_the_same_priors(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import generate_hyperparameters_samples_together, logexp_finv, optimize_together
    case = CASES[1]
    build = lambda: [make_model(case, n=129), make_model(case, dtype="f32"), make_model(case)]   # noqa: E731
    models, twins = build(), build()
    runs = M.device_runs(models, [start_of(case)] * 3, ROUNDS)
    chains = H.device_chains(models, [start_of(case)] * 3, [draws_of(case)] * 3, ITERS, STEP)
    assert [r["declined"] for r in runs] == [True, True, False]
    assert [c["status"] for c in chains] == [_lib.HMC_DECLINED, _lib.HMC_DECLINED, _lib.HMC_OK]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = optimize_together(models, max_iters=ROUNDS, optimizer="device")
        want = optimize_together(twins[:2], max_iters=ROUNDS)
        for j in (0, 1):
            assert not hasattr(got[j], "optimizer") and got[j].fun == want[j].fun and np.array_equal(got[j].x, want[j].x)
            # fun is the objective: the negative log posterior at x, prior included
            lp = models[j].log_prior()
            assert lp != 0.0 and np.isclose(got[j].fun, -models[j].log_likelihood() - lp, rtol=1e-9)
        assert got[2].optimizer == "device"
        alone = make_model(case, n=129)                                       # _objective alone sees the same posterior
        f, _ = alone._objective(logexp_finv(start_of(case)), "logexp")
        alone.set_hyperparameters(1.2, 0.9, 0.04)
        assert np.isclose(f, -alone.log_likelihood() - alone.log_prior(), rtol=1e-9) and alone.log_prior() != 0.0
        for m in models + twins:
            m.close()
        models, twins = build(), build()
        np.random.seed(21)
        drawn = generate_hyperparameters_samples_together(models, **H.SHORT)
        np.random.seed(21)
        ref = H.host_sequence(twins, **H.SHORT)
    for j in (0, 1):
        assert np.array_equal(bits(drawn[j]), bits(ref[j])), j
    assert drawn[2].shape == ref[2].shape and np.allclose(drawn[2], ref[2], rtol=1e-6)
    for m in models + twins + [alone]:
        m.close()


def test_optimize_restarts_keeps_the_highest_posterior_and_draws_from_the_priors(hip):
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, logexp_finv
    case = CASES[1]                                                           # P = 3: Gaussian, LogGaussian, InverseGamma
    model, twin = make_model(case), make_model(case)
    np.random.seed(17)
    res = model.optimize_restarts(num_restarts=4, max_iters=ROUNDS)
    state = np.random.get_state()
    np.random.seed(17)
    rows = [start_of(case)]
    for _ in range(3):
        x = np.random.randn(3)
        v = np.random.randn(1) * 1.0 + 1.0
        if v[0] > 0.0:
            x[0] = logexp_finv(v)[0]
        x[1] = logexp_finv(np.exp(np.random.randn(1) * 1.0 + 0.0))[0]
        x[2] = logexp_finv(1.0 / np.random.gamma(shape=3.0, scale=1.0 / 0.2, size=1))[0]
        rows.append(logexp_f(x))
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    out = M.device_runs([twin], [np.array(rows)], ROUNDS)[0]
    best = int(np.nanargmax(out["lml"]))
    assert res.best_run == best and len(res.runs) == 4 and res.fun == -out["lml"][best]
    for s, run in enumerate(res.runs):
        assert bits(run["lml"]) == bits(out["lml"][s]) and np.array_equal(bits(run["theta"]), bits(out["theta"][s]))
    theta = out["theta"][best]
    assert model.variance == theta[0] and model.lengthscale[0] == theta[1] and model.noise_var == theta[2]
    model.close(); twin.close()


# ---- 11. reading only; the priors stay -------------------------------------------------------------------------------------------
def test_the_models_are_only_read_and_data_changes_keep_the_priors(hip):
    case = CASES[2]                                                           # (17, 3, ARD, causal)
    Xs = np.random.default_rng(3).uniform(-2, 2, (40, case[1]))
    model = make_model(case, fit=True)
    before = model.predict(Xs)
    state = [np.array(v) for v in model.posterior_state()]
    hyper = (model.variance, model.lengthscale.copy(), model.noise_var)
    kept = device_priors(model)
    assert [k[0] for k in kept] == [3, 2, 2, 2, 0] and kept[1][1:3] == (0.2, 0.8)
    M.device_runs([model], [start_of(case)], ROUNDS)
    H.device_chains([model], [start_of(case)], [draws_of(case)], ITERS, STEP)
    prior_at(model, 2.0 * start_of(case))
    assert not model.stale and device_priors(model) == kept
    assert (model.variance, model.noise_var) == (hyper[0], hyper[2]) and np.array_equal(model.lengthscale, hyper[1])
    for a, b in zip(model.predict(Xs), before):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(model.posterior_state(), state):
        assert np.array_equal(np.array(a), b)
    lp = model.log_prior()
    rng = np.random.default_rng(9)
    X2 = rng.uniform(-2, 2, (12, case[1]))
    y2 = np.sin(X2[:, :1])
    model.set_data(X2, y2)
    assert device_priors(model) == kept and bits(model.log_prior()) == bits(lp)
    model.set_data(np.vstack([X2, X2[:1] + 0.1]), np.vstack([y2, y2[:1]]))      # (grows by one row: the append route)
    model.set_hyperparameters(0.7, np.full(3, 1.1), 0.02)
    assert device_priors(model) == kept and model.log_prior() != lp
    model.rebuild(X2, y2)
    assert device_priors(model) == kept and bits(model.log_prior()) == bits(lp) and list(model.priors) == ["variance", "lengthscale"]
    model.close()


def test_the_library_refuses_bad_descriptors_before_any_device_work(hip):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    model = make_model(CASES[1])
    kept = device_priors(model)
    D = _lib.CboHyperPrior

    def call(descs, n=None):
        arr = (D * len(descs))(*descs)
        return lib.cbo_gp_set_priors(model._handle, len(descs) if n is None else n, arr)
    good = D(_lib.PRIOR_GAMMA, 0, 2.0, 1.0, 0.0)
    none = D()
    nan, inf = float("nan"), float("inf")
    for bad, word in ((D(9, 0, 1.0, 1.0, 0.0), b"kind"), (D(-1, 0, 1.0, 1.0, 0.0), b"kind"),
                      (D(_lib.PRIOR_GAUSSIAN, 0, 0.0, 0.0, 0.0), b"sigma"), (D(_lib.PRIOR_LOGGAUSSIAN, 0, 0.0, -1.0, 0.0), b"sigma"),
                      (D(_lib.PRIOR_GAMMA, 0, 0.0, 1.0, 0.0), b"a must"), (D(_lib.PRIOR_INVGAMMA, 0, 1.0, 0.0, 0.0), b"b must"),
                      (D(_lib.PRIOR_GAMMA, 0, nan, 1.0, 0.0), b"finite"), (D(_lib.PRIOR_GAUSSIAN, 0, 0.0, inf, 0.0), b"finite"),
                      (D(_lib.PRIOR_GAMMA, 0, 1.0, 1.0, nan), b"constant")):
        assert call([good, bad, none]) == _lib.CBO_ERR_INVALID and word in lib.cbo_last_error(), lib.cbo_last_error()
        assert device_priors(model) == kept                                   # a refused call changes nothing
    assert call([good, none]) == _lib.CBO_ERR_INVALID and call([good, none, none, none]) == _lib.CBO_ERR_INVALID
    assert call([good, none, none]) == _lib.CBO_OK and device_priors(model)[0] == (_lib.PRIOR_GAMMA, 2.0, 1.0, 0.0)
    assert call([none, none, none]) == _lib.CBO_OK and all(d[0] == 0 for d in device_priors(model))
    assert call([good, none, none]) == _lib.CBO_OK and lib.cbo_gp_set_priors(model._handle, 3, None) == _lib.CBO_OK
    assert all(d[0] == 0 for d in device_priors(model))
    # the wrapper: a prior on a fixed noise, and transform="log" with priors
    fixed = make_model(CASES[4])
    with pytest.raises(ValueError, match="fixed"):
        fixed.set_prior("noise_var", P_().Gamma(1.0, 1.0))
    with pytest.raises(ValueError, match="logexp"):
        fixed.optimize(transform="log")
    with pytest.raises(ValueError):
        fixed.set_prior("period", P_().Gamma(1.0, 1.0))
    assert list(fixed.priors) == ["lengthscale"]
    th = np.array([1.0, nan, 1.0])
    ptr = (_lib.c_double_p * 1)(ctypes.cast(_lib.dptr(th), _lib.c_double_p))
    h = (ctypes.c_void_p * 1)(model._handle)
    lp, grad, st = np.zeros(1), np.zeros(_lib.HMC_MAX_PARAMS), np.zeros(1, dtype=np.int32)
    assert lib.cbo_gp_log_prior_batch(1, h, ptr, _lib.dptr(lp), _lib.dptr(grad), st.ctypes.data_as(_lib.c_int_p)) == _lib.CBO_ERR_INVALID
    model.close(); fixed.close()


# ---- 12. the agent -------------------------------------------------------------------------------------------------------------
def toy_agent(**kw):
    """tests/test_mle_sets_gpu.py's toy agent, three trials."""
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model

    class Toy(ToyGraph):
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
    rng = np.random.default_rng(4)
    xs = [rng.uniform(-5, 5, (6, 1)), rng.uniform(-5, 20, (6, 1))]
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=3, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, **kw)
        return agent, agent.run()


def agent_priors():
    pr = P_()
    return {"variance": pr.Gamma.from_EV(1.0, 10.0), "lengthscale": pr.Gamma.from_EV(1.0, 10.0), "noise_var": pr.Gamma.from_EV(0.1, 1.0)}


def test_the_agent_runs_with_priors_and_every_rebuilt_model_carries_them(hip, monkeypatch):
    from cbo_with_oop_amd import _lib
    F = __import__("importlib").import_module("cbo_with_oop_amd.GaussianProcessFactory")
    built = []
    create = F.GaussianProcessFactory.create

    def recording(*a, **kw):
        model = create(*a, **kw)
        built.append((model, kw.get("priors")))
        return model
    monkeypatch.setattr(F.GaussianProcessFactory, "create", staticmethod(recording))
    agent, mon = toy_agent(hyper_priors=agent_priors(), mle_optimizer="device", hyper_sampler="device", hyper_samples=3)
    assert len(mon.type_trial) == 3
    with_priors = [m for m, p in built if p]
    assert len(with_priors) >= 2 and all(p == agent_priors() for m, p in built if p)
    want = [(d.kind, d.p0, d.p1, d.constant) for d in (agent_priors()[k].descriptor() for k in ("variance", "lengthscale", "noise_var"))]
    for m in agent.models:                                                    # every exploration-set model, rebuilt ones included
        assert m.priors == agent_priors() and device_priors(m) == want
    for gp in agent.graph_gps.values():                                       # the graph GPs take none
        assert gp.priors == {}
    assert all(r is not None and r.shape == (3, 3) and np.all(np.isfinite(r)) for r in agent.hyper_rows)
    assert all(np.all(np.isfinite(np.asarray(y, dtype=np.float64))) for y in agent.data_y)


def test_the_agent_without_priors_records_what_it_recorded_before(hip):
    kw = dict(mle_optimizer="device", hyper_sampler="device", hyper_samples=3)
    plain, mon_plain = toy_agent(**kw)
    none, mon_none = toy_agent(hyper_priors=None, **kw)
    for a, b in zip(plain.data_x + plain.data_y, none.data_x + none.data_y):
        assert np.array_equal(bits(a), bits(b))
    assert mon_plain.type_trial == mon_none.type_trial
    assert mon_plain.global_opt == mon_none.global_opt and mon_plain.current_cost == mon_none.current_cost
    assert mon_plain.current_best_y == mon_none.current_best_y and mon_plain.feasible == mon_none.feasible
    assert len(mon_plain.chosen) == len(mon_none.chosen) == 3
    for a, b in zip(mon_plain.chosen, mon_none.chosen):
        assert (a is None) == (b is None)
        if a is not None:
            assert a[0] == b[0] and np.array_equal(bits(a[1]), bits(b[1]))
    assert none.hyper_priors is None and all(m.priors == {} for m in none.models)
