"""GPU tests of the one-launch HMC sampler (cbo_gp_hmc_sets).  The reference in every comparison is
``hmc_sample_from_draws`` driven by the model's own ``_objective`` -- one device likelihood launch per position, the host
sampler's path -- never the kernel under test.  Chains are 8 samples of 3 leapfrog steps unless said otherwise."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

NUM, ITERS = 8, 3
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def mean_fn(a):
    return 0.1 * a[:, :1]


def var_fn(a):
    return 0.2 + 0.1 * np.cos(a[:, -1:]) ** 2


# (n, d, ard, causal, fixed noise)
CASES = [(1, 1, False, False, False), (10, 1, False, False, False), (16, 2, False, False, True), (17, 4, True, True, False),
         (33, 8, False, False, False), (50, 2, True, False, True), (100, 3, True, False, False), (128, 3, False, True, False)]
# ... and the step sizes: 0.05 accepts all 8 samples of every case; the longer steps reject (2 of 8, 7 of 8, 2 of 8)
RUNS = [(c, 0.05) for c in CASES] + [(CASES[7], 0.2), (CASES[7], 0.1), (CASES[6], 0.2)]
ACCEPTED = {(CASES[7], 0.2): 2, (CASES[7], 0.1): 7, (CASES[6], 0.2): 2}
case_id = lambda c: "n{}-d{}-{}-{}-{}".format(c[0], c[1], "ard" if c[2] else "iso", "causal" if c[3] else "plain",   # noqa: E731
                                              "fixed" if c[4] else "noise")
run_id = lambda r: case_id(r[0]) + "-step{}".format(r[1])                                                           # noqa: E731


def make_model(case, fit=False, n=None, dtype=None, context=None):
    """tests/test_parity_gpu.py's small-model generator."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    n0, d, ard, causal, fixed = case
    n = n0 if n is None else n
    rng = np.random.default_rng(7 * n + d)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X[:, :1]) + 0.2 * X[:, -1:] + 0.05 * rng.standard_normal((n, 1))
    kw = dict(mean_function=mean_fn, variance_adjustment=var_fn) if causal else {}
    if dtype is not None:
        kw["dtype"] = dtype
    if context is not None:
        kw["context"] = context
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, ard=ard, variance=1.2, lengthscale=np.linspace(0.7, 1.6, d) if ard else 0.9,
                                  noise_var=0.04, fix_noise=fixed, fit=fit, **kw)


def start_of(case):
    n, d, ard, causal, fixed = case
    ls = np.linspace(0.7, 1.6, d) if ard else np.array([0.9])
    return np.concatenate([[1.2], ls, [] if fixed else [0.04]])


def draws_of(case, num=NUM):
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
    np.random.seed(1000 + case[0] + case[1])
    return hmc_draws(start_of(case).size, num)


def host_chain(model, theta0, draws, iters, step, perturb=None):
    """The reference: one likelihood launch per position.  perturb: a RandomState -- every position is evaluated at
    x (1 + 4 eps r), r uniform in [-1, 1]."""
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_sample_from_draws

    def objective(x):
        if perturb is not None:
            x = x * (1.0 + 4.0 * EPS * perturb.uniform(-1.0, 1.0, x.size))
        return model._objective(x, "logexp")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return hmc_sample_from_draws(objective, theta0, draws[0], draws[1], iters, step)


def device_chains(models, theta0s, draws, iters=ITERS, step=0.05):
    from cbo_with_oop_amd.GaussianProcessFactory import hmc_chains_device
    return hmc_chains_device(models, theta0s, draws, iters, step)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_REFERENCE = {}


def reference(run):
    """(rows, flags, k, measured deviation of the perturbed reference chains) of a run, computed once."""
    if run not in _REFERENCE:
        case, step = run
        model = make_model(case)
        theta0, draws = start_of(case), draws_of(case)
        rows, flags, ks = host_chain(model, theta0, draws, ITERS, step)
        worst = 0.0
        for seed in (1, 2, 3):
            moved, _, _ = host_chain(model, theta0, draws, ITERS, step, perturb=np.random.RandomState(seed))
            worst = max(worst, float(np.max(np.abs(moved - rows) / np.abs(rows))))
        model.close()
        _REFERENCE[run] = (rows, flags, ks, worst)
    return _REFERENCE[run]


# ---- 1. the device chain against the reference chain, same draws ------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_device_chain_decides_as_the_reference_chain_and_its_rows_agree_within_the_measured_bar(hip, run):
    """The bar: 64 times the largest relative deviation of the reference chain's rows when every position is evaluated at
    x (1 + 4 eps r) (three seeds), not below 1e-12 -- the device differs from the host by a few ulp in theta at every
    position (another log1p / exp) and in p.p; 4 ulp in x model that, 64 is the margin."""
    from cbo_with_oop_amd import _lib
    case, step = run
    rows, flags, ks, measured = reference(run)
    u = draws_of(case)[1]
    assert np.all(np.abs(u - ks) >= 1e-3), np.min(np.abs(u - ks))          # a condition of the comparison, not a skip
    if run in ACCEPTED:
        assert int(flags.sum()) == ACCEPTED[run]
    else:
        assert flags.all()
    model = make_model(case)
    out = device_chains([model], [start_of(case)], [draws_of(case)], ITERS, step)[0]
    model.close()
    assert out["status"] == _lib.HMC_OK
    assert np.array_equal(out["accept"], flags)
    bar = max(64.0 * measured, 1e-12)
    dev = float(np.max(np.abs(out["rows"] - rows) / np.abs(rows)))
    print(f"{run_id(run)}: perturbed reference {measured:.3e}, bar {bar:.3e}, device {dev:.3e}, accepted {int(flags.sum())}, "
          f"min|u-k| {np.min(np.abs(u - ks)):.3e}")
    assert dev <= bar, (dev, bar)


# ---- 2. the final state -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_final_state_is_what_the_likelihood_call_answers_at_the_final_theta(hip, case):
    model = make_model(case)
    out = device_chains([model], [start_of(case)], [draws_of(case)])[0]
    theta = out["theta"]
    assert np.array_equal(bits(theta), bits(out["rows"][-1]))               # the last row, accepted or not
    nl = model.lengthscale.size
    model.set_hyperparameters(theta[0], theta[1:1 + nl], model.noise_var if case[4] else theta[1 + nl], fit=False)
    dv, dls, dn = model.log_likelihood_gradients()
    want = np.concatenate([[dv], dls, [] if case[4] else [dn]])
    assert np.array_equal(bits(out["grad"]), bits(want)), (out["grad"], want)
    assert bits(out["lml"]) == bits(model._last_lml)
    model.close()


# ---- 3. reading only ----------------------------------------------------------------------------------------------------
def test_the_models_are_only_read(hip):
    from cbo_with_oop_amd import _lib
    case = CASES[3]                                                          # (17, 4, ARD, causal)
    theta0, draws = start_of(case), draws_of(case)
    # an unfitted model is answered and stays unfitted
    cold = make_model(case)
    first = device_chains([cold], [theta0], [draws])[0]
    assert first["status"] == _lib.HMC_OK and cold.stale
    Xs = np.random.default_rng(3).uniform(-2, 2, (70, case[1]))
    grid = hip.CandidateGrid(Xs, cold)
    rc = _lib.load().cbo_acq_sweep(cold._handle, grid._handle, 0.0, 0, 0.0, 1.0, None, None, None,
                                   ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int64()))
    assert rc == _lib.CBO_ERR_NOT_FITTED
    # a second identical call returns the same bits
    again = device_chains([cold], [theta0], [draws])[0]
    for key in ("rows", "theta", "grad"):
        assert np.array_equal(bits(first[key]), bits(again[key]))
    assert np.array_equal(first["accept"], again["accept"]) and bits(first["lml"]) == bits(again["lml"])
    grid.close(); cold.close()
    # a fitted one: hyper-parameters, fit state, the cached sweep and the kept solution are what they were
    outs = []
    for call in (True, False):
        model = make_model(case, fit=True)
        grid = hip.CandidateGrid(Xs, model, keep_solution=True)
        ei = hip.CausalExpectedImprovement(0.1, "min", model)
        before = ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True)
        state = [np.array(v) for v in model.posterior_state()]
        hyper = (model.variance, model.lengthscale.copy(), model.noise_var)
        if call:
            assert device_chains([model], [theta0], [draws])[0]["status"] == _lib.HMC_OK
        assert (model.variance, model.noise_var) == (hyper[0], hyper[2]) and np.array_equal(model.lengthscale, hyper[1])
        after = ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True)
        for key in ("acq", "mean", "var"):
            assert np.array_equal(after[key], before[key])
        for a, b in zip(model.posterior_state(), state):
            assert np.array_equal(np.array(a), b)
        assert not model.stale
        assert model.append(np.array([0.25, -0.5, 1.0, 0.5]), 0.7)           # the kept solution grows by one row
        outs.append(ei.sweep(grid, cost=2.0, want_acq=True, want_posterior=True))
        grid.close(); model.close()
    for key in ("acq", "mean", "var"):
        assert np.array_equal(outs[0][key], outs[1][key])


# ---- 4. independence from company ---------------------------------------------------------------------------------------
def test_a_models_rows_do_not_depend_on_the_other_models_of_the_call(hip):
    """Alone, among 3 and among 9 (beyond kSmallByValue = 8: the descriptors from the pinned array) -- models of different n,
    d, ARD, causal and sampled / fixed noise in one call."""
    from cbo_with_oop_amd import _lib
    cases = CASES + [CASES[1]]
    models = [make_model(c) for c in cases]
    theta0s, draws = [start_of(c) for c in cases], [draws_of(c) for c in cases]
    alone = [device_chains([m], [t], [dr])[0] for m, t, dr in zip(models, theta0s, draws)]
    nine = device_chains(models, theta0s, draws)
    three = device_chains(models[2:5], theta0s[2:5], draws[2:5])
    for got, want in list(zip(nine, alone)) + list(zip(three, alone[2:5])):
        assert got["status"] == want["status"] == _lib.HMC_OK
        for key in ("rows", "theta", "grad"):
            assert np.array_equal(bits(got[key]), bits(want[key]))
        assert np.array_equal(got["accept"], want["accept"]) and bits(got["lml"]) == bits(want["lml"])
    assert np.array_equal(bits(nine[8]["rows"]), bits(nine[1]["rows"]))     # the same model twice in one call
    for m in models:
        m.close()


# ---- 5. no leapfrog steps -----------------------------------------------------------------------------------------------
def test_without_leapfrog_steps_every_row_is_the_start(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, logexp_finv
    for case in (CASES[3], CASES[5]):
        model = make_model(case)
        theta0 = start_of(case)
        momenta, uniforms = draws_of(case)
        uniforms = uniforms.copy()
        uniforms[2], uniforms[5] = 1.0, 1.5                                  # u < 1 alone decides
        out = device_chains([model], [theta0], [(momenta, uniforms)], iters=0)[0]
        assert out["status"] == _lib.HMC_OK
        want = logexp_f(logexp_finv(theta0))
        assert np.all(out["rows"] == out["rows"][0])
        assert np.all(np.abs(out["rows"][0] - want) <= 2 * np.spacing(want))
        assert np.array_equal(out["accept"], uniforms < 1.0) and out["accept"].sum() == NUM - 2
        model.close()


# ---- 6. routing ---------------------------------------------------------------------------------------------------------
SHORT = dict(n_samples=4, n_burnin=6, subsample_interval=2, step_size=0.05, leapfrog_steps=4)


def host_sequence(models, **kw):
    """What generate_hyperparameters_samples_together promises for a model the launch does not answer: optimize_together,
    then per model the perturbation, the chain's draws and the host chain on them."""
    from cbo_with_oop_amd.GaussianProcessFactory import _objective_set, _optimizer_start, optimize_together
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
    optimize_together(models)
    num = kw["n_burnin"] + kw["n_samples"] * kw["subsample_interval"]
    starts = []
    for m in models:
        theta0 = _optimizer_start(m, "logexp")[0]
        starts.append((theta0 * (1.0 + 0.01 * np.random.randn(theta0.size)), hmc_draws(theta0.size, num)))
    out = []
    for m, (theta0, draws) in zip(models, starts):
        rows, _, _ = host_chain(m, theta0, draws, kw["leapfrog_steps"], kw["step_size"])
        _objective_set(m, rows[-1], fit=False)
        out.append(rows[kw["n_burnin"]::kw["subsample_interval"]])
    return out


def test_larger_and_fp32_models_are_declined_and_the_wrapper_answers_them_with_the_host_chain(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import generate_hyperparameters_samples_together
    case = CASES[1]
    build = lambda: [make_model(case), make_model(case, n=200), make_model(case, dtype="f32"), make_model(CASES[2])]   # noqa: E731
    models = build()
    cases = [case, case, case, CASES[2]]
    outs = device_chains(models, [start_of(c) for c in cases], [draws_of(c) for c in cases])
    assert [o["status"] for o in outs] == [_lib.HMC_OK, _lib.HMC_DECLINED, _lib.HMC_DECLINED, _lib.HMC_OK]
    for o in outs[1:3]:                                                       # nothing else written
        assert not o["rows"].any() and not o["accept"].any() and not o["theta"].any() and not o["grad"].any() and o["lml"] == 0
    alone = device_chains(models[3:], [start_of(CASES[2])], [draws_of(CASES[2])])[0]
    assert np.array_equal(bits(outs[3]["rows"]), bits(alone["rows"]))
    np.random.seed(21)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = generate_hyperparameters_samples_together(models, **SHORT)
        state = np.random.get_state()
        twins = build()
        np.random.seed(21)
        want = host_sequence(twins, **SHORT)
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
    for j in (1, 2):
        assert np.array_equal(bits(got[j]), bits(want[j])), j
        assert models[j].stale and np.array_equal(bits(models[j].lengthscale), bits(twins[j].lengthscale))
    for j in (0, 3):                                                          # the device's rows: the host's to rounding
        assert got[j].shape == want[j].shape and np.allclose(got[j], want[j], rtol=1e-6)
    with pytest.raises(RuntimeError, match="declined"):
        generate_hyperparameters_samples_together(models, host_fallback=False, **SHORT)
    for m in models + twins:
        m.close()


def duplicate_model(variance=1e12):
    """The jitter fixture's duplicated inputs under a variance that puts the factorisation's rounding above the 1e-8 on the
    diagonal, the noise fixed at 1e-12: Ky is not positive definite as assembled."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("jitter_ladder")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(f["X"], f["y"], variance=variance, lengthscale=1.0, noise_var=1e-12, fix_noise=True, fit=False)


def test_a_start_that_is_not_positive_definite_as_assembled_stops_the_chain_and_the_wrapper_repeats_it_on_the_host(
        hip, monkeypatch):
    import importlib
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
    gpf = importlib.import_module("cbo_with_oop_amd.GaussianProcessFactory")      # (the package exports the class by that name)
    model, good = duplicate_model(), make_model(CASES[1])
    theta0 = np.array([1e12, 1.0])
    np.random.seed(4)
    draws = hmc_draws(2, NUM)
    outs = device_chains([model, good], [theta0, start_of(CASES[1])], [draws, draws_of(CASES[1])])
    assert outs[0]["status"] == _lib.HMC_NOT_PD and outs[1]["status"] == _lib.HMC_OK
    alone = device_chains([good], [start_of(CASES[1])], [draws_of(CASES[1])])[0]
    assert np.array_equal(bits(outs[1]["rows"]), bits(alone["rows"]))        # the neighbour is answered as ever
    # the wrapper from that start (the optimiser would move it): the host chain's answer, ladder included
    monkeypatch.setattr(gpf, "optimize_together", lambda models, *a, **k: None)
    twin = duplicate_model()
    np.random.seed(8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = gpf.generate_hyperparameters_samples_together([model], **SHORT)[0]
        np.random.seed(8)
        want = host_sequence([twin], **SHORT)[0]
        assert np.array_equal(bits(got), bits(want)) and got.shape == (4, 2) and model.stale
        with pytest.raises(RuntimeError, match="positive definite"):
            gpf.generate_hyperparameters_samples_together([duplicate_model()], host_fallback=False, **SHORT)
    for m in (model, good, twin):
        m.close()


# ---- 7. invalid arguments -----------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_before_any_device_work(hip):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    case = CASES[3]
    model, other = make_model(case, fit=True), make_model(CASES[1])
    P = start_of(case).size
    state = [np.array(v) for v in model.posterior_state()]

    def call(n_models=None, gps=True, chains=True, status=True, models=(model,), null=None, **over):
        k = len(models)
        handles = (ctypes.c_void_p * k)(*[m._handle if m is not None else None for m in models])
        arr = (_lib.CboHmcChain * k)()
        keep = []
        for j, m in enumerate(models):
            size = over.get("n_params", P if m is not other else 3)
            num = over.get("num_samples", NUM)
            buf = dict(theta0=np.array(over.get("theta0", np.full(size, 0.8))), momenta=np.array(over.get("momenta", np.zeros(max(num, 1) * size))),
                       uniforms=np.array(over.get("uniforms", np.full(max(num, 1), 0.5))), rows_out=np.full(max(num, 1) * size, -7.0),
                       final_theta=np.full(size, -7.0), final_lml=np.full(1, -7.0), final_grad=np.full(size, -7.0))
            acc = np.full(max(num, 1), -7, dtype=np.int32)
            ch = arr[j]
            ch.n_params, ch.sample_noise, ch.num_samples = size, over.get("sample_noise", 1), num
            ch.hmc_iters, ch.stepsize = over.get("hmc_iters", ITERS), over.get("stepsize", 0.05)
            for name, a in buf.items():
                setattr(ch, name, None if name == null else _lib.dptr(a))
            ch.accept_out = None if null == "accept_out" else acc.ctypes.data_as(_lib.c_int_p)
            keep.append((buf, acc))
        st = np.full(k, -7, dtype=np.int32)
        rc = lib.cbo_gp_hmc_sets(k if n_models is None else n_models, handles if gps else None, arr if chains else None,
                                 st.ctypes.data_as(_lib.c_int_p) if status else None)
        if rc == _lib.CBO_ERR_INVALID:                                       # the outputs are untouched
            assert np.all(st == -7)
            for buf, acc in keep:
                assert np.all(acc == -7) and all(np.all(buf[name] == -7.0) for name in ("rows_out", "final_theta", "final_lml",
                                                                                       "final_grad"))
        return rc

    invalid = _lib.CBO_ERR_INVALID
    assert call() == _lib.CBO_OK
    assert call(gps=False) == invalid and call(chains=False) == invalid and call(status=False) == invalid
    assert call(models=(None,)) == invalid
    for name in ("theta0", "momenta", "uniforms", "rows_out", "accept_out", "final_theta", "final_lml", "final_grad"):
        assert call(null=name) == invalid, name
    assert call(n_models=0) == invalid and call(n_models=-2) == invalid
    assert call(num_samples=0) == invalid and call(num_samples=_lib.HMC_MAX_SAMPLES + 1) == invalid
    assert call(hmc_iters=-1) == invalid
    assert call(num_samples=_lib.HMC_MAX_SAMPLES, hmc_iters=_lib.HMC_MAX_EVALS // _lib.HMC_MAX_SAMPLES + 1) == invalid
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        assert call(stepsize=bad) == invalid, bad
        theta0 = np.full(P, 0.8)
        theta0[2] = bad
        assert call(theta0=theta0) == invalid, bad
    assert call(n_params=P - 1) == invalid and call(n_params=P + 1) == invalid      # a P that does not match the model
    assert call(sample_noise=0) == invalid and call(sample_noise=2) == invalid
    for bad in (float("nan"), float("inf")):
        momenta = np.zeros(NUM * P)
        momenta[-1] = bad
        uniforms = np.full(NUM, 0.5)
        uniforms[3] = bad
        assert call(momenta=momenta) == invalid and call(uniforms=uniforms) == invalid
    ctx = _lib.Context(model._ctx.device_id)
    try:
        stranger = make_model(CASES[1], context=ctx)
        other_rc = call(models=(other, stranger))
        assert other_rc == invalid and b"context" in lib.cbo_last_error()
        stranger.close()
    finally:
        ctx.close()
    # the models are what they were
    assert not model.stale and other.stale
    for a, b in zip(model.posterior_state(), state):
        assert np.array_equal(np.array(a), b)
    assert call() == _lib.CBO_OK
    model.close(); other.close()


# ---- 8. generate_hyperparameters_samples_together -----------------------------------------------------------------------
def test_the_wrapper_draws_as_the_per_model_sequence_and_leaves_every_model_at_its_last_row(hip):
    from cbo_with_oop_amd.GaussianProcessFactory import generate_hyperparameters_samples_together
    cases = [CASES[1], CASES[5], CASES[3]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        models = [make_model(c) for c in cases]
        np.random.seed(33)
        rows = generate_hyperparameters_samples_together(models, **SHORT)
        state = np.random.get_state()
        last = [(m.variance, m.lengthscale.copy(), m.noise_var) for m in models]
        for m, c, r in zip(models, cases, rows):
            assert r.shape == (4, start_of(c).size) and np.all(np.isfinite(r)) and np.all(r > 0)
            assert m.stale
        # the whole chains once more, step by step as the wrapper takes them: the rows returned are samples[6::2], and every
        # model sits at its chain's last row
        from cbo_with_oop_amd.GaussianProcessFactory import _optimizer_start, optimize_together
        from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
        again = [make_model(c) for c in cases]
        np.random.seed(33)
        optimize_together(again)
        theta0s, draws = [], []
        for m in again:
            theta0 = _optimizer_start(m, "logexp")[0]
            theta0s.append(theta0 * (1.0 + 0.01 * np.random.randn(theta0.size)))
            draws.append(hmc_draws(theta0.size, 6 + 4 * 2))
        full = device_chains(again, theta0s, draws, iters=4, step=0.05)
        for m, c, r, o in zip(models, cases, rows, full):
            assert np.array_equal(bits(r), bits(o["rows"][6::2]))
            nl = m.lengthscale.size
            assert m.variance == o["rows"][-1, 0] and np.array_equal(m.lengthscale, o["rows"][-1, 1:1 + nl])
            assert m.noise_var == (0.04 if c[4] else o["rows"][-1, 1 + nl])
        # the per-model sequence under the same seed leaves the generator where the one call left it
        twins = [make_model(c) for c in cases]
        np.random.seed(33)
        host = [t.generate_hyperparameters_samples(**SHORT) for t in twins]
        after = np.random.get_state()
        assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        for r, h in zip(rows, host):
            assert np.allclose(r, h, rtol=1e-6)                              # (the same chain to rounding)
        # sampler="device" on one model: that model's rows from the three-model call, the generator positioned alike
        solo = make_model(cases[1])
        np.random.seed(33)
        np.random.randn(start_of(cases[0]).size)                             # model 0's perturbation and draws
        hmc_draws(start_of(cases[0]).size, 6 + 4 * 2)
        got = solo.generate_hyperparameters_samples(sampler="device", **SHORT)
        assert np.array_equal(bits(got), bits(rows[1])) and solo.stale
        assert _optimizer_start(solo, "logexp")[0].tolist() == [last[1][0], *last[1][1]]
    for m in models + twins + again + [solo]:
        m.close()


# ---- 9. the agent -------------------------------------------------------------------------------------------------------
def toy_problem(n=12, seed=4):
    from cbo_with_oop_amd.graphs import ToyGraph
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-5, 5, (n, 1)), rng.uniform(-5, 20, (n, 1))]
    return es, targets, xs, ToyGraph.get_cost_structure(1)


def test_the_path_draws_every_sets_rows_in_one_call_and_the_rebuilt_sets_alone(hip, monkeypatch):
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType, _lib
    from cbo_with_oop_amd.graphs import ToyGraph
    lib = _lib.load()
    calls = []
    bound = lib.cbo_gp_hmc_sets
    monkeypatch.setattr(lib, "cbo_gp_hmc_sets", lambda n, *a: (calls.append(int(n)), bound(n, *a))[1])
    es, targets, xs, table = toy_problem()
    ys = [t(x) for t, x in zip(targets, xs)]
    np.random.seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys, [ToyGraph.bounds(s) for s in es],
                                  grid_shapes=[[64], [64]], comm=None, hyper_samples=3, hyper_sampler="device")
        path.update_all_gaussian_processes()
        assert calls == [2]                                                  # both sets' chains: one call
        assert all(r is not None and r.shape == (3, 3) and np.all(np.isfinite(r)) for r in path.hyper_rows)
        best = min(float(ys[0].min()), float(ys[1].min()))
        x_new, y_new = path.compute_best_acquisition_values(best)
        assert all(np.all(np.isfinite(x)) and np.all(np.isfinite(y)) for x, y in zip(x_new, y_new))
        a_set, a_idx = path.select_next_intervention(y_new)
        xs[a_idx] = np.vstack([xs[a_idx], x_new[a_idx]])
        ys[a_idx] = np.vstack([ys[a_idx], targets[a_idx](x_new[a_idx])])
        kept = [r.copy() for r in path.hyper_rows]
        path.last_intervention = a_idx
        path.update_gaussian_process_of_last_intervention()
        assert calls == [2, 1]                                               # the rebuilt set's chain alone
        assert np.array_equal(path.hyper_rows[1 - a_idx], kept[1 - a_idx])
        assert not np.array_equal(path.hyper_rows[a_idx], kept[a_idx])
        x_new, y_new = path.compute_best_acquisition_values(best)
        assert all(np.all(np.isfinite(y)) for y in y_new)


def test_the_agent_runs_with_the_device_sampler(hip):
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
    es, targets, xs, _ = toy_problem(n=6)
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=4, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, hyper_samples=2,
                    hyper_sampler="device")
        mon = agent.run()
    assert len(mon.type_trial) == 4 and agent.hyper_sampler == "device"
    assert all(r is not None and r.shape == (2, 3) and np.all(np.isfinite(r)) for r in agent.hyper_rows)
