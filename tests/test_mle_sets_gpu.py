"""GPU tests of the one-launch hyper-parameter MLE (cbo_gp_mle_sets).  The reference in every comparison is
``lockstep_lbfgs`` with an infinite box driven by the model's own ``_objective`` -- one device likelihood launch per
evaluation -- never the kernel under test.  Searches take at most 40 rounds unless said otherwise."""
import ctypes
import importlib
import warnings

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

ROUNDS = 40
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


# (n, d, ard, causal, fixed noise): tests/test_hmc_sets_gpu.py's models -- one tile, a ragged last tile, all eight tiles,
# D = 1..8 through CBO_FOR_DIM, P from 2 to 10, both noise modes
CASES = [(1, 1, False, False, False), (10, 1, False, False, False), (16, 2, False, False, True), (17, 4, True, True, False),
         (33, 8, False, False, False), (50, 2, True, False, True), (100, 3, True, False, False), (128, 3, False, True, False)]
case_id = lambda c: "n{}-d{}-{}-{}-{}".format(c[0], c[1], "ard" if c[2] else "iso", "causal" if c[3] else "plain",   # noqa: E731
                                              "fixed" if c[4] else "noise")


def make_model(case, fit=False, n=None, dtype=None, context=None):
    """tests/test_hmc_sets_gpu.py's small-model generator."""
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
    """The searches' start: the model's own parameters -- halved for the 128-row case, where from the model's own the
    reference changes a decision under the bar's perturbation (40 rounds against 37: a start the comparison cannot use)."""
    n, d, ard, causal, fixed = case
    ls = np.linspace(0.7, 1.6, d) if ard else np.array([0.9])
    return np.concatenate([[1.2], ls, [] if fixed else [0.04]]) * (0.5 if n == 128 else 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_runs(models, theta0s, max_rounds=ROUNDS):
    from cbo_with_oop_amd.GaussianProcessFactory import mle_runs_device
    return mle_runs_device(models, theta0s, max_rounds)


def same_bits(a, b):
    return (np.array_equal(a["status"], b["status"]) and np.array_equal(a["rounds"], b["rounds"])
            and all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("theta", "lml", "grad")))


def likelihood_at(model, case, theta):
    """(lml, dlml / dtheta) by cbo_gp_lml_gradients at theta."""
    nl = model.lengthscale.size
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model.set_hyperparameters(theta[0], theta[1:1 + nl], model.noise_var if case[4] else theta[1 + nl], fit=False)
        dv, dls, dn = model.log_likelihood_gradients()
    return model._last_lml, np.concatenate([[dv], dls, [] if case[4] else [dn]])


def host_search(model, theta0, max_rounds=ROUNDS, perturb=None, objective=None):
    """The reference: ``lockstep_lbfgs`` without a box on the model's ``_objective``, one likelihood launch per evaluation.
    Returns dict(theta, lml, rounds, status, decisions, trials).  perturb: a RandomState -- every evaluation is taken at
    x (1 + 4 eps r), r uniform in [-1, 1].  The status is read off the recorded values with lockstep_lbfgs' own
    expressions (it does not say why it stopped)."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, logexp_finv
    from cbo_with_oop_amd.utils_functions.causal_optimizer import lockstep_lbfgs
    trials = []
    objective = objective or (lambda x: model._objective(x, "logexp"))

    def fun(X):
        x = X[0]
        if perturb is not None:
            x = x * (1.0 + 4.0 * EPS * perturb.uniform(-1.0, 1.0, x.size))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            f, g = objective(x)
        trials.append((X[0].copy(), -float(f), -np.asarray(g, dtype=np.float64)))
        return np.array([-f]), -np.asarray(g, dtype=np.float64)[None]

    P = len(theta0)
    x0 = logexp_finv(np.asarray(theta0, dtype=np.float64))
    X, F = lockstep_lbfgs(fun, x0[None], np.full(P, -np.inf), np.full(P, np.inf), max_rounds=max_rounds)
    rounds = len(trials) - 1
    decisions, small = [], False
    bx, bf, bg = trials[0][0], -trials[0][1], -trials[0][2]
    for x, v, g in trials[1:]:
        ft = -v
        ok = bool(np.isfinite(ft)) and not ft > bf + 1e-4 * bg.dot(x - bx)
        decisions.append(ok)
        if ok:
            small = bf - ft <= 2.2e-9 * max(abs(bf), abs(ft), 1.0)
            bx, bf, bg = x, ft, -g
    assert np.array_equal(X[0], bx)
    if np.max(np.abs(bg)) <= 1e-5 and (not decisions or decisions[-1]):
        status = _lib.REFINE_PGTOL
    elif decisions and decisions[-1] and small:
        status = _lib.REFINE_FTOL
    elif rounds >= max_rounds:
        status = _lib.REFINE_MAX_ROUNDS
    else:
        status = _lib.REFINE_STEP
    return dict(theta=logexp_f(X[0]), lml=float(F[0]), rounds=rounds, status=status, decisions=decisions, trials=trials)


_REFERENCE = {}


def reference(case):
    """The reference search of a case and the measured deviation of its perturbed repeats, computed once."""
    if case not in _REFERENCE:
        model = make_model(case)
        theta0 = start_of(case)
        ref = host_search(model, theta0)
        worst, stable = 0.0, True
        for seed in (1, 2, 3):
            moved = host_search(model, theta0, perturb=np.random.RandomState(seed))
            stable = stable and moved["decisions"] == ref["decisions"] and moved["status"] == ref["status"]
            worst = max(worst, float(np.max(np.abs(moved["theta"] - ref["theta"]) / np.abs(ref["theta"]))),
                        abs(moved["lml"] - ref["lml"]) / max(1.0, abs(ref["lml"])))
        model.close()
        _REFERENCE[case] = (ref, worst, stable)
    return _REFERENCE[case]


# ---- 1. the likelihood at the end point -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_final_likelihood_is_what_the_likelihood_call_answers_at_the_final_theta(hip, case):
    from cbo_with_oop_amd import _lib
    model = make_model(case)
    out = device_runs([model], [start_of(case)])[0]
    assert not out["declined"] and out["status"][0] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP,
                                                        _lib.REFINE_MAX_ROUNDS)
    lml, grad = likelihood_at(model, case, out["theta"][0])
    assert np.array_equal(bits(out["grad"][0]), bits(grad)), (out["grad"][0], grad)
    assert bits(out["lml"][0]) == bits(lml)
    model.close()


# ---- 2. the trajectory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_device_search_decides_as_the_reference_and_ends_within_the_measured_bar(hip, case):
    """The bar: 64 times the largest relative deviation of the reference's end point (theta and lml) when every evaluation
    is taken at x (1 + 4 eps r) (three seeds), not below 1e-12 -- the device differs from the host by a few ulp in theta at
    every trial point (another log1p / exp) and in the order of the dot products' sums; 4 ulp in x model that, 64 is the
    margin.  A perturbed reference that changes a decision would make the case a bad one (another start, not a wider bar)."""
    ref, measured, stable = reference(case)
    assert stable, "a perturbed reference run changed a decision: choose another start for this case"
    model = make_model(case)
    out = device_runs([model], [start_of(case)])[0]
    model.close()
    bar = max(64.0 * measured, 1e-12)
    dev_theta = float(np.max(np.abs(out["theta"][0] - ref["theta"]) / np.abs(ref["theta"])))
    dev_lml = abs(out["lml"][0] - ref["lml"]) / max(1.0, abs(ref["lml"]))
    print(f"{case_id(case)}: reference rounds {ref['rounds']} status {ref['status']} accepted {sum(ref['decisions'])}, "
          f"device rounds {out['rounds'][0]} status {out['status'][0]}, perturbed reference {measured:.3e}, bar {bar:.3e}, "
          f"device theta {dev_theta:.3e} lml {dev_lml:.3e}, lml {ref['lml']:.6f}")
    assert (int(out["rounds"][0]), int(out["status"][0])) == (ref["rounds"], ref["status"])
    assert dev_theta <= bar and dev_lml <= bar, (dev_theta, dev_lml, bar)


# ---- 3. what holds whatever the trajectory --------------------------------------------------------------------------------
def test_the_search_never_ends_below_its_start_and_a_pgtol_end_has_a_small_gradient(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_gradfactor
    seen = set()
    for case in CASES:
        model = make_model(case)
        theta0 = start_of(case)
        start = device_runs([model], [theta0], max_rounds=0)[0]
        assert (int(start["status"][0]), int(start["rounds"][0])) == (_lib.REFINE_MAX_ROUNDS, 0)
        lml0, grad0 = likelihood_at(model, case, theta0)
        # (theta0 goes through Logexp.finv and back: the start's theta may differ from theta0 in the last place)
        assert np.allclose(start["theta"][0], theta0, rtol=4 * EPS, atol=0.0) and np.isclose(start["lml"][0], lml0, rtol=1e-9)
        out = device_runs([model], [theta0], max_rounds=60)[0]
        assert out["lml"][0] >= start["lml"][0] and 0 <= out["rounds"][0] <= 60
        seen.add(int(out["status"][0]))
        if out["status"][0] == _lib.REFINE_PGTOL:
            _, grad = likelihood_at(model, case, out["theta"][0])
            assert np.max(np.abs(grad * logexp_gradfactor(out["theta"][0]))) <= 1e-5
        again = device_runs([model], [theta0], max_rounds=60)[0]
        assert same_bits(out, again)                                         # a second call: the same bits
        model.close()
    assert seen & {_lib.REFINE_PGTOL, _lib.REFINE_FTOL}


def test_a_models_runs_do_not_depend_on_the_other_models_of_the_call(hip):
    """Alone, among all eight (descriptors by value) and among nine (beyond kSmallByValue = 8: from the pinned array)."""
    cases = CASES + [CASES[1]]
    models = [make_model(c) for c in cases]
    theta0s = [start_of(c) for c in cases]
    alone = [device_runs([m], [t])[0] for m, t in zip(models, theta0s)]
    eight = device_runs(models[:8], theta0s[:8])
    nine = device_runs(models, theta0s)
    three = device_runs(models[2:5], theta0s[2:5])
    for got, want in list(zip(eight, alone)) + list(zip(nine, alone)) + list(zip(three, alone[2:5])):
        assert not got["declined"] and same_bits(got, want)
    assert same_bits(nine[8], nine[1])                                       # the same model twice in one call
    for m in models:
        m.close()


# ---- 4. restarts ----------------------------------------------------------------------------------------------------------
def test_every_run_of_a_restarted_model_is_the_one_start_call_from_its_row(hip):
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, mle_best_run
    cases = [CASES[3], CASES[5], CASES[1]]
    models = [make_model(c) for c in cases]
    rng = np.random.default_rng(5)
    theta0s = [np.vstack([start_of(c)[None], logexp_f(rng.standard_normal((3, start_of(c).size)))]) for c in cases]
    outs = device_runs(models, theta0s)
    for m, c, rows, out in zip(models, cases, theta0s, outs):
        assert out["theta"].shape == rows.shape and out["lml"].shape == (4,)
        for s in range(4):
            solo = device_runs([m], [rows[s]])[0]
            assert solo["status"][0] == out["status"][s] and solo["rounds"][0] == out["rounds"][s]
            for k in ("theta", "lml", "grad"):
                assert np.array_equal(bits(solo[k][0]), bits(out[k][s])), (case_id(c), s, k)
        best = mle_best_run(out["lml"], [int(v) for v in out["status"]])
        assert best == int(np.nanargmax(out["lml"]))
    # sixteen starts of nine models: 144 workgroups in one call
    big = device_runs(models * 3, [np.vstack([t] * 4) for t in theta0s * 3], max_rounds=6)
    for j, out in enumerate(big):
        assert out["theta"].shape[0] == 16
        for s in range(16):
            assert bits(out["lml"][s]) == bits(big[j % 3]["lml"][s % 4])
    for m in models:
        m.close()


def test_optimize_restarts_leaves_the_model_at_the_winner_and_draws_as_specified(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, optimize_together
    case = CASES[5]                                                          # (50, 2, ARD, fixed noise): P = 3
    model, twin = make_model(case), make_model(case)
    np.random.seed(17)
    res = model.optimize_restarts(num_restarts=4, max_iters=ROUNDS)
    state = np.random.get_state()
    np.random.seed(17)
    rows = np.vstack([start_of(case)[None], logexp_f(np.array([np.random.randn(3) for _ in range(3)]))])
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]     # three randn(P) calls, nothing else
    out = device_runs([twin], [rows])[0]
    best = int(np.nanargmax(out["lml"]))
    assert res.optimizer == "device" and res.transform == "logexp" and res.best_run == best and len(res.runs) == 4
    for s, run in enumerate(res.runs):
        assert bits(run["lml"]) == bits(out["lml"][s]) and np.array_equal(bits(run["theta"]), bits(out["theta"][s]))
        assert run["status"] == out["status"][s] and run["rounds"] == out["rounds"][s]
    theta = out["theta"][best]
    assert model.stale and model.variance == theta[0] and np.array_equal(model.lengthscale, theta[1:3])
    assert model.noise_var == 0.04 and model.optimization_result is res
    assert res.fun == -out["lml"][best] and res.nit == out["rounds"][best] and res.status == out["status"][best]
    assert res.message == _lib.MLE_STATUS_NAME[res.status] and res.x.shape == res.jac.shape == (3,)
    # one start draws nothing and is the plain device optimize
    np.random.seed(17)
    before = np.random.get_state()
    one = optimize_together([twin], max_iters=ROUNDS, optimizer="device")[0]
    now = np.random.get_state()
    assert np.array_equal(before[1], now[1]) and before[2:] == now[2:]
    assert bits(one.runs[0]["lml"]) == bits(out["lml"][0]) and one.best_run == 0
    solo = make_model(case)
    got = solo.optimize(max_iters=ROUNDS, optimizer="device")
    assert got.fun == one.fun and np.array_equal(solo.lengthscale, twin.lengthscale)
    with pytest.raises(ValueError, match="num_restarts"):
        solo.optimize_restarts(num_restarts=3, optimizer="host")
    with pytest.raises(ValueError, match="transform"):
        solo.optimize(transform="log", optimizer="device")
    for m in (model, twin, solo):
        m.close()


# ---- 5. not positive definite as assembled --------------------------------------------------------------------------------
def duplicate_model(variance, noise_var, fix_noise):
    """The jitter fixture's duplicated inputs: at a large variance the factorisation's rounding is above the 1e-8 on the
    diagonal and Ky is not positive definite as assembled."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture("jitter_ladder")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(f["X"], f["y"], variance=variance, lengthscale=1.0, noise_var=noise_var, fix_noise=fix_noise,
                                  fit=False)


def pd_as_assembled(model, theta):
    """Whether cbo_gp_lml_gradients answers the model at theta from its one-launch form (the factor the search's kernel
    builds), not from the general path behind jitchol's ladder: afterwards the model is still unfitted."""
    from cbo_with_oop_amd import _lib
    nl = model.lengthscale.size
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model.set_hyperparameters(theta[0], theta[1:1 + nl], model.noise_var if model.fix_noise else theta[1 + nl], fit=False)
        try:
            model.log_likelihood_gradients()
        except np.linalg.LinAlgError:
            return False
    rc = _lib.load().cbo_gp_jitter(model._handle, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_double()))
    return rc == _lib.CBO_ERR_NOT_FITTED


TRIAL_START = np.array([100.0, 1.0, 1e-300])


def test_a_trial_point_that_is_not_positive_definite_halves_the_step(hip):
    """Duplicated rows, the noise started at 1e-300 (only the 1e-8 on the diagonal keeps Ky positive definite): the reference
    is lockstep_lbfgs on an objective that answers NaN where the likelihood call needs jitchol's ladder.  From this start
    the second and later trials shrink the lengthscale to a denormal, where Ky as assembled is not a number, let alone
    positive definite -- far from the boundary, so the host's and the device's theta, a few ulp apart, fall on the same
    side of it -- and the step is halved until the trial is answered again (9 such trials of 40 when this was written)."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f
    model = duplicate_model(TRIAL_START[0], TRIAL_START[2], False)
    assert pd_as_assembled(model, TRIAL_START)                               # the start is answered by the one-launch form

    def objective(x):
        theta = logexp_f(x)
        if not pd_as_assembled(model, theta):
            return np.nan, np.zeros_like(x)
        return model._objective(x, "logexp")
    ref = host_search(model, TRIAL_START, objective=objective)
    failed = [np.isnan(v) for _, v, _ in ref["trials"]]
    assert any(failed), "no trial point of the reference is not positive definite: choose another start"
    out = device_runs([model], [TRIAL_START])[0]
    start = device_runs([model], [TRIAL_START], max_rounds=0)[0]
    print(f"not-PD trial: reference rounds {ref['rounds']} status {ref['status']} NaN trials {sum(failed)}, device rounds "
          f"{out['rounds'][0]} status {out['status'][0]} lml {out['lml'][0]:.6f} (start {start['lml'][0]:.6f})")
    assert out["status"][0] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP, _lib.REFINE_MAX_ROUNDS)
    assert np.isfinite(out["lml"][0]) and out["lml"][0] >= start["lml"][0] and np.all(np.isfinite(out["theta"][0]))
    assert (int(out["rounds"][0]), int(out["status"][0])) == (ref["rounds"], ref["status"])
    model.close()


def test_a_start_that_is_not_positive_definite_ends_the_run_and_the_wrapper_repeats_the_model_on_the_host(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import optimize_together
    theta0 = np.array([1e12, 1.0])
    model, good = duplicate_model(1e12, 1e-12, True), make_model(CASES[1])
    assert not pd_as_assembled(model, theta0)                                # a status word from the likelihood call, no more
    outs = device_runs([model, good], [np.vstack([theta0, [1.0, 1.0]]), start_of(CASES[1])])
    assert outs[0]["status"][0] == _lib.MLE_NOT_PD and outs[0]["rounds"][0] == 0 and not outs[0]["declined"]
    assert outs[0]["status"][1] != _lib.MLE_NOT_PD and np.isfinite(outs[0]["lml"][1])     # its other start runs as ever
    assert same_bits(outs[1], device_runs([good], [start_of(CASES[1])])[0])               # ... and so does the neighbour
    # the wrapper: the host route's answer for that model, the device's for the other
    twin = duplicate_model(1e12, 1e-12, True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = optimize_together([model, good], max_iters=ROUNDS, optimizer="device")
        want = optimize_together([twin], max_iters=ROUNDS)[0]
        assert not hasattr(got[0], "optimizer") and got[1].optimizer == "device"
        assert got[0].fun == want.fun and np.array_equal(got[0].x, want.x) and model.variance == twin.variance
        with pytest.raises(RuntimeError, match="positive definite"):
            optimize_together([duplicate_model(1e12, 1e-12, True)], optimizer="device", host_fallback=False)
    for m in (model, good, twin):
        m.close()


# ---- 6. declined models ---------------------------------------------------------------------------------------------------
def test_larger_fp32_and_switched_off_models_are_declined_and_the_wrapper_takes_the_host_route(hip, monkeypatch):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import optimize_together
    case = CASES[1]
    build = lambda: [make_model(case), make_model(case, n=129), make_model(case, dtype="f32"), make_model(CASES[2])]   # noqa: E731
    models, twins = build(), build()
    cases = [case, case, case, CASES[2]]
    outs = device_runs(models, [start_of(c) for c in cases])
    assert [o["declined"] for o in outs] == [False, True, True, False]
    for o in outs[1:3]:                                                       # nothing else written
        assert np.all(o["status"] == -1) and np.all(np.isnan(o["theta"])) and np.all(np.isnan(o["lml"]))
    assert same_bits(outs[3], device_runs(models[3:], [start_of(CASES[2])])[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = optimize_together(models, max_iters=ROUNDS, optimizer="device")
        want = optimize_together(twins[1:3], max_iters=ROUNDS)
        for j in (1, 2):
            assert not hasattr(got[j], "optimizer") and got[j].fun == want[j - 1].fun and np.array_equal(got[j].x, want[j - 1].x)
        assert got[0].optimizer == got[3].optimizer == "device"
        with pytest.raises(RuntimeError, match="declined"):
            optimize_together(models, optimizer="device", host_fallback=False)
    for m in models + twins:
        m.close()
    monkeypatch.setenv("CBO_HIP_SMALL_SETS", "0")
    ctx = _lib.Context(0)
    try:
        off = make_model(case, context=ctx)
        assert device_runs([off], [start_of(case)])[0]["declined"]
        off.close()
    finally:
        ctx.close()


# ---- 7. invalid arguments -------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_before_any_device_work(hip):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    case = CASES[3]
    model, other = make_model(case, fit=True), make_model(CASES[1])
    P = start_of(case).size
    state = [np.array(v) for v in model.posterior_state()]

    def call(n_models=None, gps=True, runs=True, status=True, models=(model,), null=None, **over):
        k = len(models)
        handles = (ctypes.c_void_p * k)(*[m._handle if m is not None else None for m in models])
        arr = (_lib.CboMleRun * k)()
        keep = []
        for j, m in enumerate(models):
            size = over.get("n_params", P if m is not other else 3)
            starts = over.get("n_starts", 2)
            rows = max(starts, 1)
            buf = dict(theta0=np.array(over.get("theta0", np.full(rows * size, 0.8))), theta_out=np.full(rows * size, -7.0),
                       lml_out=np.full(rows, -7.0), grad_out=np.full(rows * size, -7.0))
            ints = dict(status_out=np.full(rows, -7, dtype=np.int32), rounds_out=np.full(rows, -7, dtype=np.int32))
            r = arr[j]
            r.n_params, r.fit_noise, r.n_starts, r.max_rounds = size, over.get("fit_noise", 1), starts, over.get("max_rounds", 3)
            for name, a in buf.items():
                setattr(r, name, None if name == null else _lib.dptr(a))
            for name, a in ints.items():
                setattr(r, name, None if name == null else a.ctypes.data_as(_lib.c_int_p))
            keep.append((buf, ints))
        st = np.full(k, -7, dtype=np.int32)
        rc = lib.cbo_gp_mle_sets(k if n_models is None else n_models, handles if gps else None, arr if runs else None,
                                 st.ctypes.data_as(_lib.c_int_p) if status else None)
        if rc == _lib.CBO_ERR_INVALID:                                       # the outputs are untouched
            assert np.all(st == -7)
            for buf, ints in keep:
                assert all(np.all(buf[name] == -7.0) for name in ("theta_out", "lml_out", "grad_out"))
                assert all(np.all(a == -7) for a in ints.values())
        return rc

    invalid = _lib.CBO_ERR_INVALID
    assert call() == _lib.CBO_OK
    assert call(gps=False) == invalid and call(runs=False) == invalid and call(status=False) == invalid
    assert call(models=(None,)) == invalid
    for name in ("theta0", "theta_out", "lml_out", "grad_out", "status_out", "rounds_out"):
        assert call(null=name) == invalid, name
    assert call(n_models=0) == invalid and call(n_models=-2) == invalid
    assert call(n_starts=0) == invalid and call(n_starts=_lib.MLE_MAX_STARTS + 1) == invalid
    assert call(n_starts=_lib.MLE_MAX_STARTS, max_rounds=0) == _lib.CBO_OK
    assert call(max_rounds=-1) == invalid and call(max_rounds=_lib.MLE_MAX_ROUNDS + 1) == invalid
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        theta0 = np.full(2 * P, 0.8)
        theta0[P + 2] = bad                                                  # (in the second start's row)
        assert call(theta0=theta0) == invalid, bad
    assert call(n_params=P - 1) == invalid and call(n_params=P + 1) == invalid      # a P that does not match the model
    assert call(fit_noise=0) == invalid and call(fit_noise=2) == invalid
    ctx = _lib.Context(model._ctx.device_id)
    try:
        stranger = make_model(CASES[1], context=ctx)
        assert call(models=(other, stranger)) == invalid and b"context" in lib.cbo_last_error()
        stranger.close()
    finally:
        ctx.close()
    # the models are what they were
    assert not model.stale and other.stale
    for a, b in zip(model.posterior_state(), state):
        assert np.array_equal(np.array(a), b)
    model.close(); other.close()


# ---- 8. reading only ------------------------------------------------------------------------------------------------------
def test_the_models_are_only_read(hip):
    case = CASES[3]                                                          # (17, 4, ARD, causal)
    Xs = np.random.default_rng(3).uniform(-2, 2, (70, case[1]))
    model = make_model(case, fit=True)
    before = model.predict(Xs)
    state = [np.array(v) for v in model.posterior_state()]
    hyper = (model.variance, model.lengthscale.copy(), model.noise_var)
    out = device_runs([model], [np.vstack([start_of(case), 0.5 * start_of(case)])])[0]
    assert not out["declined"] and np.all(np.isfinite(out["lml"]))
    assert not model.stale
    assert (model.variance, model.noise_var) == (hyper[0], hyper[2]) and np.array_equal(model.lengthscale, hyper[1])
    after = model.predict(Xs)
    for a, b in zip(after, before):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(model.posterior_state(), state):
        assert np.array_equal(np.array(a), b)
    # an unfitted model is answered and stays unfitted
    cold = make_model(case)
    assert np.isfinite(device_runs([cold], [start_of(case)])[0]["lml"][0]) and cold.stale
    model.close(); cold.close()


# ---- 9. the agent ---------------------------------------------------------------------------------------------------------
def toy_agent(**kw):
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
    rng = np.random.default_rng(4)
    xs = [rng.uniform(-5, 5, (6, 1)), rng.uniform(-5, 20, (6, 1))]
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=4, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, **kw)
        return agent, agent.run()


def test_the_agent_runs_with_the_device_optimiser_and_the_host_switch_changes_nothing(hip, monkeypatch):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    calls = []
    bound = lib.cbo_gp_mle_sets
    monkeypatch.setattr(lib, "cbo_gp_mle_sets", lambda n, *a: (calls.append(int(n)), bound(n, *a))[1])
    agent, mon = toy_agent(mle_optimizer="device", mle_restarts=2)
    assert len(mon.type_trial) == 4 and agent.mle_optimizer == "device"
    assert calls and calls[0] == 2 and 1 in calls                            # both graph GPs in one call; a closing optimize
    assert all(np.all(np.isfinite(np.asarray(y, dtype=np.float64))) for y in agent.data_y)
    for gp in agent.graph_gps.values():
        assert gp.optimization_result.optimizer == "device" and len(gp.optimization_result.runs) == 2
    calls.clear()
    plain, mon_plain = toy_agent()
    host, mon_host = toy_agent(mle_optimizer="host")
    assert not calls
    for a, b in zip(plain.data_x + plain.data_y, host.data_x + host.data_y):
        assert np.array_equal(bits(a), bits(b))
    assert mon_plain.type_trial == mon_host.type_trial
