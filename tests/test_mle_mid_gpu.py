"""GPU tests of the one-launch hyper-parameter MLE for models of 129..256 observations (cbo_gp_mle_sets_rows with
max_rows = 256, mle_mid_kernel).  The reference is never the kernel under test: it is ``lockstep_lbfgs`` with
an infinite box on the lockstep route's own evaluation -- ``_objective_set(fit=False)``, ``lml_gradients_batch([model])``
(the two-block form on the model's resident points), ``_objective_value`` -- one likelihood launch per evaluation.  Every
search takes at most 40 rounds."""
import ctypes
import warnings

import numpy as np
import pytest

from test_mle_sets_gpu import bits, host_search, same_bits

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


# (n, d, ard, causal, fixed noise): the smallest shapes at which the two-block form can go wrong -- one live row in block 2,
# a ragged second tile of block 2, P = 6, the graph GPs' shape, both blocks full at D = 8
CASES = [(129, 1, False, False, False), (145, 2, True, False, True), (160, 3, False, True, False),
         (192, 4, True, True, False), (200, 3, True, False, True), (256, 8, False, False, False)]
SMALL = [(10, 1, False, False, False), (50, 2, True, False, True), (128, 3, False, True, False)]
case_id = lambda c: "n{}-d{}-{}-{}-{}".format(c[0], c[1], "ard" if c[2] else "iso", "causal" if c[3] else "plain",   # noqa: E731
                                              "fixed" if c[4] else "noise")


def make_model(case, n=None, dtype=None, context=None):
    """tests/test_mle_sets_gpu.py's generator at these sizes; never fitted."""
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
                                  noise_var=0.04, fix_noise=fixed, fit=False, **kw)


# The searches' starts: the model's own parameters times START_SCALE[case] (1 unless noted).  A case whose reference changes a
# decision under the bar's perturbation from the model's own start gets another start here, never a wider bar.
START_SCALE = {}


def start_of(case):
    n, d, ard, causal, fixed = case
    ls = np.linspace(0.7, 1.6, d) if ard else np.array([0.9])
    return np.concatenate([[1.2], ls, [] if fixed else [0.04]]) * START_SCALE.get(case, 1.0)


def device_runs(models, theta0s, max_rounds=ROUNDS, device_rows=256):
    from cbo_with_oop_amd.GaussianProcessFactory import mle_runs_device
    return mle_runs_device(models, theta0s, max_rounds, device_rows=device_rows)


def batch_likelihood_at(model, theta):
    """(lml, dlml / dtheta) by cbo_gp_lml_gradients_batch for the model set to theta, unfitted; None where the launch's
    two-block form did not answer (Ky not positive definite as assembled: the call then walked jitchol's ladder and left
    the model fitted)."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import _objective_set, lml_gradients_batch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _objective_set(model, np.asarray(theta, dtype=np.float64), fit=False)
        a = lml_gradients_batch([model])[0]
    rc = _lib.load().cbo_gp_jitter(model._handle, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_double()))
    if a is None or rc != _lib.CBO_ERR_NOT_FITTED:
        return None
    lml, dv, dls, dn = a
    return lml, np.concatenate([[dv], dls, [] if model.fix_noise else [dn]])


def batch_objective(model, nan_when_not_pd=False):
    """The lockstep route's evaluation of one model: (-lml, -d lml / dx) at x, priors included."""
    from cbo_with_oop_amd.GaussianProcessFactory import (_has_priors, _objective_set, _objective_value, lml_gradients_batch,
                                                         log_prior_batch, logexp_f)

    def objective(x):
        theta = logexp_f(np.asarray(x, dtype=np.float64))
        if nan_when_not_pd and batch_likelihood_at(model, theta) is None:
            return np.nan, np.zeros_like(x)
        _objective_set(model, theta, fit=False)
        a = lml_gradients_batch([model])[0]
        prior = log_prior_batch([model])[0] if _has_priors(model) else None
        return _objective_value(model, theta, *a, "logexp", prior)
    return objective


_REFERENCE = {}


def reference(case):
    """The reference search of a case and the measured deviation of its perturbed repeats, computed once."""
    if case not in _REFERENCE:
        model = make_model(case)
        theta0, objective = start_of(case), batch_objective(model)
        ref = host_search(model, theta0, ROUNDS, objective=objective)
        worst, stable = 0.0, True
        for seed in (1, 2, 3):
            moved = host_search(model, theta0, ROUNDS, perturb=np.random.RandomState(seed), objective=objective)
            stable = stable and moved["decisions"] == ref["decisions"] and moved["status"] == ref["status"]
            worst = max(worst, float(np.max(np.abs(moved["theta"] - ref["theta"]) / np.abs(ref["theta"]))),
                        abs(moved["lml"] - ref["lml"]) / max(1.0, abs(ref["lml"])))
        model.close()
        _REFERENCE[case] = (ref, worst, stable)
    return _REFERENCE[case]


_ALONE = {}


def alone(case):
    """The case's model searched alone from its start, computed once and shared (never modified)."""
    if case not in _ALONE:
        model = make_model(case)
        _ALONE[case] = device_runs([model], [start_of(case)])[0]
        model.close()
    return _ALONE[case]


# ---- 1. the likelihood at the end point -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_final_likelihood_is_the_batch_likelihood_of_a_twin_at_the_final_theta(hip, case):
    from cbo_with_oop_amd import _lib
    out = alone(case)
    assert not out["declined"] and out["status"][0] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP,
                                                        _lib.REFINE_MAX_ROUNDS)
    model, twin = make_model(case), make_model(case)
    lml, grad = batch_likelihood_at(twin, out["theta"][0])
    assert np.array_equal(bits(out["grad"][0]), bits(grad)), (out["grad"][0], grad)
    assert bits(out["lml"][0]) == bits(lml)
    # no rounds: the start's likelihood, MAX_ROUNDS, 0 rounds
    theta0 = start_of(case)
    start = device_runs([model], [theta0], max_rounds=0)[0]
    assert (int(start["status"][0]), int(start["rounds"][0])) == (_lib.REFINE_MAX_ROUNDS, 0)
    # (theta0 goes through Logexp.finv and back: the start's theta may differ from theta0 in the last place)
    assert np.allclose(start["theta"][0], theta0, rtol=4 * EPS, atol=0.0)
    lml0, grad0 = batch_likelihood_at(twin, start["theta"][0])
    assert bits(start["lml"][0]) == bits(lml0) and np.array_equal(bits(start["grad"][0]), bits(grad0))
    assert model.stale                                                       # the models are only read
    model.close(); twin.close()


# ---- 2. the trajectory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_device_search_decides_as_the_reference_and_ends_within_the_measured_bar(hip, case):
    """DESIGN.md §4v's bar: 64 times the largest relative deviation of the reference's end point (theta and lml) when every
    evaluation is taken at x (1 + 4 eps r) (three seeds), not below 1e-12.  A perturbed reference that changes a decision
    makes the start a bad one (another start in START_SCALE, not a wider bar).  Measured values: DESIGN.md §4z."""
    ref, measured, stable = reference(case)
    out = alone(case)
    bar = max(64.0 * measured, 1e-12)
    dev_theta = float(np.max(np.abs(out["theta"][0] - ref["theta"]) / np.abs(ref["theta"])))
    dev_lml = abs(out["lml"][0] - ref["lml"]) / max(1.0, abs(ref["lml"]))
    print(f"{case_id(case)}: reference rounds {ref['rounds']} status {ref['status']} accepted {sum(ref['decisions'])} "
          f"stable {stable}, device rounds {out['rounds'][0]} status {out['status'][0]}, perturbed reference {measured:.3e}, "
          f"bar {bar:.3e}, device theta {dev_theta:.3e} lml {dev_lml:.3e}, lml {ref['lml']:.6f}")
    assert stable, "a perturbed reference run changed a decision: choose another start for this case"
    assert (int(out["rounds"][0]), int(out["status"][0])) == (ref["rounds"], ref["status"])
    assert dev_theta <= bar and dev_lml <= bar, (dev_theta, dev_lml, bar)


# ---- 3. independence ------------------------------------------------------------------------------------------------------
def test_a_models_runs_do_not_depend_on_the_other_models_of_the_call(hip):
    """Alone, among the six, in a mixed call of nine (six mid, three small) and in one of twelve whose nine mid models are
    beyond kSmallByValue = 8 (descriptors from the pinned array).  The small models of such a call give cbo_gp_mle_sets'
    bits; a second call gives the same bits."""
    mids, smalls = [make_model(c) for c in CASES], [make_model(c) for c in SMALL]
    t_mid, t_small = [start_of(c) for c in CASES], [start_of(c) for c in SMALL]
    want = [alone(c) for c in CASES]
    six = device_runs(mids, t_mid)
    # interleaved: the call sorts its models into the two launches itself
    order = [("m", 0), ("s", 0), ("m", 1), ("m", 2), ("s", 1), ("m", 3), ("m", 4), ("s", 2), ("m", 5)]
    pick = lambda kind, j: ((mids, t_mid) if kind == "m" else (smalls, t_small))                       # noqa: E731
    nine = device_runs([pick(k, j)[0][j] for k, j in order], [pick(k, j)[1][j] for k, j in order])
    again = device_runs([pick(k, j)[0][j] for k, j in order], [pick(k, j)[1][j] for k, j in order])
    twelve = device_runs(mids + smalls + mids[:3], t_mid + t_small + t_mid[:3])
    plain = device_runs(smalls, t_small, device_rows=128)                      # cbo_gp_mle_sets itself
    for got, ref in zip(six, want):
        assert not got["declined"] and same_bits(got, ref)
    for (kind, j), got, rep in zip(order, nine, again):
        assert not got["declined"] and same_bits(got, want[j] if kind == "m" else plain[j]) and same_bits(got, rep)
    for got, ref in zip(twelve, want + plain + want[:3]):
        assert not got["declined"] and same_bits(got, ref)
    assert not same_bits(want[0], want[1])
    for m in mids + smalls:
        m.close()


# ---- 4. restarts ----------------------------------------------------------------------------------------------------------
def test_every_run_of_a_restarted_model_is_the_one_start_call_from_its_row(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, mle_best_run
    cases = [CASES[1], CASES[3]]
    models = [make_model(c) for c in cases]
    rng = np.random.default_rng(5)
    theta0s = [np.vstack([start_of(c)[None], logexp_f(rng.standard_normal((3, start_of(c).size)))]) for c in cases]
    outs = device_runs(models, theta0s)
    for m, c, rows, out in zip(models, cases, theta0s, outs):
        assert out["theta"].shape == rows.shape and out["lml"].shape == (4,)
        assert same_bits({k: v[:1] for k, v in out.items() if k != "declined"}, alone(c))
        for s in range(1, 4):
            solo = device_runs([m], [rows[s]])[0]
            assert solo["status"][0] == out["status"][s] and solo["rounds"][0] == out["rounds"][s]
            for k in ("theta", "lml", "grad"):
                assert np.array_equal(bits(solo[k][0]), bits(out[k][s])), (case_id(c), s, k)
    for m in models:
        m.close()
    # optimize_restarts on a 200-row model: the model is left at the best run
    case = CASES[4]
    model, twin = make_model(case), make_model(case)
    np.random.seed(17)
    res = model.optimize_restarts(num_restarts=4, max_iters=ROUNDS, device_rows=256)
    np.random.seed(17)
    rows = np.vstack([start_of(case)[None], logexp_f(np.array([np.random.randn(4) for _ in range(3)]))])
    out = device_runs([twin], [rows])[0]
    best = mle_best_run(out["lml"], [int(v) for v in out["status"]])
    assert best == int(np.nanargmax(out["lml"]))
    assert res.optimizer == "device" and res.best_run == best and len(res.runs) == 4
    for s, run in enumerate(res.runs):
        assert bits(run["lml"]) == bits(out["lml"][s]) and np.array_equal(bits(run["theta"]), bits(out["theta"][s]))
        assert run["status"] == out["status"][s] and run["rounds"] == out["rounds"][s]
    theta = out["theta"][best]
    assert model.stale and model.variance == theta[0] and np.array_equal(model.lengthscale, theta[1:4])
    assert model.noise_var == 0.04 and model.optimization_result is res and res.fun == -out["lml"][best]
    assert res.message == _lib.MLE_STATUS_NAME[res.status]
    # ... and without the keyword the same model is declined and takes the lockstep route: no restarts there
    solo = make_model(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert not hasattr(solo.optimize(max_iters=ROUNDS, optimizer="device"), "optimizer")
    for m in (model, twin, solo):
        m.close()


# ---- 5. priors ------------------------------------------------------------------------------------------------------------
def test_with_priors_the_final_value_is_the_batch_likelihood_plus_the_log_prior_bit_for_bit(hip):
    from cbo_with_oop_amd.GaussianProcessFactory import log_prior_batch
    from cbo_with_oop_amd.utils_functions import priors as pr
    for case in (CASES[0], CASES[4]):
        model, twin, never = make_model(case), make_model(case), make_model(case)
        for m in (model, twin):
            m.set_prior("variance", pr.Gamma(2.0, 1.5))
            m.set_prior("lengthscale", pr.LogGaussian(0.2, 0.8))
        out = device_runs([model], [start_of(case)])[0]
        assert not out["declined"] and not same_bits(out, alone(case))
        theta = out["theta"][0]
        lml, grad = batch_likelihood_at(twin, theta)
        lp, dlp = log_prior_batch([twin], [theta])[0]
        assert lp != 0.0 and np.any(dlp != 0.0)
        assert bits(out["lml"][0]) == bits(lml + lp), (out["lml"][0], lml, lp)
        assert np.array_equal(bits(out["grad"][0]), bits(grad + dlp)), (out["grad"][0], grad, dlp)
        # priors unset: the launch without priors, the bits of a model that never had any
        model.unset_priors()
        assert same_bits(device_runs([model], [start_of(case)])[0], device_runs([never], [start_of(case)])[0])
        assert same_bits(device_runs([never], [start_of(case)])[0], alone(case))
        for m in (model, twin, never):
            m.close()


# ---- 6. not positive definite as assembled --------------------------------------------------------------------------------
NOT_PD_START = np.array([100.0, 1.0, 1e-300])


def duplicate_model(offset, n=150, noise_var=1e-300, noise_y=0.05):
    """One dimension, every row of the first half twice.  ``offset`` moves the inputs away from the origin: the squared
    distances come from |x|^2 + |x'|^2 - 2 x x', so at an offset of 1e4 they carry an absolute error near 1e-8 and Ky
    = K + 1e-8 I at variance 100 is not positive definite as assembled (at offset 0 the 1e-8 on the diagonal keeps it so)."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(3)
    half = rng.uniform(-2, 2, (n // 2, 1))
    X = np.vstack([half, half]) + offset
    y = np.sin(X - offset) + noise_y * rng.standard_normal((n, 1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, variance=NOT_PD_START[0], lengthscale=NOT_PD_START[1], noise_var=noise_var,
                                  fix_noise=False, fit=False)


def test_a_start_that_is_not_positive_definite_ends_the_run_and_the_wrapper_takes_the_host_route(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import optimize_together
    model, good = duplicate_model(1e4), make_model(CASES[0])
    probe = duplicate_model(1e4)
    assert batch_likelihood_at(probe, NOT_PD_START) is None                      # a status word from the likelihood launch
    probe.close()
    outs = device_runs([model, good], [np.vstack([NOT_PD_START, [1.0, 1.0, 0.5]]), start_of(CASES[0])])
    assert outs[0]["status"][0] == _lib.MLE_NOT_PD and outs[0]["rounds"][0] == 0 and not outs[0]["declined"]
    assert same_bits(outs[1], alone(CASES[0]))                                   # the neighbour runs as ever
    assert same_bits(device_runs([good], [start_of(CASES[0])])[0], alone(CASES[0]))     # ... and the info word was cleared
    twin = duplicate_model(1e4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = optimize_together([model, good], max_iters=ROUNDS, optimizer="device", device_rows=256)
        want = optimize_together([twin], max_iters=ROUNDS)[0]
        assert not hasattr(got[0], "optimizer") and got[1].optimizer == "device"
        assert got[0].fun == want.fun and np.array_equal(got[0].x, want.x) and model.variance == twin.variance
        with pytest.raises(RuntimeError, match="positive definite"):
            optimize_together([duplicate_model(1e4)], optimizer="device", device_rows=256, host_fallback=False)
    for m in (model, good, twin):
        m.close()


TRIAL_START = np.array([1.0, 1.0, 0.5])


def test_a_trial_point_that_is_not_positive_definite_halves_the_step(hip):
    """The duplicated rows at the offset of 1e4, started at a noise of 0.5, far above the squared distances' error: the start
    is positive definite as assembled, but the search's first long steps take the noise below that error, where Ky is not
    (trials 2, 3 and 4 of the reference's 23 rounds when this was written; from the origin with the noise at 1e-300 no
    trial of 40 rounds fails: a start the test cannot use).  The reference is lockstep_lbfgs on an objective that answers
    NaN where the likelihood launch's two-block form does not answer."""
    from cbo_with_oop_amd import _lib
    model = duplicate_model(1e4, noise_var=TRIAL_START[2])
    assert batch_likelihood_at(model, TRIAL_START) is not None                   # the start is answered by the two-block form
    ref = host_search(model, TRIAL_START, ROUNDS, objective=batch_objective(model, nan_when_not_pd=True))
    failed = [np.isnan(v) for _, v, _ in ref["trials"]]
    out = device_runs([model], [TRIAL_START])[0]
    start = device_runs([model], [TRIAL_START], max_rounds=0)[0]
    print(f"not-PD trial: reference rounds {ref['rounds']} status {ref['status']} NaN trials {sum(failed)}, device rounds "
          f"{out['rounds'][0]} status {out['status'][0]} lml {out['lml'][0]:.6f} (start {start['lml'][0]:.6f})")
    assert any(failed), "no trial point of the reference is not positive definite: choose another start"
    assert out["status"][0] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP, _lib.REFINE_MAX_ROUNDS)
    assert np.isfinite(out["lml"][0]) and out["lml"][0] > start["lml"][0] and np.all(np.isfinite(out["theta"][0]))
    assert (int(out["rounds"][0]), int(out["status"][0])) == (ref["rounds"], ref["status"])
    assert same_bits(device_runs([model], [TRIAL_START])[0], out)                # the info word was cleared
    model.close()


# ---- 7. routing -----------------------------------------------------------------------------------------------------------
def test_larger_fp32_and_switched_off_models_are_declined_and_refusals_come_before_any_device_work(hip, monkeypatch):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import optimize_together
    lib = _lib.load()
    case = CASES[0]
    build = lambda: [make_model(case), make_model(case, n=257), make_model(case, dtype="f32")]          # noqa: E731
    models, twins = build(), build()
    outs = device_runs(models, [start_of(case)] * 3)
    assert [o["declined"] for o in outs] == [False, True, True]
    for o in outs[1:]:                                                        # nothing else written
        assert np.all(o["status"] == -1) and np.all(np.isnan(o["theta"])) and np.all(np.isnan(o["lml"]))
    assert device_runs(models[:1], [start_of(case)], device_rows=128)[0]["declined"]      # the default: 129 rows are declined
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = optimize_together(models, max_iters=ROUNDS, optimizer="device", device_rows=256)
        want = optimize_together(twins[1:], max_iters=ROUNDS)
        for j in (1, 2):
            assert not hasattr(got[j], "optimizer") and got[j].fun == want[j - 1].fun and np.array_equal(got[j].x, want[j - 1].x)
        assert got[0].optimizer == "device"
        with pytest.raises(RuntimeError, match="declined"):
            optimize_together(models, optimizer="device", device_rows=256, host_fallback=False)

    # 257 mid runs, and a max_rows that is neither 128 nor 256: CBO_ERR_INVALID, nothing written
    def call(ms, starts, max_rows):
        k = len(ms)
        handles = (ctypes.c_void_p * k)(*[m._handle for m in ms])
        arr = (_lib.CboMleRun * k)()
        keep = []
        for j in range(k):
            buf = dict(theta0=np.full(starts * 3, 0.8), theta_out=np.full(starts * 3, -7.0), lml_out=np.full(starts, -7.0),
                       grad_out=np.full(starts * 3, -7.0))
            ints = dict(status_out=np.full(starts, -7, dtype=np.int32), rounds_out=np.full(starts, -7, dtype=np.int32))
            r = arr[j]
            r.n_params, r.fit_noise, r.n_starts, r.max_rounds = 3, 1, starts, 2
            for name, a in buf.items():
                setattr(r, name, _lib.dptr(a))
            for name, a in ints.items():
                setattr(r, name, a.ctypes.data_as(_lib.c_int_p))
            keep.append((buf, ints))
        st = np.full(k, -7, dtype=np.int32)
        rc = lib.cbo_gp_mle_sets_rows(k, handles, arr, max_rows, st.ctypes.data_as(_lib.c_int_p))
        untouched = np.all(st == -7) and all(np.all(b[name] == -7.0) for b, _ in keep for name in ("theta_out", "lml_out", "grad_out")) \
            and all(np.all(a == -7) for _, i in keep for a in i.values())
        return rc, untouched
    mid = models[0]
    assert call([mid] * 17, 16, 256) == (_lib.CBO_ERR_INVALID, True) and b"256 runs" in lib.cbo_last_error()     # 272 runs
    assert call([mid] * 16 + [mid], 16, 128)[0] == _lib.CBO_OK                # (declined, all of them: no mid run at 128)
    for bad in (200, 0, 129, 512, -256):
        assert call([mid], 2, bad) == (_lib.CBO_ERR_INVALID, True) and b"max_rows" in lib.cbo_last_error()
    rc, untouched = call([mid] * 16, 16, 256)                                 # 256 runs: the most one call takes
    assert rc == _lib.CBO_OK and not untouched
    for m in models + twins:
        m.close()
    monkeypatch.setenv("CBO_HIP_SMALL_SETS", "0")
    ctx = _lib.Context(0)
    try:
        # switched off, both bands are declined; the host route's result is checked on the small model (on such a context the
        # lockstep route's likelihood batch does not answer an unfitted model of 129..256 rows, with or without this call)
        off, low, twin = make_model(case, context=ctx), make_model(SMALL[0], context=ctx), make_model(SMALL[0], context=ctx)
        assert [o["declined"] for o in device_runs([off, low], [start_of(case), start_of(SMALL[0])])] == [True, True]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = optimize_together([low], max_iters=ROUNDS, optimizer="device", device_rows=256)[0]
            want = optimize_together([twin], max_iters=ROUNDS)[0]
        assert not hasattr(got, "optimizer") and got.fun == want.fun and np.array_equal(got.x, want.x)
        off.close(); low.close(); twin.close()
    finally:
        ctx.close()


# ---- 8. the agent ---------------------------------------------------------------------------------------------------------
def toy_agent(**kw):
    """tests/test_mle_sets_gpu.py's toy agent with 140 observational rows at the start and 10 more per observe step."""
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model

    class Toy(ToyGraph):
        manipulative_variables = ("X", "Z")
        _fit_dependencies = (("X",), ("Z",))
        _fit_parameters = ([1.0, 1.0, 10.0, False], [1.0, 1.0, 10.0, False])

    sem = Toy.define_sem()
    rng = np.random.default_rng(11)
    draws = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(170)]
    obs = {v: np.array([r[v] for r in draws]) for v in draws[0] if not v.startswith("U")}
    init = {k: v[:140] for k, v in obs.items()}
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    rng = np.random.default_rng(4)
    xs = [rng.uniform(-5, 5, (6, 1)), rng.uniform(-5, 20, (6, 1))]
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return CBO(Toy, init, obs, data, exploration_set=es, num_trials=3, initial_num_obs_samples=140,
                   num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets, **kw)


def test_the_agents_observe_step_is_one_device_call_with_no_likelihood_batch_call(hip, monkeypatch):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    calls = {"rows": [], "sets": [], "batch": []}
    bound = {name: getattr(lib, name) for name in ("cbo_gp_mle_sets_rows", "cbo_gp_mle_sets", "cbo_gp_lml_gradients_batch")}
    monkeypatch.setattr(lib, "cbo_gp_mle_sets_rows",
                        lambda n, g, r, rows, st: (calls["rows"].append((int(n), int(rows))), bound["cbo_gp_mle_sets_rows"](n, g, r, rows, st))[1])
    monkeypatch.setattr(lib, "cbo_gp_mle_sets", lambda n, *a: (calls["sets"].append(int(n)), bound["cbo_gp_mle_sets"](n, *a))[1])
    monkeypatch.setattr(lib, "cbo_gp_lml_gradients_batch",
                        lambda n, *a: (calls["batch"].append(int(n)), bound["cbo_gp_lml_gradients_batch"](n, *a))[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = toy_agent(mle_optimizer="device", mle_device_rows=256, mle_restarts=2)
        agent.graph_gps = agent.graph.fit_all_gaussian_processes(agent.measurements, lockstep=agent.lockstep, **agent._mle_kwargs())
        assert calls == {"rows": [(2, 256)], "sets": [], "batch": []}        # the first fit: 140 rows, both graph GPs in one call
        for c in calls.values():
            c.clear()
        agent.observe()
        assert calls == {"rows": [(2, 256)], "sets": [], "batch": []}        # observe(): 150 rows
        for gp in agent.graph_gps.values():
            assert gp.X.shape[0] == 150 and gp.optimization_result.optimizer == "device" and len(gp.optimization_result.runs) == 2
        for c in calls.values():
            c.clear()
        agent.intervene()                                                     # its closing optimize(): one call, a small model
        assert calls["rows"] == [(1, 256)] and not calls["sets"] and not calls["batch"]
        # the default: the launch declines both graph GPs and the lockstep route evaluates them, today's counts
        for c in calls.values():
            c.clear()
        plain = toy_agent(mle_optimizer="device")
        plain.graph_gps = plain.graph.fit_all_gaussian_processes(plain.measurements, lockstep=plain.lockstep, **plain._mle_kwargs())
        first = {k: list(v) for k, v in calls.items()}
        plain.observe()
    assert not calls["rows"] and calls["sets"] == [2, 2] and first["sets"] == [2] and first["batch"]
    assert len(calls["batch"]) > len(first["batch"]) and max(calls["batch"]) == 2      # (a model that has ended drops out)
    for gp in plain.graph_gps.values():
        assert not hasattr(gp.optimization_result, "optimizer")
