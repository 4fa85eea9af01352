"""CPU tests of the one-launch hyper-parameter MLE: the search logic of csrc/mle_search.h driven on the
host by tests/support/mle_search_sim.cpp (g++, no HIP) against ``lockstep_lbfgs`` with an infinite box on the same
function, the entry point's declaration and binding, the restarts' draws, the choice of the best run and the argument
checks of the Python layers."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, logexp_finv, logexp_gradfactor
from cbo_with_oop_amd.utils_functions.causal_optimizer import lockstep_lbfgs

gpf = importlib.import_module("cbo_with_oop_amd.GaussianProcessFactory")       # (the package exports the class by that name)

SOURCE = os.path.join(ROOT, "tests", "support", "mle_search_sim.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cbo_with_oop_amd", "csrc")]
hexes = lambda a: " ".join(float(v).hex() for v in np.ravel(a))                                  # noqa: E731
INPUTS = []          # every text the simulator was given: the sanitizer build at the end runs them again


def _build(exe, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, *INCLUDES, SOURCE, "-o", str(exe)])


def _run(exe, text):
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """run(P, start, kind, extra, max_rounds=200, nan_at=-1, start_is_x=1, extra_feeds=0) -> dict(points [(x, lml, moved)],
    status, rounds, lml, theta, grad, x) of one search of the state machine, every number exchanged as a hexadecimal float."""
    exe = tmp_path_factory.mktemp("mle_sim") / "mle_search_sim"
    _build(exe)

    def run(P, start, kind, extra, max_rounds=200, nan_at=-1, start_is_x=1, extra_feeds=0):
        text = f"{P} {max_rounds} {nan_at} {start_is_x} {extra_feeds}\n{hexes(start)}\n{kind}\n{extra}\n"
        INPUTS.append(text)
        points, end = [], None
        for line in _run(exe, text).stdout.splitlines():
            tok = line.split()
            if tok[0] == "P":
                v = [float.fromhex(t) for t in tok[1:-1]]
                points.append((np.array(v[:P]), v[P], tok[-1] == "1"))
            else:
                v = [float.fromhex(t) for t in tok[3:]]
                end = dict(status=int(tok[1]), rounds=int(tok[2]), lml=v[0], theta=np.array(v[1:1 + P]),
                           grad=np.array(v[1 + P:1 + 2 * P]), x=np.array(v[1 + 2 * P:1 + 3 * P]), line=line)
        return dict(end, points=points)
    return run


# ---- the two objectives, as functions of x for lockstep_lbfgs (it maximises: value = lml, gradient = dlml/dtheta * dtheta/dx)

def quad_of(w, c):
    w, c = np.asarray(w, dtype=np.float64), np.asarray(c, dtype=np.float64)

    def lml(theta):
        r = np.log(theta) - c
        return -np.sum(w * r * r / 2.0, axis=-1), -(w * r) / theta
    return lml


def rosen_of(b):
    def lml(theta):
        u = np.log(theta)
        du = np.zeros_like(u)
        v, o = u[..., 1:] - u[..., :-1] ** 2, 1.0 - u[..., :-1]
        total = np.sum(b * v * v + o * o, axis=-1) + (1.0 - u[..., -1]) ** 2 / 2.0
        du[..., :-1] += -4.0 * b * v * u[..., :-1] - 2.0 * o
        du[..., 1:] += 2.0 * b * v
        du[..., -1] -= 1.0 - u[..., -1]
        return -total, -du / theta
    return lml


def reference(lml_of_theta, x0, max_rounds=200, perturb=None):
    """``lockstep_lbfgs`` with an infinite box from x0 on the objective; returns (x_end, lml_end, trials [(x, lml)],
    decisions): decisions[r - 1] says whether round r's trial passed the Armijo test -- replayed from the recorded values
    with the very expression lockstep_lbfgs evaluates.  ``perturb`` (a Generator): every evaluation is taken at
    x (1 + 4 eps r), r uniform in [-1, 1] -- the recipe of the bar."""
    trials = []

    def fun(X):
        Xe = X if perturb is None else X * (1.0 + 4.0 * np.finfo(np.float64).eps * perturb.uniform(-1.0, 1.0, X.shape))
        theta = logexp_f(Xe)
        v, dl = lml_of_theta(theta)
        g = dl * logexp_gradfactor(theta)
        trials.append((X[0].copy(), float(v[0]), g[0].copy()))
        return v, g

    P = len(x0)
    X, F = lockstep_lbfgs(fun, np.array([x0], dtype=np.float64), np.full(P, -np.inf), np.full(P, np.inf), max_rounds=max_rounds)
    # lockstep_lbfgs evaluates finished searches along with the others: with one search it stops instead, nothing to trim
    decisions = []
    base_x, base_f, base_g = trials[0][0], -trials[0][1], -trials[0][2]
    for x, v, g in trials[1:]:
        ft = -v
        ok = bool(np.isfinite(ft)) and not ft > base_f + 1e-4 * base_g.dot(x - base_x)
        decisions.append(ok)
        if ok:
            base_x, base_f, base_g = x, ft, -g
    assert np.array_equal(X[0], base_x)                          # the replay ends where lockstep_lbfgs ended
    return X[0], float(F[0]), trials, decisions


def relative(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def bar_of(lml_of_theta, x0, ref):
    """64 x the largest relative deviation of lockstep_lbfgs' own end point (theta and lml) under the perturbed
    evaluations, three seeds, not below 1e-12.  A perturbed run must take the decisions of the clean one: a case where it
    does not is badly chosen (another start, not a wider bar)."""
    x_ref, f_ref, _, dec_ref = ref
    worst = 0.0
    for seed in (1, 2, 3):
        xp, fp, _, dec = reference(lml_of_theta, x0, perturb=np.random.default_rng(seed))
        assert dec == dec_ref, "a perturbed reference run changed a decision: choose another start for this case"
        worst = max(worst, relative(logexp_f(xp), logexp_f(x_ref)), abs(fp - f_ref) / max(1.0, abs(f_ref)))
    return max(64.0 * worst, 1e-12), worst


CASES = [
    ("quad", 1, dict(w=[2.0], c=[0.5]), [1.5]),
    ("quad", 2, dict(w=[1.0, 6.0], c=[-0.5, 1.0]), [0.25, -0.75]),
    ("quad", 3, dict(w=[0.5, 2.0, 9.0], c=[0.25, -1.0, 0.75]), [1.0, 1.0, -0.5]),
    ("quad", 10, dict(w=[0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0],
                      c=[0.1, -0.2, 0.3, -0.4, 0.5, -0.6, 0.7, -0.8, 0.9, -1.0]), [0.5] * 10),
    ("rosen", 1, dict(b=4.0), [0.25]),
    ("rosen", 2, dict(b=4.0), [0.5, 1.5]),
    ("rosen", 3, dict(b=4.0), [0.5, 1.5, 1.0]),
    ("rosen", 10, dict(b=2.0), [1.2, 0.8, 1.1, 0.9, 1.3, 0.7, 1.0, 1.2, 0.8, 1.1]),
]


def objective(kind, params):
    if kind == "quad":
        return quad_of(params["w"], params["c"]), f"{hexes(params['w'])}\n{hexes(params['c'])}"
    return rosen_of(params["b"]), hexes([params["b"]])


@pytest.mark.parametrize("kind,P,params,x0", CASES, ids=[f"{k}-{p}" for k, p, _, _ in CASES])
def test_the_state_machine_follows_lockstep_lbfgs_round_for_round(sim, kind, P, params, x0):
    lml_of_theta, extra = objective(kind, params)
    ref = reference(lml_of_theta, x0)
    x_ref, f_ref, trials, decisions = ref
    bar, worst = bar_of(lml_of_theta, x0, ref)
    got = sim(P, x0, kind, extra)
    moved = [m for _, _, m in got["points"]]
    print(f"{kind} P={P}: rounds {got['rounds']} (reference {len(trials) - 1}), accepted {sum(decisions)}, "
          f"perturbed reference deviation {worst:.3e}, bar {bar:.3e}, "
          f"theta deviation {relative(got['theta'], logexp_f(x_ref)):.3e}, "
          f"lml deviation {abs(got['lml'] - f_ref) / max(1.0, abs(f_ref)):.3e}")
    assert got["rounds"] == len(trials) - 1 and len(got["points"]) == len(trials)
    assert moved[0] and moved[1:] == decisions                   # the same accept / halve decision every round
    assert got["status"] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP)
    assert relative(got["theta"], logexp_f(x_ref)) <= bar
    assert abs(got["lml"] - f_ref) <= bar * max(1.0, abs(f_ref))
    # the reported state is consistent: theta is Logexp.f of the reported x, lml and gradient are the objective's there
    assert np.allclose(got["theta"], logexp_f(got["x"]), rtol=1e-15, atol=0.0)
    v, dl = lml_of_theta(got["theta"])
    assert np.isclose(got["lml"], v, rtol=1e-13, atol=1e-300) and np.allclose(got["grad"], dl, rtol=1e-12, atol=1e-14)
    if got["status"] == _lib.REFINE_PGTOL:
        assert np.max(np.abs(got["grad"] * logexp_gradfactor(got["theta"]))) <= 1e-5


def test_a_long_run_wraps_the_rings(sim):
    """More than 8 accepted steps at P = 10: pairs are overwritten oldest first, the trajectory stays lockstep_lbfgs'."""
    kind, P, params, x0 = CASES[-1]
    lml_of_theta, extra = objective(kind, params)
    _, _, trials, decisions = reference(lml_of_theta, x0)
    got = sim(P, x0, kind, extra)
    assert sum(decisions) > 8 and sum(m for _, _, m in got["points"][1:]) == sum(decisions)
    # ... and a bound on the rounds ends it where the reference stands after as many
    x_cut, f_cut, cut_trials, _ = reference(lml_of_theta, x0, max_rounds=12)
    cut = sim(P, x0, kind, extra, max_rounds=12)
    assert (cut["status"], cut["rounds"], len(cut_trials)) == (_lib.REFINE_MAX_ROUNDS, 12, 13)
    assert np.allclose(cut["x"], x_cut, rtol=1e-9) and np.isclose(cut["lml"], f_cut, rtol=1e-9)


def test_non_finite_values_and_bounded_rounds(sim):
    lml_of_theta, extra = objective("quad", CASES[2][2])
    x0 = CASES[2][3]
    # a NaN start ends the search there
    got = sim(3, x0, "quad", extra, nan_at=0)
    assert (got["status"], got["rounds"], len(got["points"])) == (_lib.REFINE_NAN_START, 0, 1)
    assert np.isnan(got["lml"]) and np.array_equal(got["x"], x0)
    # a NaN trial is an Armijo failure: the next trial is half as far along the same direction, the accepted point stays
    clean = sim(3, x0, "quad", extra)
    got = sim(3, x0, "quad", extra, nan_at=1)
    (p0, _, _), (p1, v1, m1), (p2, _, _) = got["points"][:3]
    assert np.isnan(v1) and not m1 and np.array_equal(p1, clean["points"][1][0])
    assert np.allclose(p2 - p0, 0.5 * (p1 - p0), rtol=1e-12, atol=0.0)
    assert got["status"] in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL) and np.isfinite(got["lml"])
    assert np.allclose(got["theta"], clean["theta"], rtol=1e-4)
    # max_rounds = 0: the start is evaluated, nothing moves
    got = sim(3, x0, "quad", extra, max_rounds=0)
    assert (got["status"], got["rounds"], len(got["points"])) == (_lib.REFINE_MAX_ROUNDS, 0, 1)
    assert np.array_equal(got["x"], x0) and got["lml"] == got["points"][0][1]
    # feeding a finished search changes nothing
    assert sim(3, x0, "quad", extra, extra_feeds=3)["line"] == clean["line"]
    assert sim(3, x0, "quad", extra, max_rounds=0, extra_feeds=2)["line"] == got["line"]
    # from parameters instead of a position: the search transforms them itself
    theta0 = logexp_f(np.array(x0))
    got = sim(3, theta0, "quad", extra, start_is_x=0, max_rounds=0)
    assert np.allclose(got["x"], logexp_finv(theta0), rtol=1e-15) and np.allclose(got["theta"], theta0, rtol=1e-15)


def test_the_sanitized_simulator_runs_the_tests_inputs_clean(sim, tmp_path):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in (a stand-alone build: nothing is
    preloaded), on every input the tests above gave it."""
    for kind, P, params, x0 in CASES:                            # (whatever ran before: these inputs at the least)
        sim(P, x0, kind, objective(kind, params)[1])
    sim(3, CASES[2][3], "quad", objective("quad", CASES[2][2])[1], nan_at=1, extra_feeds=2)
    exe = tmp_path / "mle_search_sim_san"
    _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for text in INPUTS:
        out = _run(exe, text)
        assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr


# ---- the restarts' draws, the best run, the argument checks -------------------------------------------------------------

def test_mle_restart_starts():
    np.random.seed(11)
    rows = gpf.mle_restart_starts(4, 5)
    after = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(11)
    expect = [np.random.randn(4) for _ in range(4)]
    assert rows.shape == (4, 4) and np.array_equal(rows, np.array(expect))
    # the generator is left where (num_restarts - 1) calls of randn(P) leave it
    state = np.random.get_state()
    assert np.array_equal(after[0], state[1]) and after[1] == state[2]
    # one start draws nothing
    np.random.seed(11)
    before = np.random.get_state()
    assert gpf.mle_restart_starts(4, 1).shape == (0, 4)
    now = np.random.get_state()
    assert np.array_equal(before[1], now[1]) and before[2] == now[2]


def test_the_best_run():
    ok, nan_start, not_pd = _lib.REFINE_FTOL, _lib.REFINE_NAN_START, _lib.MLE_NOT_PD
    assert gpf.mle_best_run([1.0, 3.0, 2.0], [ok] * 3) == 1
    assert gpf.mle_best_run([3.0, 1.0, 3.0], [ok] * 3) == 0                       # ties go to the lowest index
    assert gpf.mle_best_run([np.nan, -7.0, np.nan], [ok] * 3) == 1                # a NaN never wins
    assert gpf.mle_best_run([np.nan, 5.0, 1.0], [ok, not_pd, _lib.REFINE_MAX_ROUNDS]) == 2
    assert gpf.mle_best_run([np.nan, np.nan], [nan_start, not_pd]) is None        # all failed: the start is kept
    assert gpf.mle_best_run([-np.inf, np.nan], [ok, nan_start]) == 0


def test_argument_checks_come_before_any_device_call():
    for bad in ("gpu", None, 1):
        with pytest.raises(ValueError, match="optimizer"):
            gpf.checked_mle_optimizer(bad)
        with pytest.raises(ValueError, match="optimizer"):
            gpf.optimize_together([], optimizer=bad)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="num_restarts"):
            gpf.checked_mle_optimizer("device", bad)
    with pytest.raises(ValueError, match="num_restarts"):
        gpf.optimize_together([], num_restarts=2)                                  # restarts on the host route: out of scope
    with pytest.raises(ValueError, match="transform"):
        gpf.optimize_together([], transform="log", optimizer="device")
    assert gpf.optimize_together([], optimizer="device") == []
    from cbo_with_oop_amd.CBO import CBO, CBOAcquisitionPath
    with pytest.raises(ValueError, match="optimizer"):
        CBOAcquisitionPath(None, [["X"]], None, "min", [], [], [None], mle_optimizer="scipy")
    with pytest.raises(ValueError, match="num_restarts"):
        CBOAcquisitionPath(None, [["X"]], None, "min", [], [], [None], mle_optimizer="host", mle_restarts=4)
    with pytest.raises(ValueError, match="optimizer"):
        CBO(None, None, None, None, mle_optimizer="scipy")
    from cbo_with_oop_amd.utils_functions.utils import fit_gaussian_process, fit_gaussian_processes
    with pytest.raises(ValueError, match="optimizer"):
        fit_gaussian_process(None, None, None, optimizer="scipy")
    with pytest.raises(ValueError, match="num_restarts"):
        fit_gaussian_processes([], [], [], num_restarts=3)


def test_the_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert re.search(r"int cbo_gp_mle_sets\(int n_models, cbo_gp \*const \*gps, const cbo_mle_run \*runs, "
                     r"int \*model_status_out\);", header)
    assert "cbo_gp_mle_sets" in _lib.SIGNATURES
    for name, value in (("CBO_MLE_MAX_STARTS", _lib.MLE_MAX_STARTS), ("CBO_MLE_MAX_ROUNDS", _lib.MLE_MAX_ROUNDS),
                        ("CBO_MLE_NOT_PD", _lib.MLE_NOT_PD)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert re.search(r"#define CBO_MLE_DECLINED CBO_REFINE_DECLINED", header) and _lib.MLE_DECLINED == _lib.REFINE_DECLINED
    assert _lib.MLE_NOT_PD not in (_lib.REFINE_PGTOL, _lib.REFINE_FTOL, _lib.REFINE_STEP, _lib.REFINE_MAX_ROUNDS,
                                   _lib.REFINE_NAN_START, _lib.REFINE_DECLINED)
    fields = [f for f, _ in _lib.CboMleRun._fields_]
    assert fields == ["n_params", "fit_noise", "n_starts", "max_rounds", "theta0", "theta_out", "lml_out", "grad_out",
                      "status_out", "rounds_out"]
