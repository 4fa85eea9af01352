"""CPU tests of the one-launch HMC sampler: the chain of csrc/hmc_chain.h driven on the host by
tests/support/hmc_chain_sim.cpp (g++, no HIP) against ``hmc_sample_from_draws`` on the same closed-form objective, the
draw order of ``hmc_draws`` against ``hmc_sample``, and the constructors' sampler switches."""
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cbo_with_oop_amd import CBO as cbo_module
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.GaussianProcessFactory import logexp_f, logexp_finv
from cbo_with_oop_amd.utils_functions.integrated_hyper import (IntegratedHyperParameterAcquisition, hmc_draws, hmc_sample,
                                                                hmc_sample_from_draws)

LOG_LIM = math.log(np.finfo(np.float64).max)


def hexes(a):
    return " ".join(float(v).hex() for v in np.ravel(a))


def sim_input(theta0, a, b, momenta, uniforms, hmc_iters, stepsize, nan_at=-1, start_is_x=False):
    """The simulator's stdin for one chain (also what a stand-alone sanitizer run of it reads)."""
    return (f"{len(theta0)} {len(uniforms)} {hmc_iters} {nan_at} {int(start_is_x)}\n{hexes([stepsize])}\n{hexes(theta0)}\n{hexes(a)}\n{hexes(b)}\n"
            f"{hexes(momenta)}\n{hexes(uniforms)}\n")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """run(theta0, a, b, momenta, uniforms, hmc_iters, stepsize, nan_at=-1, start_is_x=False) -> (positions [x per evaluation], rows, accept
    flags, (evaluations, theta, lml, dlml)) of one chain of the state machine."""
    exe = tmp_path_factory.mktemp("hmc_sim") / "hmc_chain_sim"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbo_with_oop_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "hmc_chain_sim.cpp"), "-o", str(exe)])

    def run(theta0, a, b, momenta, uniforms, hmc_iters, stepsize, nan_at=-1, start_is_x=False):
        P = len(theta0)
        out = subprocess.run([str(exe)],
                             input=sim_input(theta0, a, b, momenta, uniforms, hmc_iters, stepsize, nan_at, start_is_x),
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.returncode, out.stderr)
        positions, rows, flags, final = [], [], [], None
        for line in out.stdout.splitlines():
            tok = line.split()
            v = [float.fromhex(t) for t in tok[2:]] if tok[0] != "S" else [float.fromhex(t) for t in tok[3:]]
            if tok[0] == "X":
                assert int(tok[1]) == len(positions)
                positions.append(np.array(v))
            elif tok[0] == "S":
                assert int(tok[1]) == len(rows)
                flags.append(tok[2] == "1")
                rows.append(v)
            else:
                final = (int(tok[1]), np.array(v[:P]), v[P], np.array(v[P + 1:]))
        return positions, np.array(rows), np.array(flags), final
    return run


def quadratic(a, b, nan_at=-1):
    """The simulator's objective in Python, operation for operation, with libm's transform (``math``): (-lml, -dlml/dtheta
    (1 - exp(-theta))) as a function of x, and the list of the positions it was asked for."""
    asked = []

    def objective(x):
        e = len(asked)
        asked.append(np.array(x, dtype=np.float64))
        lml, g = 0.0, []
        for k, xk in enumerate(np.asarray(x, dtype=np.float64).tolist()):
            th = xk if xk > 36.0 else math.log1p(math.exp(max(xk, -LOG_LIM)))
            lml = lml + ((a[k] * th) * th / 2.0 + b[k] * th)
            dl = -(a[k] * th + b[k])
            g.append(-(dl * (1.0 if th > 36.0 else -math.expm1(-th))))
        lml = -lml
        if e == nan_at:
            lml = float("nan")
        return -lml, np.array(g)
    return objective, asked


# dyadic coefficients: the products with theta and the sums stay a few operations each on both sides
CHAINS = [
    # (P, a, b, theta0, stepsize, hmc_iters, num_samples, seed)
    (1, [0.5], [-1.25], [1.5], 0.125, 3, 8, 1),
    (3, [0.5, 2.0, 0.25], [-1.0, -3.5, 0.5], [1.2, 0.9, 0.04], 0.0625, 3, 8, 2),
    (10, [0.5, 1.0, 2.0, 0.25, 4.0, 0.5, 1.5, 0.75, 1.0, 8.0], [-1.0, -0.5, -3.0, 0.25, -2.0, -1.5, 0.5, -0.75, -2.0, -0.5],
     np.linspace(0.3, 2.1, 10).tolist(), 0.03125, 3, 8, 3),
    # steps long enough for rejections
    (3, [8.0, 16.0, 4.0], [-8.0, -4.0, -2.0], [1.2, 0.9, 0.4], 0.5, 4, 24, 4),
    (1, [32.0], [-16.0], [0.7], 0.375, 5, 24, 5),
    # hmc_iters = 0: no proposal moves; u < 1 accepts
    (3, [0.5, 2.0, 0.25], [-1.0, -3.5, 0.5], [1.2, 0.9, 0.04], 0.0625, 0, 5, 6),
]


def draws_for(P, num, seed):
    np.random.seed(seed)
    return hmc_draws(P, num)


def compare(sim, P, a, b, theta0, stepsize, hmc_iters, num, seed, nan_at=-1):
    """The start: numpy's ``log(expm1(theta0))`` and libm's differ by a few ulp, as the two ``log1p(exp(x))`` of the rows do,
    and a chain that starts elsewhere is elsewhere at every position.  So the simulator's own start is held to 4 ulp of
    numpy's, like the rows, and the chain compared bit for bit is the one it runs from numpy's start."""
    momenta, uniforms = draws_for(P, num, seed)
    objective, asked = quadratic(a, b, nan_at)
    rows, flags, ks = hmc_sample_from_draws(objective, theta0, momenta, uniforms, hmc_iters, stepsize)
    x0 = logexp_finv(np.array(theta0))
    own = sim(theta0, a, b, momenta, uniforms, 0, stepsize)[0][0]
    assert np.all(np.abs(own - x0) <= 4 * np.spacing(np.abs(x0))), (own, x0)
    positions, s_rows, s_flags, (evals, theta, lml, dlml) = sim(x0, a, b, momenta, uniforms, hmc_iters, stepsize, nan_at,
                                                                 start_is_x=True)
    assert evals == 1 + num * hmc_iters == len(positions) == len(asked)       # once per position
    assert np.array_equal(s_flags, flags)                                     # the accept decisions
    for e, (p, q) in enumerate(zip(positions, asked)):                        # every earlier decision agreed: bit for bit
        assert np.array_equal(p.view(np.uint64), q.view(np.uint64)), (e, p, q)
    ulp = np.spacing(np.abs(rows))
    assert np.all(np.abs(s_rows - rows) <= 4 * ulp), np.max(np.abs(s_rows - rows) / ulp)
    assert np.all(np.abs(theta - rows[-1]) <= 4 * np.spacing(np.abs(rows[-1])))   # the last state is the last row
    return flags, ks, s_rows, (theta, lml, dlml)


@pytest.mark.parametrize("P,a,b,theta0,stepsize,hmc_iters,num,seed", CHAINS[:3])
def test_the_state_machine_follows_hmc_sample_from_draws_position_for_position(sim, P, a, b, theta0, stepsize, hmc_iters, num,
                                                                               seed):
    compare(sim, P, a, b, theta0, stepsize, hmc_iters, num, seed)


def test_chains_that_accept_and_reject_decide_alike_and_a_nan_position_rejects_its_sample(sim):
    for chain in CHAINS[3:5]:
        flags, ks, _, _ = compare(sim, *chain)
        assert flags.any() and not flags.all()                               # both kinds of decision
        assert np.all(ks[~flags] < 1.0)
    # NaN at evaluation 6 = sample 1's proposal (3 steps per sample; H_new is NaN): that sample is rejected, the chain goes on
    P, a, b, theta0, stepsize, hmc_iters, num, seed = CHAINS[1]
    clean, _, clean_rows, _ = compare(sim, P, a, b, theta0, stepsize, hmc_iters, num, seed)
    flags, ks, rows, _ = compare(sim, P, a, b, theta0, stepsize, hmc_iters, num, seed, nan_at=6)
    assert clean[1] and not flags[1] and np.isnan(ks[1])
    assert flags[0] == clean[0] and np.array_equal(rows[0], clean_rows[0]) and flags[2:].any()
    assert np.all(np.isfinite(rows))


def test_no_leapfrog_steps_keep_every_row_at_the_start(sim):
    P, a, b, theta0, stepsize, hmc_iters, num, seed = CHAINS[5]
    momenta, uniforms = draws_for(P, num, seed)
    uniforms[2] = 1.0                                                       # u < 1 fails: the one rejection
    positions, rows, flags, (evals, theta, _, _) = sim(theta0, a, b, momenta, uniforms, hmc_iters, stepsize)
    assert evals == 1 and len(positions) == 1
    assert flags.tolist() == [True, True, False, True, True]
    assert np.all(rows == rows[0]) and np.array_equal(theta, rows[0])
    assert np.all(np.abs(rows[0] - np.array(theta0)) <= 4 * np.spacing(np.array(theta0)))


@pytest.mark.parametrize("P,num,hmc_iters", [(1, 7, 2), (3, 12, 3), (10, 5, 0)])
def test_hmc_draws_are_hmc_samples_own_draws_in_its_own_order(P, num, hmc_iters):
    a, b = np.linspace(0.5, 2.0, P), np.linspace(-1.0, 0.5, P)
    theta0 = np.linspace(0.4, 1.9, P)
    np.random.seed(77)
    want = hmc_sample(quadratic(a, b)[0], theta0, num, hmc_iters, 0.3)
    state_want = np.random.get_state()
    np.random.seed(77)
    momenta, uniforms = hmc_draws(P, num)
    state_got = np.random.get_state()
    assert momenta.shape == (num, P) and uniforms.shape == (num,)
    rows, flags, ks = hmc_sample_from_draws(quadratic(a, b)[0], theta0, momenta, uniforms, hmc_iters, 0.3)
    assert np.array_equal(rows.view(np.uint64), want.view(np.uint64))
    assert flags.dtype == bool and flags.shape == ks.shape == (num,)
    assert state_want[0] == state_got[0] and np.array_equal(state_want[1], state_got[1]) and state_want[2:] == state_got[2:]
    assert np.array_equal(logexp_f(np.zeros(1)), [math.log(2.0)])


def test_the_sampler_switches_are_checked_in_the_constructors_before_any_device_call():
    obj = object()
    path = lambda **kw: cbo_module.CBOAcquisitionPath(obj, [["X"], ["Z"]], obj, "min", [obj, obj], [obj, obj], [obj, obj],   # noqa: E731
                                                      comm=None, **kw)
    assert path().hyper_sampler == "host" and path(hyper_samples=3, hyper_sampler="device").hyper_sampler == "device"
    for bad in ("gpu", None, True, 1):
        with pytest.raises(ValueError, match="hyper_sampler"):
            path(hyper_samples=3, hyper_sampler=bad)
    with pytest.raises(ValueError, match="callable"):
        path(hyper_samples=lambda model, s: None, hyper_sampler="device")
    assert path(hyper_samples=lambda model, s: None).hyper_sampler == "host"
    from cbo_with_oop_amd.graphs import CompleteGraph
    es = CompleteGraph.get_exploration_set("MIS")
    data = [(np.zeros((3, len(s))), np.zeros((3, 1))) for s in es]
    make = lambda **kw: cbo_module.CBO(CompleteGraph, {"A": np.zeros((2, 1))}, {"A": np.zeros((2, 1))}, data, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="hyper_sampler"):
        make(hyper_samples=2, hyper_sampler="both")
    with pytest.raises(ValueError, match="callable"):
        make(hyper_samples=lambda model, s: None, hyper_sampler="device")
    for cls in (cbo_module.CBOAcquisitionPath, cbo_module.CBO):
        assert inspect.signature(cls.__init__).parameters["hyper_sampler"].default == "host"
    assert inspect.signature(IntegratedHyperParameterAcquisition.__init__).parameters["sampler"].default == "host"
    with pytest.raises(ValueError, match="sampler"):
        IntegratedHyperParameterAcquisition(obj, lambda model: None, sampler="gpu")
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    assert inspect.signature(HipGaussianProcess.generate_hyperparameters_samples).parameters["sampler"].default == "host"


def test_the_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cbo_hip.h")).read()
    assert "int cbo_gp_hmc_sets(int n_models, cbo_gp *const *gps, const cbo_hmc_chain *chains, int *status_out);" in header
    assert "cbo_gp_hmc_sets" in _lib.SIGNATURES
    assert f"#define CBO_HMC_MAX_SAMPLES {_lib.HMC_MAX_SAMPLES}\n" in header
    assert f"#define CBO_HMC_MAX_EVALS {_lib.HMC_MAX_EVALS}\n" in header
    assert (_lib.HMC_OK, _lib.HMC_NOT_PD, _lib.HMC_DECLINED) == (0, 1, 2)
    assert "enum { CBO_HMC_OK = 0, CBO_HMC_NOT_PD = 1, CBO_HMC_DECLINED = 2 };" in header
    assert _lib.HMC_MAX_PARAMS == _lib.MAX_DIM + 2
    fields = [name for name, _ in _lib.CboHmcChain._fields_]
    assert fields == ["n_params", "sample_noise", "num_samples", "hmc_iters", "stepsize", "theta0", "momenta", "uniforms",
                      "rows_out", "accept_out", "final_theta", "final_lml", "final_grad"]
