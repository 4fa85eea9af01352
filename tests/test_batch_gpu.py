"""GPU tests of greedy batch selection (cbo_acq_sweep_batch: the kernels of kernels_batch.hip behind the EI / arg-max
epilogue; contract in include/cbo_hip.h and DESIGN.md 4g).

Shapes: n in {37, 128, 129, 300} (one ragged slice of the pass over V, the last row of a 64-row slice, the first row of the
next, several slices with a ragged last one), m in {1, 5, 63, 257, 1000} (one candidate, B = m, an odd count below one
strip, more than one workgroup of the final stage, more than one 512-column workgroup of the pass), d in {1, 3}.

Accuracy is judged by conftest.assert_parity against the 80-bit refit (oracle.truth) of the data the believer would have:
|hip - truth| <= 1e-5 + 8 |oracle - truth|, the bar of every other parity test here.  The restatement of emukit's loop the
picks are compared with is test_batch_host.believer."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, assert_parity, load_fixture
from oracle import gp_oracle as O
from oracle.truth import truth_predict
from test_batch_host import believer

pytestmark = pytest.mark.gpu

INVALID, NOT_FITTED, UNSUPPORTED = -1, -5, -6
HYPER = dict(variance=1.3, lengthscale=0.9, noise_var=1e-3)


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def mean_fn(a):
    return 0.3 * np.sin(a).sum(1, keepdims=True)


def var_fn(a):
    return 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2


def make_case(n, m, d, causal, seed=0, dtype="f64", offset=0, keep=False, fit=True):
    """(model, grid, data dict) of a random problem; the data dict is what the oracle needs."""
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(1000 * n + 10 * m + d + seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.cos(1.5 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.5, 2.5, (m, d))
    kw = dict(mean_function=mean_fn, variance_adjustment=var_fn) if causal else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        g = HipGaussianProcess(X, y, dtype=dtype, fit=fit, **HYPER, **kw)
    grid = CandidateGrid(Xs, g, index_offset=offset, keep_solution=keep)
    data = dict(X=X, y=y, Xs=Xs, mX=mean_fn(X) if causal else None, vX=var_fn(X) if causal else None,
                mXs=mean_fn(Xs) if causal else None, vXs=var_fn(Xs) if causal else None)
    return g, grid, data


def batch(lib, g, grid, y_best, task, B, cost=1.0, jitter=0.0, update=0, want=True, vals=True, idxs=True):
    """cbo_acq_sweep_batch: (rc, best_vals, best_idxs, acq, mean, var)."""
    m = len(grid)
    acq, mean, var = (np.empty(m), np.empty(m), np.empty(m)) if want else (None, None, None)
    n_out = max(int(B), 1) if isinstance(B, int) else 1
    bv = np.full(n_out, np.nan) if vals else None
    bi = np.full(n_out, -1, dtype=np.int64) if idxs else None
    rc = lib.load().cbo_acq_sweep_batch(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task] if isinstance(task, str) else task,
                                        float(jitter), float(cost), B, update, lib.dptr(bv),
                                        bi.ctypes.data_as(lib.c_int64_p) if idxs else None, lib.dptr(acq), lib.dptr(mean),
                                        lib.dptr(var))
    return rc, bv, bi, acq, mean, var


def plain(lib, g, grid, y_best, task, cost=1.0, jitter=0.0):
    """cbo_acq_sweep: (acq, mean, var, best_val, best_idx)."""
    m = len(grid)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                       float(cost), lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                       ctypes.byref(bi)))
    return acq, mean, var, bv.value, bi.value


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# (n, m, d, B, causal, task, index_offset)
CASES = [(37, 1, 1, 1, False, "min", 0),
         (37, 5, 1, 5, False, "min", 0),                  # B = m
         (128, 63, 3, 2, True, "min", 0),
         (129, 257, 1, 5, False, "max", 0),
         (129, 63, 1, 5, True, "max", 7),
         (300, 1000, 3, 5, True, "min", 0),
         (300, 257, 3, 2, False, "min", 100000),
         (128, 1000, 1, 2, False, "min", 0)]


@pytest.mark.parametrize("n,m,d,B,causal,task,offset", CASES)
def test_pick_0_and_batch_of_one_are_the_plain_sweeps_bits(lib, n, m, d, B, causal, task, offset):
    g, grid, data = make_case(n, m, d, causal, offset=offset)
    y_best = float(data["y"].min() if task == "min" else data["y"].max())
    acq, mean, var, bv, bi = plain(lib, g, grid, y_best, task, cost=2.0, jitter=0.01)
    rc, vals, idxs, acq1, mean1, var1 = batch(lib, g, grid, y_best, task, 1, cost=2.0, jitter=0.01)
    assert rc == 0
    assert same_bits(vals[0], bv) and idxs[0] == bi
    assert same_bits(acq1, acq) and same_bits(mean1, mean) and same_bits(var1, var)
    rc, vals, idxs, _, mean_b, _ = batch(lib, g, grid, y_best, task, B, cost=2.0, jitter=0.01)
    assert rc == 0
    assert same_bits(vals[0], bv) and idxs[0] == bi
    assert same_bits(mean_b, mean)                                 # the believed residual is zero: mu never moves
    assert np.all((idxs >= offset) & (idxs < offset + m))
    grid.close()


def check_model_untouched(lib, keep, n=300, m=257, d=3, causal=True):
    """cbo_acq_sweep and cbo_gp_get_posterior before and after a B = 5 call, and two B = 5 calls."""
    g, grid, data = make_case(n, m, d, causal, keep=keep)
    y_best = float(data["y"].min())
    L0, a0 = np.empty((n, n)), np.empty(n)
    lib.check(lib.load().cbo_gp_get_posterior(g._handle, lib.dptr(L0), lib.dptr(a0)))
    before = plain(lib, g, grid, y_best, "min")
    rc, vals, idxs, acq, mean, var = batch(lib, g, grid, y_best, "min", 5)
    assert rc == 0
    after = plain(lib, g, grid, y_best, "min")
    for x, z in zip(before, after):
        assert same_bits(x, z)
    L1, a1 = np.empty((n, n)), np.empty(n)
    lib.check(lib.load().cbo_gp_get_posterior(g._handle, lib.dptr(L1), lib.dptr(a1)))
    assert same_bits(L0, L1) and same_bits(a0, a1)
    rc, vals2, idxs2, acq2, mean2, var2 = batch(lib, g, grid, y_best, "min", 5)
    assert rc == 0
    assert same_bits(vals, vals2) and np.array_equal(idxs, idxs2)
    assert same_bits(acq, acq2) and same_bits(mean, mean2) and same_bits(var, var2)
    # a fresh candidate set (nothing cached, nothing kept) gives the same batch
    g2, grid2, _ = make_case(n, m, d, causal, keep=False)
    rc, vals3, idxs3, _, _, var3 = batch(lib, g2, grid2, y_best, "min", 5)
    assert rc == 0 and np.array_equal(idxs, idxs3) and same_bits(vals, vals3) and same_bits(var, var3)
    grid.close(); grid2.close()
    return True


@pytest.mark.parametrize("keep", [False, True])
def test_the_model_and_the_candidates_are_left_as_they_were(lib, keep):
    assert check_model_untouched(lib, keep)


def run_child(code, **env):
    """A fresh process (the knobs are read at cbo_init): returns its stdout; its failure is the test's."""
    full = dict(os.environ)
    full.update(env)
    prelude = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
    r = subprocess.run([sys.executable, "-c", prelude + code], env=full, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_the_model_is_left_alone_without_the_sweep_cache(lib):
    out = run_child("import test_batch_gpu as t\nfrom cbo_with_oop_amd import _lib\n"
                    "print('ok', t.check_model_untouched(_lib, False), t.check_model_untouched(_lib, True))\n",
                    CBO_HIP_SWEEP_CACHE="0")
    assert "ok True True" in out


@pytest.mark.parametrize("n,m,d,B,causal,task,offset", CASES)
def test_last_pick_against_the_long_double_refit(lib, n, m, d, B, causal, task, offset):
    g, grid, data = make_case(n, m, d, causal, offset=offset)
    X, y, Xs = data["X"], data["y"], data["Xs"]
    y_best = float(y.min() if task == "min" else y.max())
    rc, vals, idxs, acq, mean, var = batch(lib, g, grid, y_best, task, B)
    assert rc == 0
    picks = (idxs - offset)[:B - 1]                               # the device's own picks: no near-tie decides this check
    tk = dict(variance=HYPER["variance"], lengthscale=HYPER["lengthscale"], noise_var=HYPER["noise_var"],
              diag_add=HYPER["noise_var"] + 1e-8)
    mean_t0, _, _ = truth_predict(X, y, Xs, data["mX"], data["vX"], data["mXs"], data["vXs"], **tk)
    Xa = np.vstack([X, Xs[picks]])
    ya = np.vstack([y, mean_t0[picks]])
    mXa = vXa = None
    if causal:
        mXa = np.vstack([data["mX"], data["mXs"][picks]])
        vXa = np.vstack([data["vX"], data["vXs"][picks]])
    mean_t, var_t, _ = truth_predict(Xa, ya, Xs, mXa, vXa, data["mXs"], data["vXs"], **tk)
    post = O.fit(Xa, ya, mXa, vXa, **HYPER)
    mean_o, var_o = O.predict(post, Xs, data["mXs"], data["vXs"])
    print("var: ", assert_parity(var, var_o, var_t, "variance at the last pick"))
    print("mean:", assert_parity(mean, mean_o, mean_t, "mean at the last pick"))
    grid.close()


def fixture_case(name, y_best=None, dtype="f64", keep=False):
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    f = load_fixture(name)
    ls = f["lengthscale_arg"]
    kw = {}
    if f["mX"] is not None:
        tables = {"m": np.vstack([f["mX"], f["mXs"]]), "v": np.vstack([f["vX"], f["vXs"]])}
        pts = np.vstack([f["X"], f["Xs"]])

        def lookup(which):
            def fn(a):
                a = np.atleast_2d(a)
                rows = [int(np.flatnonzero(np.all(pts == r[None, :], axis=1))[0]) for r in a]
                return tables[which][rows]
            return fn
        kw = dict(mean_function=lookup("m"), variance_adjustment=lookup("v"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        g = HipGaussianProcess(f["X"], f["y"], dtype=dtype, variance=float(f["variance"]), lengthscale=ls,
                               ard=not np.isscalar(ls), noise_var=float(f["noise_var"]), **kw)
    return g, CandidateGrid(f["Xs"], g, keep_solution=keep), f


def truth_acq(f, ref, t, task, cost):
    """EI / cost over the candidates from the long-double posterior of the data the restatement's pick t was fitted on."""
    X, y, mX, vX = ref["data"][t]
    mean_t, var_t, _ = truth_predict(X, y, f["Xs"], mX, vX, f["mXs"], f["vXs"], variance=float(f["variance"]),
                                     lengthscale=f["lengthscale_arg"], noise_var=float(f["noise_var"]),
                                     diag_add=float(f["noise_var"]) + 1e-8)
    return O.expected_improvement(mean_t, var_t, ref["y_best"][t], task) / cost


def truth_var(f, ref, t):
    X, y, mX, vX = ref["data"][t]
    return truth_predict(X, y, f["Xs"], mX, vX, f["mXs"], f["vXs"], variance=float(f["variance"]),
                         lengthscale=f["lengthscale_arg"], noise_var=float(f["noise_var"]),
                         diag_add=float(f["noise_var"]) + 1e-8)[1]


def check_values(f, ref, vals, task, cost):
    """best_vals[t] under the parity rule, every pick against the long-double acquisition of its own data."""
    for t in range(len(vals)):
        p = int(ref["idx"][t])
        assert_parity(vals[t], ref["val"][t], truth_acq(f, ref, t, task, cost)[p, 0], f"best_vals[{t}]")


@pytest.mark.parametrize("name", ["causal_d2", "graph_ard_d4", "complete_bo_d3"])
def test_the_picks_are_the_restatements(lib, name):
    B = 5
    g, grid, f = fixture_case(name)
    ref = believer(f, B)
    assert np.all(ref["gap"] > 1e-6), ref["gap"]                   # no near-tie decides a pick of the restatement
    assert len(set(ref["idx"].tolist())) == B
    rc, vals, idxs, acq, mean, var = batch(lib, g, grid, float(f["y_best"]), f["task"], B, cost=float(f["cost"]))
    assert rc == 0
    print(name, "device", idxs, vals, "restatement", ref["idx"], ref["val"])
    assert np.array_equal(idxs, ref["idx"])
    assert len(set(idxs.tolist())) == B and np.all(vals > 0)       # no index twice while the acquisition is positive
    check_values(f, ref, vals, f["task"], float(f["cost"]))
    assert_parity(var, ref["var"], truth_var(f, ref, B - 1), "var_out at the last pick")
    grid.close()


@pytest.mark.parametrize("name,shift", [("causal_d2", 0.5), ("graph_ard_d4", 1.0)])
def test_update_incumbent_moves_y_best_on_the_device(lib, name, shift):
    B = 5
    g, grid, f = fixture_case(name)
    first = believer(f, 1, task="min")
    y_best = float(first["mean"][first["idx"][0], 0]) + shift
    fixed = believer(f, B, y_best=y_best, task="min")
    moved = believer(f, B, y_best=y_best, task="min", update_incumbent=True)
    assert np.all(fixed["gap"] > 1e-6) and np.all(moved["gap"] > 1e-6)
    assert moved["y_best"][1] < y_best                             # the incumbent does move
    assert not np.array_equal(fixed["idx"], moved["idx"])
    cost = float(f["cost"])
    rc, vals_m, idxs_m, *_ = batch(lib, g, grid, y_best, "min", B, cost=cost, update=1)
    assert rc == 0
    rc, vals_f, idxs_f, *_ = batch(lib, g, grid, y_best, "min", B, cost=cost, update=0)
    assert rc == 0
    print(name, "moved", idxs_m, moved["idx"], "fixed", idxs_f, fixed["idx"])
    assert np.array_equal(idxs_m, moved["idx"])
    assert np.array_equal(idxs_f, fixed["idx"])
    assert not np.array_equal(idxs_m, idxs_f)
    check_values(f, moved, vals_m, "min", cost)
    check_values(f, fixed, vals_f, "min", cost)
    grid.close()


def test_update_incumbent_for_the_max_task(lib):
    """y_best <- max(y_best, mean_p): with an incumbent BELOW the first pick's mean the second pick's value is the plain
    sweep's at the moved incumbent on the believed model -- checked through the restatement's picks."""
    g, grid, f = fixture_case("graph_ard_d4")
    first = believer(f, 1, task="max", y_best=0.0)
    y_best = float(first["mean"][first["idx"][0], 0]) - 1.0
    moved = believer(f, 3, y_best=y_best, task="max", update_incumbent=True)
    assert np.all(moved["gap"] > 1e-6)
    rc, vals, idxs, *_ = batch(lib, g, grid, y_best, "max", 3, cost=float(f["cost"]), update=1)
    assert rc == 0
    assert np.array_equal(idxs, moved["idx"])
    check_values(f, moved, vals, "max", float(f["cost"]))
    grid.close()


def test_an_fp32_model_answers_from_the_fp64_factor(lib):
    g64, grid64, data = make_case(300, 257, 3, True)
    g32, grid32, _ = make_case(300, 257, 3, True, dtype="f32")
    y_best = float(data["y"].min())
    for B in (1, 5):
        rc, v64, i64, a64, m64, s64 = batch(lib, g64, grid64, y_best, "min", B)
        assert rc == 0
        rc, v32, i32, a32, m32, s32 = batch(lib, g32, grid32, y_best, "min", B)
        assert rc == 0
        assert np.array_equal(i64, i32)
        assert same_bits(s64, s32) and same_bits(m64, m32) and same_bits(v64, v32)
    # ... and the fp32 sweep of the same pair is what it was (its cache is not the batch's)
    before = plain(lib, g32, grid32, y_best, "min")
    batch(lib, g32, grid32, y_best, "min", 5)
    after = plain(lib, g32, grid32, y_best, "min")
    for x, z in zip(before, after):
        assert same_bits(x, z)
    grid64.close(); grid32.close()


def test_errors(lib):
    g, grid, data = make_case(37, 5, 1, False)
    ok = dict(y_best=0.0, task="min", B=2)
    assert batch(lib, g, grid, **ok)[0] == 0
    for B in (0, -1, 65, 6):                                       # outside 1..CBO_MAX_BATCH, above m
        assert batch(lib, g, grid, 0.0, "min", B)[0] == INVALID
    assert batch(lib, g, grid, 0.0, "min", 2, vals=False)[0] == INVALID
    assert batch(lib, g, grid, 0.0, "min", 2, idxs=False)[0] == INVALID
    for cost in (0.0, -1.0, float("nan")):
        assert batch(lib, g, grid, 0.0, "min", 2, cost=cost)[0] == INVALID
    for update in (2, -1):
        assert batch(lib, g, grid, 0.0, "min", 2, update=update)[0] == INVALID
    assert batch(lib, g, grid, 0.0, 2, 2)[0] == INVALID            # check_sweep_args: the task
    gc, gridc, _ = make_case(37, 5, 1, True)
    assert batch(lib, gc, grid, 0.0, "min", 2)[0] == INVALID       # a causal model, candidates without priors
    g3, grid3, _ = make_case(37, 5, 3, False)
    assert batch(lib, g, grid3, 0.0, "min", 2)[0] == INVALID       # dimensions differ
    assert b"dimension" in lib.load().cbo_last_error()
    gu, gridu, _ = make_case(200, 5, 1, False, fit=False)          # (beyond the one-launch small-model path)
    assert batch(lib, gu, gridu, 0.0, "min", 2)[0] == NOT_FITTED
    for k in (grid, gridc, grid3, gridu):
        k.close()


def test_unsupported_when_the_workspace_cannot_hold_every_column(lib):
    out = run_child("import test_batch_gpu as t\nfrom cbo_with_oop_amd import _lib\n"
                    "g, grid, data = t.make_case(300, 1000, 3, False)\n"
                    "rc2 = t.batch(_lib, g, grid, 0.0, 'min', 2)[0]\n"
                    "msg = _lib.load().cbo_last_error().decode()\n"
                    "rc1 = t.batch(_lib, g, grid, 0.0, 'min', 1)[0]\n"
                    "print('rc', rc2, rc1, msg)\n", CBO_HIP_WORKSPACE_MB="1")
    assert f"rc {UNSUPPORTED} 0" in out and "CBO_HIP_WORKSPACE_MB" in out


def test_python_layer_returns_the_points_of_the_c_call(lib):
    from cbo_with_oop_amd import CausalExpectedImprovement, find_next_y_point
    from cbo_with_oop_amd.utils_functions import CausalGradientAcquisitionOptimizer, Cost, GreedyBatchPointCalculator
    g, grid, data = make_case(129, 63, 1, False)
    y_best = float(data["y"].min())
    space = [(-2.5, 2.5)]
    costs = {"X": lambda col: 2.0}
    opt = CausalGradientAcquisitionOptimizer(space, grid_shape=[257])
    pts = opt.candidates()
    from cbo_with_oop_amd import CandidateGrid
    k = CandidateGrid(pts, g)
    rc, vals, idxs, *_ = batch(lib, g, k, y_best, "min", 3, cost=2.0)
    assert rc == 0
    acquisition = CausalExpectedImprovement(y_best, "min", g) / Cost(costs, ["X"])
    calc = GreedyBatchPointCalculator(g, acquisition, opt, 3)
    x = calc.compute_next_points()
    assert x.shape == (3, 1) and np.array_equal(x, pts[idxs])
    assert same_bits(calc.last_result["best_val"], vals)
    y3, x3 = find_next_y_point(space, g, y_best, ["X"], costs, grid_shape=[257], batch_size=3)
    assert y3.shape == (3, 1) and x3.shape == (3, 1)
    assert np.array_equal(x3, pts[idxs]) and same_bits(y3[:, 0], vals)
    # batch_size=None: the single-point path, unchanged
    y1, x1 = find_next_y_point(space, g, y_best, ["X"], costs, grid_shape=[257])
    res = CausalExpectedImprovement(y_best, "min", g).sweep(k, cost=2.0)
    assert y1.shape == (1, 1) and x1.shape == (1, 1)
    assert same_bits(y1[0, 0], res["best_val"]) and np.array_equal(x1[0], pts[res["best_idx"]])
    assert same_bits(y3[0, 0], y1[0, 0]) and np.array_equal(x3[0], x1[0])
    # variable costs: y[t] over the point's own cost
    var_costs = {"X": lambda col: 1.0 + np.sum(np.abs(col))}
    yv, xv = find_next_y_point(space, g, y_best, ["X"], var_costs, grid_shape=[257], batch_size=3)
    y1v, x1v = find_next_y_point(space, g, y_best, ["X"], var_costs, grid_shape=[257])
    assert np.array_equal(xv, pts[idxs]) and same_bits(yv[0, 0], y1v[0, 0])
    batch_cost = 1.0 + np.sum(np.abs(pts))
    for t in (1, 2):
        assert np.isclose(yv[t, 0], vals[t] * 2.0 / (1.0 + abs(xv[t, 0])), rtol=1e-12)
    k.close(); grid.close()
