"""GPU tests of leave-one-out cross-validation on the device (cbo_gp_loo, cbo_gp_loo_batch: kernels_loo.hip; contract in
include/cbo_hip.h and DESIGN.md 4i).

The reference is loo_support.closed_form on the oracle's kernel matrix.  Tolerances are ten times the gap between that
closed form and n brute-force refits on the same data (tests/test_loo_host.py: G_FIXTURE per golden fixture, G_SYNTHETIC
per size of the synthetic data), at least 1e-12, measured as loo_support.gap measures it: mean relative to the scale of
|y|, variance relative, lpd absolute.  The first rows of a fixture take the fixture's tolerance: Ky of a subset is a
principal submatrix of the fixture's, so by Cauchy interlacing its condition number is no larger, and neither is the
rounding error of either form.

Sizes of the general path (rows are padded to 128; the pair kernel takes 256-row blocks, the strip kernel 128): 129 (the
second block holds one row), 300 (384 padded rows: no multiple of 256, the strip kernel), 515 (640: a partial third block of
a pair), 700 in a child process whose workspace holds 128 columns (six chunks of the identity, trailing systems at rows 0,
0, 256, 256, 512, 512), 1100 (1152 padded rows: from 1024 on the right-looking schedule), and 100 and 128, which reach the
general path only when fitted and called through cbo_gp_loo."""
import ctypes
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import loo_support as S
from conftest import ROOT, load_fixture
from test_loo_host import G_FIXTURE, G_SYNTHETIC, gpu_tolerance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def _model(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def _synthetic_model(n, **kw):
    X, y = S.synthetic(n)
    return _model(X, y, noise_var=S.SYNTHETIC_NOISE, **kw), X, y


def _synthetic_reference(X, y):
    Ky, r, yy = S.ky_and_residual(X, y, noise_var=S.SYNTHETIC_NOISE)
    return S.closed_form(Ky, r, yy), yy


def _fixture_model(f, rows, fit):
    ls = f["lengthscale_arg"]
    kw = dict(variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls), noise_var=float(f["noise_var"]), fit=fit)
    if f["mX"] is not None:
        lut_m = {tuple(r): v for r, v in zip(map(tuple, f["X"]), f["mX"][:, 0])}
        lut_v = {tuple(r): v for r, v in zip(map(tuple, f["X"]), f["vX"][:, 0])}
        kw["mean_function"] = lambda a: np.array([[lut_m[tuple(r)]] for r in a])
        kw["variance_adjustment"] = lambda a: np.array([[lut_v[tuple(r)]] for r in a])
    return _model(f["X"][:rows], f["y"][:rows], **kw)


def _loo(lib, model):
    """cbo_gp_loo with all four outputs: ((mean, var, lpd), sum)."""
    n = model.X.shape[0]
    mean, var, lpd = np.zeros(n), np.zeros(n), np.zeros(n)
    total = ctypes.c_double(0.0)
    lib.check(lib.load().cbo_gp_loo(model._handle, lib.dptr(mean), lib.dptr(var), lib.dptr(lpd), ctypes.byref(total)))
    return (mean, var, lpd), total.value


def _loo_batch(lib, models):
    """cbo_gp_loo_batch: (return code, sums, per-model lpd, status)."""
    k = len(models)
    handles = (ctypes.c_void_p * k)(*[m._handle for m in models])
    sums, status = np.zeros(k), np.full(k, 77, dtype=np.int32)
    cat = np.zeros(sum(m.X.shape[0] for m in models))
    rc = lib.load().cbo_gp_loo_batch(k, handles, lib.dptr(sums), lib.dptr(cat), status.ctypes.data_as(lib.c_int_p))
    return rc, sums, np.split(cat, np.cumsum([m.X.shape[0] for m in models])[:-1]), status


def _check(what, got, ref, y, tol):
    g = S.gap(got, ref, y)
    print(f"{what}: gap to the closed form {g:.3e}, tolerance {tol:.3e}")
    assert g <= tol, what


@pytest.mark.parametrize("n", [100, 128, 129, 300, 515, 1100])
def test_general_path_matches_closed_form(lib, n):
    model, X, y = _synthetic_model(n)
    ref, yy = _synthetic_reference(X, y)
    got, total = _loo(lib, model)
    _check(f"n = {n}", got, ref, yy, gpu_tolerance(G_SYNTHETIC[n]))
    assert total == pytest.approx(math.fsum(got[2]), rel=1e-12)
    model.close()


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import loo_support as S
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
X, y = S.synthetic(700)
m = HipGaussianProcess(X, y, noise_var=S.SYNTHETIC_NOISE)
m._ctx.set_profiling(True)
m._ctx.reset_timers()
mean, var, lpd, total = m._loo(True, True, True)
np.savez({out!r}, mean=mean, var=var, lpd=lpd, total=total, launches=m._ctx.timers()["n_trsm_launches"])
"""


def test_general_path_in_chunks_of_a_small_workspace(lib, tmp_path):
    """CBO_HIP_WORKSPACE_MB is read when the context is created: a child process with a 1 MB workspace (128 columns of the
    768 padded rows) solves the identity of n = 700 in six chunks, four of them as trailing systems."""
    out = str(tmp_path / "loo700.npz")
    env = dict(os.environ, CBO_HIP_WORKSPACE_MB="1")
    subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)], env=env,
                   check=True, timeout=300)
    got = np.load(out)
    assert int(got["launches"]) >= 3
    X, y = S.synthetic(700)
    ref, yy = _synthetic_reference(X, y)
    _check("n = 700 in chunks", (got["mean"], got["var"], got["lpd"]), ref, yy, gpu_tolerance(G_SYNTHETIC[700]))
    assert float(got["total"]) == pytest.approx(math.fsum(got["lpd"]), rel=1e-12)
    # one chunk in this process: the same answer within the same tolerance
    model, _, _ = _synthetic_model(700)
    one, _ = _loo(lib, model)
    _check("n = 700 in one chunk", one, ref, yy, gpu_tolerance(G_SYNTHETIC[700]))
    model.close()


@pytest.mark.parametrize("name", S.FIXTURE_NAMES)
def test_fitted_fixtures_through_cbo_gp_loo(lib, name):
    f = load_fixture(name)
    model = _fixture_model(f, None, fit=True)
    Ky, r, y = S.fixture_system(f)
    got, total = _loo(lib, model)
    _check(name, got, S.closed_form(Ky, r, y), y, gpu_tolerance(G_FIXTURE[name]))
    assert total == pytest.approx(math.fsum(got[2]), rel=1e-12)
    model.close()


# (fixture, rows, fitted beforehand): sizes 1, 2, 17, 50, 128 and two whole fixtures on the small path, causal and plain,
# one fitted model of 129 rows in the middle on the general path
MIXED = [("causal_d2", 1, False), ("toy_bo_d2", 2, False), ("graph_ard_d4", 17, False), ("coral_max_d3", 50, False),
         ("graph_ard_d4", 129, True), ("graph_ard_d4", 128, False), ("causal_d2", 40, False), ("toy_bo_d2", 20, False)]


def test_small_path_batch_on_the_fixtures(lib):
    fixtures = {name: load_fixture(name) for name in S.FIXTURE_NAMES}
    models = [_fixture_model(fixtures[name], rows, fit) for name, rows, fit in MIXED]
    rc, sums, lpds, status = _loo_batch(lib, models)
    assert rc == lib.CBO_OK and np.all(status == lib.CBO_OK)
    for (name, rows, fit), model, total, lpd in zip(MIXED, models, sums, lpds):
        Ky, r, y = S.fixture_system(fixtures[name], rows)
        ref = S.closed_form(Ky, r, y)
        tol = gpu_tolerance(G_FIXTURE[name])
        gap = float(np.max(np.abs(lpd - ref[2])))
        print(f"{name}[:{rows}]: lpd gap {gap:.3e}, tolerance {tol:.3e}")
        assert gap <= tol, (name, rows)
        assert total == pytest.approx(math.fsum(lpd), rel=1e-12)
        assert model.stale == (not fit)                      # nothing was fitted on the way
        # a one-model batch returns the bits the model has in the mixed batch
        rc1, sums1, lpds1, status1 = _loo_batch(lib, [model])
        assert rc1 == lib.CBO_OK and status1[0] == lib.CBO_OK
        assert sums1[0] == total and np.array_equal(lpds1[0], lpd), (name, rows)
    # the small path's mean and variance too: a fitted small model through cbo_gp_loo is the general path on the same data
    for (name, rows, fit), model, lpd in zip(MIXED, models, lpds):
        if fit or rows < 17:
            continue
        model.ensure_fitted()
        got, _ = _loo(lib, model)
        Ky, r, y = S.fixture_system(fixtures[name], rows)
        _check(f"{name}[:{rows}] fitted", got, S.closed_form(Ky, r, y), y, gpu_tolerance(G_FIXTURE[name]))
        assert float(np.max(np.abs(got[2] - lpd))) <= 2.0 * gpu_tolerance(G_FIXTURE[name])     # each within one of the reference
    for m in models:
        m.close()


def test_unfitted_large_model_in_a_batch_disturbs_nobody(lib):
    f = load_fixture("graph_ard_d4")
    models = [_fixture_model(f, 50, False), _fixture_model(f, 129, False), _fixture_model(f, 17, False)]
    rc, sums, lpds, status = _loo_batch(lib, models)
    assert rc == lib.CBO_OK
    assert list(status) == [lib.CBO_OK, lib.CBO_ERR_NOT_FITTED, lib.CBO_OK]
    for i in (0, 2):
        _, sums1, lpds1, _ = _loo_batch(lib, [models[i]])
        assert sums1[0] == sums[i] and np.array_equal(lpds1[0], lpds[i])
    for m in models:
        m.close()


def test_a_model_the_batch_launch_declines_takes_the_general_path_between_its_neighbours(lib):
    """The jitter fixture (duplicate rows under a negative noise: the launch's pivot at the duplicate is about -2e-9, far
    below rounding, so it declines there) between two ordinary small models: the batch fits it with the jitchol ladder and
    answers with cbo_gp_loo's bits on a fitted twin; the neighbours stay unfitted and get their one-model batches' bits; the
    same call again and the neighbours alone right after return the same bits."""
    so = lib.load()
    fj, fo = load_fixture("jitter_ladder"), load_fixture("graph_ard_d4")
    ladder, twin = _fixture_model(fj, None, False), _fixture_model(fj, None, True)
    models = [_fixture_model(fo, 17, False), ladder, _fixture_model(fo, 25, False)]
    n = fj["X"].shape[0]
    lpd_twin, total_twin = np.zeros(n), ctypes.c_double(0.0)
    lib.check(so.cbo_gp_loo(twin._handle, None, None, lib.dptr(lpd_twin), ctypes.byref(total_twin)))
    alone = [_loo_batch(lib, [models[i]]) for i in (0, 2)]
    out, tries = np.empty(1), ctypes.c_int(-1)
    for attempt in ("the call", "the same call again"):
        rc, sums, lpds, status = _loo_batch(lib, models)
        print(attempt, "sums", sums.tolist(), "twin", total_twin.value, "status", status.tolist())
        assert rc == lib.CBO_OK and np.all(status == lib.CBO_OK)
        assert sums[1] == total_twin.value and np.array_equal(lpds[1].view(np.uint64), lpd_twin.view(np.uint64))
        for i, (_, sums1, lpds1, _) in zip((0, 2), alone):
            assert sums1[0] == sums[i] and np.array_equal(lpds1[0].view(np.uint64), lpds[i].view(np.uint64)), (attempt, i)
        assert so.cbo_gp_log_marginal(ladder._handle, lib.dptr(out)) == lib.CBO_OK         # the general path fitted it ...
        assert so.cbo_gp_jitter(ladder._handle, ctypes.byref(tries), None) == lib.CBO_OK and tries.value >= 1   # ... by the ladder
        for i in (0, 2):
            assert so.cbo_gp_log_marginal(models[i]._handle, lib.dptr(out)) == lib.CBO_ERR_NOT_FITTED
    rc, sums, lpds, status = _loo_batch(lib, models[::2])
    assert rc == lib.CBO_OK and np.all(status == lib.CBO_OK)
    for j, (_, sums1, lpds1, _) in enumerate(alone):
        assert sums1[0] == sums[j] and np.array_equal(lpds1[0].view(np.uint64), lpds[j].view(np.uint64)), j
    assert twin.jitter_tries >= 1                                                          # the premise: the fixture needs it
    for m in models + [twin]:
        m.close()


def test_end_to_end_against_models_fitted_without_the_point(lib):
    """Independent of the restatement: the device's own prediction of y_i from a model fitted on the other 299 points.
    cbo_gp_predict adds the noise to its variance but not the 1e-8 GPy adds to the diagonal of Ky, which the LOO variance --
    a predictive variance of the observation under Ky -- contains: it is added here."""
    n = 300
    model, X, y = _synthetic_model(n)
    mean, var = model.loo_predict()
    assert mean.shape == (n, 1) and var.shape == (n, 1)
    tol = gpu_tolerance(G_SYNTHETIC[n])
    scale = float(np.max(np.abs(y)))
    for i in (0, 130, n - 1):
        keep = np.arange(n) != i
        rest = _model(X[keep], y[keep], noise_var=S.SYNTHETIC_NOISE)
        m_i, v_i = rest.predict(X[i:i + 1])
        v_i = v_i[0, 0] + 1e-8
        print(f"i = {i}: mean gap {abs(mean[i, 0] - m_i[0, 0]) / scale:.3e}, var gap {abs(var[i, 0] - v_i) / v_i:.3e}, "
              f"tolerance {tol:.3e}")
        assert abs(mean[i, 0] - m_i[0, 0]) / scale <= tol
        assert abs(var[i, 0] - v_i) / v_i <= tol
        rest.close()
    model.close()


@pytest.mark.parametrize("n0,k", [(190, 10), (199, 1)])
def test_after_growth(lib, n0, k):
    X, y = S.synthetic(200)
    grown = _model(X[:n0], y[:n0], noise_var=S.SYNTHETIC_NOISE)
    if k == 1:
        assert grown.append(X[n0:], y[n0:])
    else:
        assert grown.append_block(X[n0:], y[n0:])
    fresh = _model(X, y, noise_var=S.SYNTHETIC_NOISE)
    a, total_a = _loo(lib, grown)
    b, total_b = _loo(lib, fresh)
    ref, yy = _synthetic_reference(X, y)
    tol = gpu_tolerance(G_SYNTHETIC[200])
    _check(f"{n0} + {k} against a fit on 200", a, b, yy, tol)
    _check(f"{n0} + {k} against the closed form", a, ref, yy, tol)
    assert total_a == pytest.approx(total_b, abs=200 * tol)
    grown.close()
    fresh.close()


def test_read_only_and_repeatable(lib):
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    rng = np.random.default_rng(5)
    big, _, yb = _synthetic_model(300)
    small, _, ys = _synthetic_model(50)
    Xs = rng.uniform(-3, 3, (1500, 2))
    sweeps = []
    for model, y in ((big, yb), (small, ys)):
        grid, plain = CandidateGrid(Xs, model, keep_solution=True), CandidateGrid(Xs, model)
        acq = CausalExpectedImprovement(float(y.min()), "min", model)
        sweeps.append((acq, grid, plain, acq.sweep(grid, cost=2.0, want_acq=True, want_posterior=True),
                       acq.sweep(plain, cost=2.0, want_acq=True, want_posterior=True)))
    first, total1 = _loo(lib, big)
    second, total2 = _loo(lib, big)
    assert all(np.array_equal(a, b) for a, b in zip(first, second)) and total1 == total2
    assert total1 == pytest.approx(math.fsum(first[2]), rel=1e-12)
    rc, sums, lpds, status = _loo_batch(lib, [small, big])
    assert rc == lib.CBO_OK and np.all(status == lib.CBO_OK)
    assert sums[1] == total1 and np.array_equal(lpds[1], first[2])
    for acq, grid, plain, before_kept, before_plain in sweeps:
        for cands, before in ((grid, before_kept), (plain, before_plain)):
            after = acq.sweep(cands, cost=2.0, want_acq=True, want_posterior=True)
            assert all(np.array_equal(after[k], before[k]) for k in ("mean", "var", "acq"))
            assert after["best_idx"] == before["best_idx"] and after["best_val"] == before["best_val"]
    assert not big.stale and not small.stale
    big.close()
    small.close()


def test_fp32_model_answers_from_the_fp64_factor(lib):
    a, _, _ = _synthetic_model(300)
    b, _, _ = _synthetic_model(300, dtype="f32")
    ra, ta = _loo(lib, a)
    rb, tb = _loo(lib, b)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and ta == tb
    a.close()
    b.close()


def test_errors(lib):
    so = lib.load()
    unfitted, _, _ = _synthetic_model(40, fit=False)
    fitted, _, _ = _synthetic_model(40)
    out, total = np.zeros(40), ctypes.c_double(0.0)
    assert so.cbo_gp_loo(unfitted._handle, lib.dptr(out), None, None, None) == lib.CBO_ERR_NOT_FITTED
    assert so.cbo_gp_loo(fitted._handle, None, None, None, None) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo(None, lib.dptr(out), None, None, ctypes.byref(total)) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo(fitted._handle, None, None, None, ctypes.byref(total)) == lib.CBO_OK          # any one output will do
    handles = (ctypes.c_void_p * 1)(fitted._handle)
    sums, status = np.zeros(1), np.zeros(1, dtype=np.int32)
    st = status.ctypes.data_as(lib.c_int_p)
    assert so.cbo_gp_loo_batch(0, handles, lib.dptr(sums), None, st) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo_batch(-1, handles, lib.dptr(sums), None, st) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo_batch(1, None, lib.dptr(sums), None, st) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo_batch(1, handles, None, None, st) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo_batch(1, handles, lib.dptr(sums), None, None) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo_batch(1, (ctypes.c_void_p * 1)(None), lib.dptr(sums), None, st) == lib.CBO_ERR_INVALID
    assert so.cbo_gp_loo_batch(1, handles, lib.dptr(sums), None, st) == lib.CBO_OK and status[0] == lib.CBO_OK
    # (lpd_cat may be NULL.)  The small path and the general one are two routes to the same sum
    assert sums[0] == pytest.approx(total.value, abs=40 * gpu_tolerance(G_SYNTHETIC[100]))
    unfitted.close()
    fitted.close()


def test_python_surface(lib):
    from cbo_with_oop_amd import GaussianProcessFactory, GaussianProcessType
    from cbo_with_oop_amd.utils_functions.model_check import loo_scores, prefer_causal_prior
    rng = np.random.default_rng(11)
    # (the factory's noise is 1e-10: points a lengthscale apart keep Ky well conditioned)
    xs = [np.linspace(-5.0, 6.0, 12)[:, None], np.linspace(-5.0, 19.0, 16)[:, None]]
    ys = [np.sin(x) + 0.1 * rng.standard_normal(x.shape) for x in xs]
    # set 0: a prior mean that is the truth; set 1: one that is badly wrong
    priors = [(lambda a: np.sin(a[:, :1]), lambda a: 0.1 + 0.0 * a[:, :1]),
              (lambda a: 5.0 + 3.0 * np.cos(3.0 * a[:, :1]), lambda a: 0.1 + 0.0 * a[:, :1])]
    causal = [GaussianProcessFactory.create(GaussianProcessType.CAUSAL_GP, x, y, p, emukit_wrapper=True)
              for x, y, p in zip(xs, ys, priors)]
    plain = [GaussianProcessFactory.create(GaussianProcessType.NON_CAUSAL_GP, x, y, None, emukit_wrapper=True)
             for x, y in zip(xs, ys)]
    for m in causal + plain:
        lpd = m.loo()
        assert lpd.shape == (m.X.shape[0], 1)
        mean, var = m.loo_predict()
        assert mean.shape == lpd.shape and var.shape == lpd.shape and np.all(var > 0)
        assert m.loo_score() == pytest.approx(math.fsum(lpd[:, 0]), rel=1e-12)
    expected = [c.loo_score() > p.loo_score() for c, p in zip(causal, plain)]
    assert prefer_causal_prior(causal, plain) == expected
    scores = loo_scores(causal + plain)
    for s, m in zip(scores, causal + plain):
        assert s == pytest.approx(m.loo_score(), abs=1e-6 * max(1.0, abs(s)))
    for m in causal + plain:
        m.close()
