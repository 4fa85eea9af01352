"""GPU tests of the block append (cbo_gp_append_block: the kernels of kernels_append.hip; contract in include/cbo_hip.h and
DESIGN.md 4h).

Every comparison is against a fresh ``HipGaussianProcess`` on the grown data, at the tolerances of
``test_append_only_trial_step_matches_full_refit`` (tests/test_parity_gpu.py): mean 1e-9 / 1e-11, variance 1e-8 / 1e-13,
acquisition rtol 1e-6 where above 1e-6 of its maximum, the same winner, L 1e-10 / 1e-13, alpha 1e-7 / 1e-9,
log-likelihood rel 1e-10.  1500 candidates: no multiple of 64 or 256.  Shapes (n0, k, d) are the smallest that reach each
code path: 44 + 7 crosses the 16-row tile at 48 inside one panel; 120 + 8 fills the padding exactly; 130 + 64 is the
largest block, touches five tiles and needs a two-block forward solve; 1100 + 17 has k no multiple of 4 or 16 and nine
row blocks; 300 + 9 is causal.
"""
import ctypes
import warnings

import numpy as np
import pytest

from accuracy_support import check_alpha, check_factor, lapack_factor, sample_rows

pytestmark = pytest.mark.gpu

M = 1500


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def _f(a):
    return np.sin(a[:, :1]) + 0.3 * np.cos(2 * a[:, -1:])


def _mean_fn(a):
    return 0.1 * a[:, :1]


def _var_adj(a):
    return 0.2 + 0.1 * np.cos(a[:, 1:2]) ** 2


def _kw(causal=False, **more):
    kw = dict(noise_var=1e-2, lengthscale=0.9)
    if causal:
        kw.update(mean_function=_mean_fn, variance_adjustment=_var_adj)
    kw.update(more)
    return kw


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n, d))
    y = _f(X) + 0.05 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2, 2, (M, d))
    return X, y, Xs


def _model(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def _sweep(model, cands, best):
    from cbo_with_oop_amd import CausalExpectedImprovement
    return CausalExpectedImprovement(best, "min", model).sweep(cands, cost=2.0, want_acq=True, want_posterior=True)


def _grid(Xs, model, keep=True):
    from cbo_with_oop_amd import CandidateGrid
    return CandidateGrid(Xs, model, keep_solution=keep)


def _assert_sweeps_agree(a, b):
    np.testing.assert_allclose(a["mean"], b["mean"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(a["var"], b["var"], rtol=1e-8, atol=1e-13)
    big = b["acq"][:, 0] > 1e-6 * b["acq"].max()
    np.testing.assert_allclose(a["acq"][big], b["acq"][big], rtol=1e-6)
    assert a["best_idx"] == b["best_idx"]


def _assert_models_agree(inc, ref):
    La, alpha_a = inc.posterior_state()
    Lb, alpha_b = ref.posterior_state()
    np.testing.assert_allclose(La, Lb, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(alpha_a, alpha_b, rtol=1e-7, atol=1e-9)
    assert inc.log_likelihood() == pytest.approx(ref.log_likelihood(), rel=1e-10)


def _same_bits(a, b, keys=("mean", "var", "acq")):
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["best_idx"] == b["best_idx"] and a["best_val"] == b["best_val"]


SHAPES = [(44, 7, 1, False), (120, 8, 2, False), (130, 64, 2, False), (1100, 17, 3, False), (300, 9, 2, True)]


@pytest.mark.parametrize("n0,k,d,causal", SHAPES)
def test_block_append_matches_full_refit(hip, n0, k, d, causal):
    """One block onto a swept model with a kept solution: the factor, alpha, the likelihood and the sweep that extends the
    resident V by k rows agree with a fresh model on the grown data; so does a grid without a kept solution."""
    X, y, Xs = _data(n0 + k, d, seed=n0 + k)
    kw = _kw(causal)
    inc = _model(X[:n0], y[:n0], **kw)
    grid, plain = _grid(Xs, inc), _grid(Xs, inc, keep=False)
    _sweep(inc, grid, float(y[:n0].min()))
    _sweep(inc, plain, float(y[:n0].min()))
    assert inc.append_block(X[n0:], y[n0:])
    assert np.array_equal(inc.X, X) and np.array_equal(inc.Y, y)
    best = float(y.min())
    ref = _model(X, y, **kw)
    b = _sweep(ref, Xs, best)
    _assert_sweeps_agree(_sweep(inc, grid, best), b)
    _assert_sweeps_agree(_sweep(inc, plain, best), b)
    _assert_models_agree(inc, ref)
    # a full refit of the grown model reproduces the reference (the resident data are complete)
    inc.set_data(X, y)
    c = _sweep(inc, grid, best)
    big = b["acq"][:, 0] > 1e-6 * b["acq"].max()
    np.testing.assert_allclose(c["acq"][big], b["acq"][big], rtol=1e-9)
    for m in (inc, ref):
        m.close()


@pytest.mark.parametrize("n0,k,d", [(130, 64, 2), (1100, 17, 3)])
def test_block_append_backward_error(hip, n0, k, d):
    """check_factor and check_alpha (<= 8 x LAPACK) on the device-assembled Ky of the grown data, the rows of the block in
    the sample."""
    X, y, _ = _data(n0 + k, d, seed=n0)
    m = _model(X[:n0], y[:n0], noise_var=1e-4)
    assert m.append_block(X[n0:], y[n0:])
    n = n0 + k
    L, alpha = m.posterior_state()
    Ky = m.assembled_Ky()
    rows = np.union1d(sample_rows(n, np.random.default_rng(n0)), np.arange(n0, n))
    L_ref = lapack_factor(Ky)
    f = check_factor(L, Ky, rows, L_ref)
    a = check_alpha(alpha, Ky, y[:n, 0], L_ref)
    print(f"\nMEASURED block {n0}+{k}: factor ratio {f['ratio']:.2f}, alpha ratio {a['ratio']:.2f}")
    assert f["ok"], f
    assert a["ok"], a
    m.close()


@pytest.mark.parametrize("case", ["padding", "f32", "ladder"])
def test_declines_leave_everything_untouched(hip, case):
    """append_block returns False and the next sweep returns the bits it returned before."""
    X, y, Xs = _data(121 + 8, 2, seed=3)
    n0, kw = 121, _kw()
    if case == "f32":
        n0, kw = 100, _kw(dtype="f32")
    if case == "ladder":
        # duplicated rows under a negative noise variance: level 0 of the jitchol ladder fails (tests/test_accuracy_gpu.py)
        n0, kw = 100, dict(noise_var=-1.1e-8)
        X[n0 - n0 // 8:n0] = X[:n0 // 8]
    m = _model(X[:n0], y[:n0], **kw)
    if case == "ladder":
        assert m.jitter_tries >= 1
    grid = _grid(Xs, m, keep=case != "f32")
    best = float(y[:n0].min())
    before = _sweep(m, grid, best)
    state = m.posterior_state()
    assert m.append_block(X[n0:n0 + 8], y[n0:n0 + 8]) is False
    assert m.X.shape[0] == n0 and m.Y.shape[0] == n0
    after = _sweep(m, grid, best)
    assert _same_bits(before, after)
    again = m.posterior_state()
    assert np.array_equal(state[0], again[0]) and np.array_equal(state[1], again[1])
    m.close()


def test_block_of_one_is_the_single_append(hip):
    """k = 1 delegates to cbo_gp_append: the same bits as ``append`` on a twin model, factor and sweep."""
    X, y, Xs = _data(201, 2, seed=9)
    a, b = _model(X[:200], y[:200], **_kw()), _model(X[:200], y[:200], **_kw())
    ga, gb = _grid(Xs, a), _grid(Xs, b)
    best = float(y.min())
    _sweep(a, ga, best); _sweep(b, gb, best)
    assert a.append_block(X[200:], y[200:]) and b.append(X[200], y[200])
    assert _same_bits(_sweep(a, ga, best), _sweep(b, gb, best))
    sa, sb = a.posterior_state(), b.posterior_state()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    a.close(); b.close()


def _run_sequence(X, y, Xs, n0, steps, kw):
    """steps: ('block', k), ('one',) or ('sweep',); returns the model, the sweeps and the rows consumed."""
    m = _model(X[:n0], y[:n0], **kw)
    grid = _grid(Xs, m)
    out = [_sweep(m, grid, float(y[:n0].min()))]
    n = n0
    for s in steps:
        if s[0] == "block":
            assert m.append_block(X[n:n + s[1]], y[n:n + s[1]])
            n += s[1]
        elif s[0] == "one":
            assert m.append(X[n], y[n])
            n += 1
        else:
            out.append(_sweep(m, grid, float(y[:n].min())))
    return m, out, n


SEQUENCES = {
    "block_sweep_block_sweep": [("block", 20), ("sweep",), ("block", 5), ("sweep",)],
    "block_block_sweep": [("block", 20), ("block", 5), ("sweep",)],
    "block_one_sweep": [("block", 20), ("one",), ("sweep",)],
    "one_block_sweep": [("one",), ("block", 20), ("sweep",)],
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_sequences_match_full_refit(hip, name):
    """The kept V extended twice; a V older than the parent (substitution); blocks mixed with single appends."""
    n0 = 150
    X, y, Xs = _data(n0 + 30, 2, seed=21)
    m, out, n = _run_sequence(X, y, Xs, n0, SEQUENCES[name], _kw())
    ref = _model(X[:n], y[:n], **_kw())
    _assert_sweeps_agree(out[-1], _sweep(ref, Xs, float(y[:n].min())))
    _assert_models_agree(m, ref)
    m.close(); ref.close()


def test_kept_solution_gains_rows_without_a_substitution(hip):
    """Which path a sweep takes, by the substitution's launch counter: none after one block on a swept set with a kept
    solution; the substitution when the V is older than the parent (two blocks, no sweep between) and for a set that
    keeps no solution."""
    from cbo_with_oop_amd import _lib
    n0 = 150
    X, y, Xs = _data(n0 + 30, 2, seed=23)
    ctx = _lib.Context.get()
    m = _model(X[:n0], y[:n0], **_kw())
    kept, plain = _grid(Xs, m), _grid(Xs, m, keep=False)
    best = float(y.min())

    def launches(grid):
        ctx.set_profiling(True); ctx.reset_timers()
        try:
            _sweep(m, grid, best)
            return ctx.timers()["n_trsm_launches"]
        finally:
            ctx.set_profiling(False)

    _sweep(m, kept, best); _sweep(m, plain, best)
    assert m.append_block(X[n0:n0 + 20], y[n0:n0 + 20])
    assert launches(kept) == 0
    assert launches(plain) >= 1
    assert m.append_block(X[n0 + 20:n0 + 25], y[n0 + 20:n0 + 25])
    assert m.append_block(X[n0 + 25:n0 + 30], y[n0 + 25:n0 + 30])
    assert launches(kept) >= 1
    m.close()


def test_same_sequence_same_bits(hip):
    """Two models taken through the same calls: identical bits of L, alpha and every sweep output."""
    n0 = 150
    X, y, Xs = _data(n0 + 30, 2, seed=22)
    steps = SEQUENCES["block_sweep_block_sweep"]
    a, oa, _ = _run_sequence(X, y, Xs, n0, steps, _kw())
    b, ob, _ = _run_sequence(X, y, Xs, n0, steps, _kw())
    for ra, rb in zip(oa, ob):
        assert _same_bits(ra, rb)
    sa, sb = a.posterior_state(), b.posterior_state()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    a.close(); b.close()


def test_other_consumers_see_the_grown_model(hip):
    """predict, the likelihood gradients, the full covariance of 40 points and a batch of 3 after a block append, against
    the refit model at the tolerances of their own tests' comparisons between two device paths."""
    from cbo_with_oop_amd import CausalExpectedImprovement
    n0, k = 300, 12
    X, y, Xs = _data(n0 + k, 2, seed=31)
    inc = _model(X[:n0], y[:n0], **_kw())
    grid = _grid(Xs, inc)
    _sweep(inc, grid, float(y[:n0].min()))
    assert inc.append_block(X[n0:], y[n0:])
    ref = _model(X, y, **_kw())
    mean_a, var_a = inc.predict(Xs[:200])
    mean_b, var_b = ref.predict(Xs[:200])
    np.testing.assert_allclose(mean_a, mean_b, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(var_a, var_b, rtol=1e-8, atol=1e-13)
    for ga, gb in zip(inc.log_likelihood_gradients(), ref.log_likelihood_gradients()):
        np.testing.assert_allclose(ga, gb, rtol=1e-7, atol=1e-9)
    _, cov_a = inc.predict(Xs[:40], full_cov=True)
    _, cov_b = ref.predict(Xs[:40], full_cov=True)
    np.testing.assert_allclose(cov_a, cov_b, rtol=1e-8, atol=1e-12)
    best = float(y.min())
    ba = CausalExpectedImprovement(best, "min", inc).sweep_batch(grid, 3, cost=2.0)
    bb = CausalExpectedImprovement(best, "min", ref).sweep_batch(Xs, 3, cost=2.0)
    assert np.array_equal(ba["best_idx"], bb["best_idx"])
    np.testing.assert_allclose(ba["best_val"], bb["best_val"], rtol=1e-6)
    inc.close(); ref.close()


def test_argument_errors(hip):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    X, y, _ = _data(60, 2, seed=41)
    done = ctypes.c_int(7)
    xn, yn = np.ascontiguousarray(X[50:]), np.ascontiguousarray(y[50:, 0])
    plain = _model(X[:50], y[:50], **_kw())
    call = lambda h, k, x, yy, pm, pv, out: lib.cbo_gp_append_block(h, k, _lib.dptr(x), _lib.dptr(yy), _lib.dptr(pm),
                                                                    _lib.dptr(pv), out)
    for k in (0, -1, 65):
        assert call(plain._handle, k, xn, yn, None, None, ctypes.byref(done)) == _lib.CBO_ERR_INVALID
    assert call(plain._handle, 10, None, yn, None, None, ctypes.byref(done)) == _lib.CBO_ERR_INVALID
    assert call(plain._handle, 10, xn, None, None, None, ctypes.byref(done)) == _lib.CBO_ERR_INVALID
    assert call(plain._handle, 10, xn, yn, None, None, None) == _lib.CBO_ERR_INVALID
    assert call(None, 10, xn, yn, None, None, ctypes.byref(done)) == _lib.CBO_ERR_INVALID
    causal = _model(X[:50], y[:50], **_kw(True))
    pv = np.full(10, 0.2)
    assert call(causal._handle, 10, xn, yn, None, None, ctypes.byref(done)) == _lib.CBO_ERR_INVALID
    assert call(causal._handle, 10, xn, yn, pv, None, ctypes.byref(done)) == _lib.CBO_ERR_INVALID
    unfitted = _model(X[:50], y[:50], fit=False, **_kw())
    assert call(unfitted._handle, 10, xn, yn, None, None, ctypes.byref(done)) == _lib.CBO_ERR_NOT_FITTED
    assert unfitted.append_block(xn, yn) is False                   # the wrapper declines a stale model, as ``append``
    # none of the rejected calls changed a model
    assert plain.X.shape[0] == 50 and int(lib.cbo_gp_n(plain._handle)) == 50 and int(lib.cbo_gp_n(causal._handle)) == 50
    for m in (plain, causal, unfitted):
        m.close()
