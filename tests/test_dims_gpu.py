"""GPU tests of the dimension-specialised kernels (kmat_tile_kernel<D, OUT32>, cov_tile_kernel<D, SYM>, ivr_tile_kernel<D>,
batch_final_kernel<D>, lml_grad_tile_kernel<D>, small_lml_kernel<D>, mid_lml_body<D>, small_assemble<D>, small_kstar<D>,
small_batch_picks<D>, the append kernels' K(Xb, X*)) and of the kernels that loop to a run-time d (pred_gradients_kernel, the
hyper-marginalised sweep, prep_points*), at every input dimension 3..8.

Part one, without a tolerance.  A problem with two live coordinates is zero-extended into D columns (tests/dims_support.py:
19 placements, every slot of every D live at least once; at D = 8, where squared_norm sums by a pairwise tree, the adjacent
pairs, and the anti-diagonal pairs held to each other's bits) and every output must keep the two-column problem's BITS
(np.array_equal); whatever belongs to a dummy column (d mean / dx_k, d var / dx_k, d lml / d lengthscale_k) must be an
exact zero.  Why that holds, and why two live coordinates: dims_support's docstring and DESIGN.md §2.  The two-column
problem is tied to the numpy oracle in the same test, at the tolerance the service's own GPU test applies to that
quantity, so the chain is oracle <-> device at d = 2 <-> device at every D.  The tolerances' sources:
  fit, predict        tests/test_parity_gpu.py::test_ragged_sizes_and_dims (mean 1e-7 / 1e-9, variance 1e-6, L 1e-9 / 1e-12,
                      alpha 1e-6 / 1e-9); acquisition and winner ::test_acquisition_sweep_matches_oracle (rtol 1e-5 where
                      above 1e-6 of the maximum, the same index)
  fp32 sweep          tests/test_f32_gpu.py (variance 2e-4 (1 + max v), acquisition 5e-5 of its maximum, mean 1e-5 of max |y|,
                      the oracle's winner among the top 8)
  covariance          tests/test_covariance_gpu.py (1e-9 sigma^2); samples: tests/test_posterior_samples_gpu.py's
                      check_factor at 1e-9 sigma^2 and check_product; IVR: tests/test_ivr_gpu.py's restated() and its bound
  greedy batch        tests/test_batch_gpu.py::test_last_pick_against_the_long_double_refit (conftest.assert_parity, rtol 1e-5)
  append              tests/test_append_block_gpu.py against a fresh model on the grown data (mean 1e-9 / 1e-11, variance
                      1e-8 / 1e-13, acquisition 1e-6, the same winner, L 1e-10 / 1e-13, alpha 1e-7 / 1e-9), the fresh model
                      against the oracle as for fit
  likelihood          tests/test_parity_gpu.py::test_likelihood_gradients_match_the_restatement (lml rel 1e-9, gradients rel
                      1e-6 / 1e-8 of the largest)
  prediction grads    ::test_prediction_gradients_for_a_whole_grid (1e-8 of max |dmean|, 1e-7 of max |dvar|)
  hyper-marginalised  tests/test_hyper_gpu.py's accuracy form (conftest.assert_parity, rtol 1e-5, where above 1e-6 of the maximum)
  predict_do          ::test_do_calculus_inputs_built_on_the_device (mean 1e-9 / 1e-12, variance 1e-7)
  one-launch sets     the winner of the oracle at rtol 1e-5 (the smoke run's bar); further picks of the batch: the bits of
                      cbo_acq_sweep_batch on a fitted twin (the contract of include/cbo_hip.h)
Every problem has noise 1e-2, so cond(Ky) <= n (sigma^2 + max v) / noise + 1 < 4.5e4 (dims_support.condition_bound): the
oracle alone is good to about 1e-11 and none of these bounds is near it.

Part two, all D coordinates live: one oracle comparison per D in 5..8 for each service the suite had not run beyond d = 4
(test_dense_*), ARD lengthscales sqrt(D) linspace(0.8, 1.2, D), the same tolerances; likelihood and prediction gradients by
tests/accuracy_support.check_gradients against the long-double restatements, as tests/test_accuracy_gpu.py judges them.

Shapes: n = 130 (past one 128-row block, a ragged 16-row tile and a ragged 64-tile), m = 70 (past one 64-column strip);
likelihood gradients at n = 100 (one-workgroup kernel), 200 (two-block form) and 300 (general path).

Left out on purpose:
  * HMC and every L-BFGS route (optimize, optimize_together, refine=True, cbo_acq_refine_sets, uniform anchors): their state
    depends on the number of parameters -- momentum draws and BFGS history make an embedded run a different run.
    cbo_acq_refine_sets and the HMC chains already run at d = 8 (tests/test_sets_refine_gpu.py, tests/test_hmc_sets_gpu.py).
  * the MES, constrained and point-wise epilogues: they read only q and mu and have no dimension in them.
"""
import ctypes
import warnings

import numpy as np
import pytest

import dims_support as S
from accuracy_support import check_gradients
from conftest import assert_parity
from oracle import gp_oracle as O
from oracle import truth as T

pytestmark = pytest.mark.gpu

N, M = 130, 70
OFFSET = 1000
DENSE_DIMS = (5, 6, 7, 8)


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


# --------------------------------------------------------------------------------------------------- problems
class View:
    """One concrete problem: the data, the device model's and the oracle's keyword arguments, the further point sets of
    the services (``extra``), and where its live columns are.  ``base`` is the two-column problem, ``embedded`` its
    zero-extension, ``dense`` a problem with all D coordinates live."""

    def __init__(self, X, y, Xs, hip_kw, orc_kw, extra, prior=(None, None), live=None):
        self.X, self.y, self.Xs, self.hip_kw, self.orc_kw, self.extra = X, y, Xs, hip_kw, orc_kw, extra
        self.prior_mean, self.prior_var = prior
        self.causal = prior[0] is not None
        self.D = X.shape[1]
        self.live = list(range(self.D)) if live is None else list(live)
        self.dense = live is None and self.D > 2
        self.ard = bool(hip_kw["ard"])

    def model(self, n=None, context=None, **more):
        from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
        n = self.X.shape[0] if n is None else n
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return HipGaussianProcess(self.X[:n], self.y[:n], context=context, **self.hip_kw, **more)

    def priors(self, pts):
        """(m(pts), v(pts)) for the oracle, (None, None) for a plain model."""
        return (self.prior_mean(pts), self.prior_var(pts)) if self.causal else (None, None)

    def post(self, n=None, X=None, y=None, **hyper):
        X = self.X[:n] if X is None else X
        y = self.y[:n] if y is None else y
        kw = dict(self.orc_kw)
        kw.update(hyper)
        if self.causal:
            kw["mX"], kw["vX"] = self.priors(X)
        return O.fit(X, y, **kw)


def extras(rng, d):
    """The services' further point sets in d columns (lifted with the problem) and their dimension-free inputs."""
    return dict(X1=rng.uniform(-2.0, 2.0, (37, d)), X2=rng.uniform(-2.0, 2.0, (33, d)), Xint=rng.uniform(-2.0, 2.0, (200, d)),
                Z=rng.standard_normal((5, M)), values=rng.uniform(-2.0, 2.0, (M, 1)))


LIFTED = ("X1", "X2", "Xint")


def base_view(n, m, seed, variant):
    p = S.base_problem(n, m, seed, variant)
    prior = (S.prior_mean, S.prior_var) if p["causal"] else (None, None)
    return View(p["X"], p["y"], p["Xs"], S.hip_kwargs(p), S.oracle_hyper(p), extras(np.random.default_rng(seed + 7), 2),
                prior), p


def embedded_view(base, p, D, pos):
    ex = {k: (S.embed(a, D, pos) if k in LIFTED else a) for k, a in base.extra.items()}
    prior = (S.lifted(S.prior_mean, pos), S.lifted(S.prior_var, pos)) if p["causal"] else (None, None)
    return View(S.embed(base.X, D, pos), base.y, S.embed(base.Xs, D, pos), S.hip_kwargs(p, D, pos),
                S.oracle_hyper(p, D, pos), ex, prior, live=pos)


def dense_view(n, m, D, seed):
    q = S.dense_problem(n, m, D, seed)
    hyper = dict(variance=q["variance"], lengthscale=q["lengthscale"], noise_var=q["noise_var"])
    assert S.condition_bound(n) < 4.5e4
    return View(q["X"], q["y"], q["Xs"], dict(ard=True, **hyper), hyper, extras(np.random.default_rng(seed + 7), D))


def equal_bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def compare(base_out, out, view, what, fails):
    """Every entry of an embedding's outputs against the base problem's: the same bits.  A key that starts with ``cols:``
    names an array whose last axis is the input dimension: the live columns carry the base's bits, the dummy columns exact
    zeros (either sign)."""
    assert base_out.keys() == out.keys()
    dummy = [k for k in range(view.D) if k not in view.live]
    for key, want in base_out.items():
        got = np.asarray(out[key])
        if key.startswith("cols:"):
            if not np.array_equal(got[..., view.live], np.asarray(want)):
                fails.append(f"{what}: {key} differs in the live columns")
            if not np.all(got[..., dummy] == 0.0):
                fails.append(f"{what}: {key} is not zero in a dummy column")
        elif not equal_bits(got, want):
            fails.append(f"{what}: {key} differs")


def live_form(out, view):
    """An embedding's outputs in the base problem's form: of a ``cols:`` array the live columns alone."""
    return {k: (np.asarray(val)[..., view.live] if k.startswith("cols:") else val) for k, val in out.items()}


def over_embeddings(variant, run, check, n=N, m=M, seed=11):
    """The base problem's outputs against the oracle (``check``), then every embedding of dims_support.BIT_EMBEDDINGS
    against the base's bits.  The anti-diagonal placements of D = 8 (TREE_EMBEDDINGS; squared_norm's pairwise tree, see
    dims_support) keep one set of bits among themselves: the first is held to the oracle, the others to its bits."""
    base, p = base_view(n, m, seed, variant)
    assert S.condition_bound(n, max_prior_var=0.13) < 4.5e4
    base_out = run(base)
    check(base, base_out)
    fails = []
    for D, pos in S.BIT_EMBEDDINGS:
        view = embedded_view(base, p, D, pos)
        compare(base_out, run(view), view, f"{variant} D={D} live={pos}", fails)
    first = embedded_view(base, p, *S.TREE_EMBEDDINGS[0])
    first_out = run(first)
    check(first, first_out)
    compare(live_form(first_out, first), first_out, first, f"{variant} tree D=8 live={first.live}", fails)    # the dummy columns
    for D, pos in S.TREE_EMBEDDINGS[1:]:
        view = embedded_view(base, p, D, pos)
        compare(live_form(first_out, first), run(view), view, f"{variant} tree D={D} live={pos}", fails)
    assert not fails, "\n".join(fails)


def same_as_oracle(got, want, what, rtol=1e-5):
    """conftest.assert_parity with the oracle as its own arbiter (these problems are well conditioned): rtol alone."""
    return assert_parity(got, want, want, what, rtol=rtol)


# ------------------------------------------------------------------------------------------------ fit and sweep
def incumbent(view, task):
    return float(view.y.min() if task == "min" else view.y.max())


def run_fit(view, dtype="f64"):
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    m = view.model(dtype=dtype)
    out = {}
    out["L"], out["alpha"] = m.posterior_state()
    out["mean"], out["var"] = m.predict(view.Xs)
    grid = CandidateGrid(view.Xs, m, index_offset=OFFSET)
    for task in ("min", "max"):
        r = CausalExpectedImprovement(incumbent(view, task), task, m).sweep(grid, cost=1.0, want_acq=True, want_posterior=True)
        for k, val in r.items():
            out[f"{task}:{k}"] = val
    grid.close()
    m.close()
    return out


def check_fit(view, out, dtype="f64"):
    post = view.post()
    mXs, vXs = view.priors(view.Xs)
    mu, v = O.predict(post, view.Xs, mXs, vXs)
    assert post.tries == 0
    assert np.allclose(out["L"], post.L, rtol=1e-9, atol=1e-12) and np.allclose(out["alpha"], post.alpha, rtol=1e-6, atol=1e-9)
    f32 = dtype == "f32"
    var_tol = 2e-4 * (1.0 + (float(np.max(vXs)) if view.causal else 0.0))
    for mean, var in ((out["mean"], out["var"]), (out["min:mean"], out["min:var"]), (out["max:mean"], out["max:var"])):
        if f32:
            assert np.max(np.abs(mean - mu)) <= 1e-5 * np.max(np.abs(view.y)) and np.max(np.abs(var - v)) <= var_tol
        else:
            assert np.allclose(mean, mu, rtol=1e-7, atol=1e-9) and np.allclose(var, v, rtol=1e-6)
    for task in ("min", "max"):
        acq, val, idx, _, _ = O.acquisition_sweep(post, view.Xs, incumbent(view, task), mXs, vXs, task, 1.0)
        got = out[f"{task}:acq"]
        assert int(np.argmax(got[:, 0])) + OFFSET == out[f"{task}:best_idx"]
        assert got[out[f"{task}:best_idx"] - OFFSET, 0] == out[f"{task}:best_val"]
        if f32:
            assert np.max(np.abs(got - acq)) <= 5e-5 * np.max(np.abs(acq))
            assert idx in np.argsort(-got[:, 0], kind="stable")[:8]
        else:
            big = np.abs(acq[:, 0]) > 1e-6 * np.max(np.abs(acq))
            same_as_oracle(got[big], acq[big], f"acq {task}")
            assert out[f"{task}:best_idx"] == idx + OFFSET
            assert np.isclose(out[f"{task}:best_val"], val, rtol=1e-5, atol=1e-300)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("variant", S.VARIANTS)
def test_fit_and_sweep_keep_their_bits_under_zero_extension(hip, variant, dtype):
    """kmat_tile_kernel<D, false> (fit, K*) and <D, true> (the fp32 sweep), prep_points*, the factorisation and the sweep's
    substitution behind them: L, alpha, predict, and both tasks' acquisition, posterior and winner (with an index offset)."""
    over_embeddings(variant, lambda v: run_fit(v, dtype), lambda v, out: check_fit(v, out, dtype))


# ---------------------------------------------------------------------------------------------- joint posterior
def run_joint(view):
    from cbo_with_oop_amd import IntegratedVarianceReduction
    m = view.model()
    ex = view.extra
    out = {}
    out["mean"], out["cov"] = m.predict(view.Xs, full_cov=True)
    out["cross"] = m.posterior_covariance_between_points(ex["X1"], ex["X2"])
    out["samples"] = m.posterior_samples_f(view.Xs, size=5, normals=ex["Z"])
    out["sample_jitter"] = np.array(m.last_sample_jitter, dtype=np.float64)
    ivr = IntegratedVarianceReduction(m, [(-2.0, 2.0)] * view.D, x_monte_carlo=ex["Xint"])
    out["ivr"] = ivr.evaluate(view.Xs)
    m.close()
    return out


def check_joint(view, out):
    from test_covariance_gpu import restated_cov
    from test_ivr_gpu import restated
    from test_posterior_samples_gpu import check_factor, check_product, device_factor
    post, ex = view.post(), view.extra
    sig2, noise = post.variance, post.noise_var
    vXs, v1, v2, vi = (view.priors(a)[1] for a in (view.Xs, ex["X1"], ex["X2"], ex["Xint"]))
    sigma = restated_cov(post, view.Xs, view.Xs, vXs, vXs, sym=True)
    assert np.max(np.abs(out["cov"] - (sigma + noise * np.eye(M)))) <= 1e-9 * sig2
    assert np.array_equal(out["cov"], out["cov"].T)
    assert np.max(np.abs(out["cross"] - restated_cov(post, ex["X1"], ex["X2"], v1, v2))) <= 1e-9 * sig2
    m = view.model()
    assert np.array_equal(out["mean"], m.predict(view.Xs)[0])
    L, mean, (tries, jitter) = device_factor(m, view.Xs)
    assert (tries == 0) == (jitter == 0.0)
    check_factor(L, sigma, jitter, 1e-9 * sig2)
    check_product(out["samples"][:, 0, :], mean, L, ex["Z"])
    m.close()
    ref, bound = restated(post, view.Xs, ex["Xint"], vXs, vi)
    assert np.all(np.abs(out["ivr"] - ref) <= bound), np.max(np.abs(out["ivr"] - ref) / bound)


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_joint_posterior_keeps_its_bits_under_zero_extension(hip, variant):
    """cov_tile_kernel<D, true> (predict(full_cov=True), the samples' Sigma), <D, false> (37 x 33 cross covariance) and
    ivr_tile_kernel<D> (200 integration points); the samples' jitter ladder included."""
    over_embeddings(variant, run_joint, check_joint)


# --------------------------------------------------------------------------------------------- batch and append
B = 5
N0, K_BLOCK = 130, 9            # (121 + 9 would cross the 128-row padding, where append_block declines by contract)
N1 = N0 + K_BLOCK


def run_batch(view):
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    m = view.model(N)
    out = {}
    grid = CandidateGrid(view.Xs, m, index_offset=OFFSET)
    for update in (0, 1):
        r = CausalExpectedImprovement(incumbent(view, "min"), "min", m).sweep_batch(
            grid, B, cost=1.0, update_incumbent=bool(update), want_acq=True, want_posterior=True)
        for k, val in r.items():
            out[f"batch{update}:{k}"] = val
    grid.close()
    m.close()
    return out


def check_batch(view, out):
    """tests/test_batch_gpu.py::test_last_pick_against_the_long_double_refit with the oracle (cond(Ky) < 4.5e4) as the
    arbiter: mean and variance at the last pick against a refit on the data the believer would have, the device's own
    picks taken as given (no near-tie decides the check)."""
    post0 = view.post(N)
    mXs, vXs = view.priors(view.Xs)
    believed, _ = O.predict(post0, view.Xs, mXs, vXs)
    for update in (0, 1):
        idxs = out[f"batch{update}:best_idx"]
        assert np.all((idxs >= OFFSET) & (idxs < OFFSET + M))
        picks = (idxs - OFFSET)[:B - 1]
        post = view.post(X=np.vstack([view.X[:N], view.Xs[picks]]), y=np.vstack([view.y[:N], believed[picks]]))
        mu, v = O.predict(post, view.Xs, mXs, vXs)
        same_as_oracle(out[f"batch{update}:var"], v, "variance at the last pick")
        scale = 3 * np.max(np.abs(view.y))
        same_as_oracle(out[f"batch{update}:mean"] + scale, mu + scale, "mean at the last pick")
    acq, val, idx, _, _ = O.acquisition_sweep(post0, view.Xs, incumbent(view, "min"), mXs, vXs, "min", 1.0)
    assert out["batch0:best_idx"][0] == out["batch1:best_idx"][0] == idx + OFFSET                # pick 0 is the plain sweep's
    assert np.isclose(out["batch0:best_val"][0], val, rtol=1e-5, atol=1e-300)


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_greedy_batch_keeps_its_bits_under_zero_extension(hip, variant):
    """batch_final_kernel<D> (K(x_pick, X*) of the general path): five picks, the incumbent fixed and moving."""
    over_embeddings(variant, run_batch, check_batch, n=N + 1)


def sweep_of(m, grid, best):
    from cbo_with_oop_amd import CausalExpectedImprovement
    return CausalExpectedImprovement(best, "min", m).sweep(grid, cost=1.0, want_acq=True, want_posterior=True)


def run_append(view):
    from cbo_with_oop_amd import CandidateGrid
    X, y = view.X, view.y
    m = view.model(N0)
    grid = CandidateGrid(view.Xs, m, keep_solution=True)
    out = {}
    sweep_of(m, grid, float(y[:N0].min()))
    assert m.append_block(X[N0:N1], y[N0:N1])
    for k, val in sweep_of(m, grid, float(y[:N1].min())).items():
        out[f"block:{k}"] = val
    out["block:L"], out["block:alpha"] = m.posterior_state()
    assert m.append(X[N1], y[N1, 0])
    for k, val in sweep_of(m, grid, float(y[:N1 + 1].min())).items():
        out[f"row:{k}"] = val
    out["row:L"], out["row:alpha"] = m.posterior_state()
    grid.close()
    m.close()
    return out


def check_append(view, out):
    mXs, vXs = view.priors(view.Xs)
    for tag, n in (("block", N1), ("row", N1 + 1)):
        fresh = view.model(n)
        b = sweep_of(fresh, view.Xs, float(view.y[:n].min()))
        np.testing.assert_allclose(out[f"{tag}:mean"], b["mean"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(out[f"{tag}:var"], b["var"], rtol=1e-8, atol=1e-13)
        big = b["acq"][:, 0] > 1e-6 * b["acq"].max()
        np.testing.assert_allclose(out[f"{tag}:acq"][big], b["acq"][big], rtol=1e-6)
        assert out[f"{tag}:best_idx"] == b["best_idx"]
        L, alpha = fresh.posterior_state()
        np.testing.assert_allclose(out[f"{tag}:L"], L, rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(out[f"{tag}:alpha"], alpha, rtol=1e-7, atol=1e-9)
        fresh.close()
        post = view.post(n)
        mu, v = O.predict(post, view.Xs, mXs, vXs)
        assert np.allclose(b["mean"], mu, rtol=1e-7, atol=1e-9) and np.allclose(b["var"], v, rtol=1e-6)
        assert np.allclose(L, post.L, rtol=1e-9, atol=1e-12) and np.allclose(alpha, post.alpha, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_appends_keep_their_bits_under_zero_extension(hip, variant):
    """The append kernels' K(Xb, X*): a block of 9 onto 130 rows with a kept solution and the sweep that extends the resident
    V (factor, alpha, the q-derived variance, the winner), then one more row by ``append`` and its sweep."""
    over_embeddings(variant, run_append, check_append, n=N1 + 1)


# ------------------------------------------------------------------------------------------ likelihood gradients
def run_lml(view):
    from cbo_with_oop_amd.GaussianProcessFactory import lml_gradients_batch
    small = view.X.shape[0] <= 128
    m = view.model(fit=not small)
    out = {}
    dv, dls, dn = m.log_likelihood_gradients()
    out["lml"], out["dvariance"], out["dnoise"] = m._last_lml, dv, dn
    out["cols:dls" if view.ard else "dls"] = dls
    other = view.model(view.X.shape[0] - 3, fit=not small)
    b_lml, b_dv, b_dls, b_dn = lml_gradients_batch([other, m])[1]
    out["batch:lml"], out["batch:dvariance"], out["batch:dnoise"] = b_lml, b_dv, b_dn
    out["cols:batch:dls" if view.ard else "batch:dls"] = b_dls
    other.close()
    m.close()
    return out


def check_lml(view, out):
    post = view.post()
    o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
    scale = max(abs(o_dv), np.max(np.abs(o_dls)), abs(o_dn))
    for tag in ("", "batch:"):
        assert out[tag + "lml"] == pytest.approx(O.log_marginal_likelihood(post), rel=1e-9)
        assert out[tag + "dvariance"] == pytest.approx(o_dv, rel=1e-6, abs=1e-8 * scale)
        assert out[tag + "dnoise"] == pytest.approx(o_dn, rel=1e-6, abs=1e-8 * scale)
        dls = out["cols:" + tag + "dls"] if view.ard else out[tag + "dls"]
        np.testing.assert_allclose(dls, o_dls, rtol=1e-6, atol=1e-8 * scale)


@pytest.mark.parametrize("n", [100, 200, 300])
@pytest.mark.parametrize("variant", S.VARIANTS)
def test_likelihood_gradients_keep_their_bits_under_zero_extension(hip, variant, n):
    """small_lml_kernel<D> (n = 100), mid_lml_body<D> (200) and lml_grad_tile_kernel<D> (300), alone and through
    lml_gradients_batch: lml, d/d variance, d/d noise and the live lengthscales' gradients keep their bits, a dummy
    lengthscale's gradient is an exact zero; the iso model's single lengthscale gradient keeps its bits."""
    over_embeddings(variant, run_lml, check_lml, n=n)


# ------------------------------------------------------------------------------------------ prediction gradients
def forced_context(monkeypatch, **env):
    """A fresh context whose knobs are pinned (they are read when the context is created)."""
    from cbo_with_oop_amd import _lib
    for k, val in env.items():
        monkeypatch.setenv(k, str(val))
    ctx = _lib.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def run_pred_gradients(view, ctx2):
    out = {}
    for tag, ctx in (("", None), ("chunked:", ctx2)):
        m = view.model(context=ctx)
        out["cols:" + tag + "dmean"], out["cols:" + tag + "dvar"] = m.get_prediction_gradients(view.Xs)
        m.close()
    return out


def check_pred_gradients(view, out):
    dmo, dvo = O.predict_gradients(view.post(), view.Xs, view.priors(view.Xs)[1])
    assert np.max(np.abs(out["cols:dmean"] - dmo)) <= 1e-8 * np.max(np.abs(dmo))
    assert np.max(np.abs(out["cols:dvar"] - dvo)) <= 1e-7 * np.max(np.abs(dvo))
    assert np.array_equal(out["cols:chunked:dmean"], out["cols:dmean"])
    assert np.array_equal(out["cols:chunked:dvar"], out["cols:dvar"])


@pytest.fixture
def one_strip_context(monkeypatch):
    """A context without a workspace budget: every chunked call works one 64-column strip at a time, so 70 points take two
    chunks (cbo_api.hip, ensure_workspaces: at least one strip)."""
    ctx = forced_context(monkeypatch, CBO_HIP_WORKSPACE_MB=0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_prediction_gradients_keep_their_bits_under_zero_extension(hip, variant, one_strip_context):
    """pred_gradients_kernel at 70 points, in one chunk and in two: the live columns keep their bits, d / dx_k of a dummy
    column is an exact zero."""
    over_embeddings(variant, lambda v: run_pred_gradients(v, one_strip_context), check_pred_gradients)


# --------------------------------------------------------------------------------------- hyper-marginalised sweep
HYPER_FACTORS = np.array([[1.0, 1.0, 1.0, 1.0], [0.6, 1.5, 0.8, 2.0], [1.7, 0.7, 1.3, 1.0]])     # variance, ls, ls, noise


def hyper_rows(view):
    """H = 3 rows of (variance, lengthscale x L, noise): the model's own and two spread around them.  An embedded ARD row
    carries the D lengthscales embed_lengthscales builds from the row's two live ones."""
    ls = np.atleast_1d(np.asarray(view.hip_kw["lengthscale"], dtype=np.float64))
    rows = []
    for f in HYPER_FACTORS:
        if not view.ard:
            scaled = ls * f[1]
        elif view.dense:
            scaled = ls * np.linspace(f[1], f[2], view.D)
        else:
            scaled = ls[view.live] * f[1:3]
            if view.D > 2:
                scaled = S.embed_lengthscales(scaled, view.D, view.live)
        rows.append(np.concatenate([[view.hip_kw["variance"] * f[0]], scaled, [view.hip_kw["noise_var"] * f[3]]]))
    return np.ascontiguousarray(rows)


def run_hyper(view):
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement, IntegratedHyperParameterAcquisition
    m = view.model()
    grid = CandidateGrid(view.Xs, m, index_offset=OFFSET)
    out = {}
    for task in ("min", "max"):
        yb = incumbent(view, task)
        acq = IntegratedHyperParameterAcquisition(m, lambda mdl: CausalExpectedImprovement(yb, task, mdl), samples=hyper_rows(view))
        r = acq.sweep(grid, cost=1.0, want_acq=True)
        out[f"{task}:acq"], out[f"{task}:best_val"], out[f"{task}:best_idx"] = r["acq"], r["best_val"], r["best_idx"]
    grid.close()
    m.close()
    return out


def check_hyper(view, out):
    mXs, vXs = view.priors(view.Xs)
    rows = hyper_rows(view)
    for task in ("min", "max"):
        total = np.zeros((M, 1))
        for row in rows:
            post = view.post(variance=float(row[0]), lengthscale=row[1:-1].copy() if view.ard else float(row[1]),
                             noise_var=float(row[-1]))
            total = total + O.acquisition_sweep(post, view.Xs, incumbent(view, task), mXs, vXs, task, 1.0)[0]
        want = total / rows.shape[0]
        got = out[f"{task}:acq"]
        big = np.abs(want[:, 0]) > 1e-6 * np.max(np.abs(want))
        same_as_oracle(got[big], want[big], f"marginalised acq {task}")
        assert out[f"{task}:best_idx"] == int(np.argmax(got[:, 0])) + OFFSET
        assert out[f"{task}:best_val"] == got[out[f"{task}:best_idx"] - OFFSET, 0]
        assert out[f"{task}:best_idx"] == int(np.argmax(want[:, 0])) + OFFSET


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_hyper_marginalised_sweep_keeps_its_bits_under_zero_extension(hip, variant):
    """cbo_acq_sweep_hyper's general path (n = 130) with H = 3 rows; an ARD row carries D lengthscales."""
    over_embeddings(variant, run_hyper, check_hyper)


# ------------------------------------------------------------------------------------------------- predict_do
N_OBS = 33


def do_indices(view):
    """Two intervention layouts: values[:, 0] into the first live column, then into the last; every other column observed."""
    out = []
    for col in (view.live[0], view.live[-1]):
        idx = [-1] * view.D
        idx[col] = 0
        out.append(idx)
    return out


def run_predict_do(view):
    m = view.model()
    out = {}
    for i, idx in enumerate(do_indices(view)):
        out[f"do{i}:mean"], out[f"do{i}:var"] = m.predict_do(view.X[:N_OBS], idx, view.extra["values"])
    m.close()
    return out


def check_predict_do(view, out):
    from cbo_with_oop_amd.DoCalculus import intervened_inputs
    post = view.post()
    for i, idx in enumerate(do_indices(view)):
        x = intervened_inputs(view.X[:N_OBS], idx, view.extra["values"])
        mo, vo = O.predict(post, x)
        assert np.allclose(out[f"do{i}:mean"][:, 0], mo.reshape(M, N_OBS).mean(1), rtol=1e-9, atol=1e-12)
        assert np.allclose(out[f"do{i}:var"][:, 0], vo.reshape(M, N_OBS).mean(1), rtol=1e-7, atol=0)


@pytest.mark.parametrize("variant", ["iso", "ard"])
def test_predict_do_keeps_its_bits_under_zero_extension(hip, variant):
    """cbo_gp_predict_do (plain models only), the dummy columns kept as observed (-1 in the index)."""
    over_embeddings(variant, run_predict_do, check_predict_do)


# ------------------------------------------------------------------------------------------ one-launch small models
SETS = [(17, 65), (50, 130), (128, 200)]


def set_views(variant, seed=23):
    return [base_view(n, m, seed + n, variant) for n, m in SETS]


def handles(objs):
    return (ctypes.c_void_p * len(objs))(*[o._handle for o in objs])


def run_sets(views):
    from cbo_with_oop_amd import CandidateGrid, _lib
    from sets_batch_support import sets_batch
    models = [v.model(fit=False) for v in views]
    grids = [CandidateGrid(v.Xs, m, index_offset=OFFSET * (i + 1)) for i, (v, m) in enumerate(zip(views, models))]
    s = len(views)
    costs = np.ones(s)
    out = {}
    for task in ("min", "max"):
        yb = np.array([incumbent(v, task) for v in views])
        vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
        _lib.check(_lib.load().cbo_acq_sweep_sets(s, handles(models), handles(grids), _lib.dptr(yb), _lib.TASK_CODE[task], 0.0,
                                                  _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)))
        out[f"sets:{task}:val"], out[f"sets:{task}:idx"] = vals, idxs
        for update in (0, 1):
            rc, bv, bi = sets_batch(_lib, models, grids, yb, task, 3, costs, update=update)
            _lib.check(rc)
            out[f"batch{update}:{task}:val"], out[f"batch{update}:{task}:idx"] = bv, bi
    assert all(m.stale for m in models)                                      # the launches left the models alone
    for o in grids + models:
        o.close()
    return out


def check_sets(views, out):
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement
    for task in ("min", "max"):
        for i, v in enumerate(views):
            mXs, vXs = v.priors(v.Xs)
            yb = incumbent(v, task)
            _, val, idx, _, _ = O.acquisition_sweep(v.post(), v.Xs, yb, mXs, vXs, task, 1.0)
            assert out[f"sets:{task}:idx"][i] == idx + OFFSET * (i + 1)
            assert np.isclose(out[f"sets:{task}:val"][i], val, rtol=1e-5, atol=1e-300)
            twin = v.model()
            grid = CandidateGrid(v.Xs, twin, index_offset=OFFSET * (i + 1))
            for update in (0, 1):
                r = CausalExpectedImprovement(yb, task, twin).sweep_batch(grid, 3, cost=1.0, update_incumbent=bool(update))
                assert np.array_equal(out[f"batch{update}:{task}:idx"][i], r["best_idx"])
                assert equal_bits(out[f"batch{update}:{task}:val"][i], r["best_val"])
                assert out[f"batch{update}:{task}:idx"][i][0] == out[f"sets:{task}:idx"][i]
                assert out[f"batch{update}:{task}:val"][i][0] == out[f"sets:{task}:val"][i]
            grid.close()
            twin.close()


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_one_launch_small_models_keep_their_bits_under_zero_extension(hip, variant):
    """small_assemble<D>, small_kstar<D> (cbo_acq_sweep_sets) and small_batch_picks<D> (cbo_acq_sweep_sets_batch, B = 3), which
    every other one-launch kind shares: three unfitted sets (n = 17, 50, 128; m = 65, 130, 200), all embedded alike."""
    pairs = set_views(variant)
    views = [v for v, _ in pairs]
    base_out = run_sets(views)
    check_sets(views, base_out)
    fails = []
    embedded = lambda D, pos: [embedded_view(v, p, D, pos) for v, p in pairs]
    for D, pos in S.BIT_EMBEDDINGS:
        compare(base_out, run_sets(embedded(D, pos)), views[0], f"{variant} D={D} live={pos}", fails)
    first = embedded(*S.TREE_EMBEDDINGS[0])
    first_out = run_sets(first)
    check_sets(first, first_out)
    for D, pos in S.TREE_EMBEDDINGS[1:]:
        compare(first_out, run_sets(embedded(D, pos)), views[0], f"{variant} tree D={D} live={pos}", fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------- part two: all D coordinates live
@pytest.mark.parametrize("D", DENSE_DIMS)
def test_dense_joint_posterior_against_the_oracle(hip, D):
    view = dense_view(N, M, D, seed=100 + D)
    check_joint(view, run_joint(view))


@pytest.mark.parametrize("D", DENSE_DIMS)
def test_dense_greedy_batch_and_appends_against_the_oracle(hip, D):
    view = dense_view(N1 + 1, M, D, seed=200 + D)
    check_batch(view, run_batch(view))
    check_append(view, run_append(view))


@pytest.mark.parametrize("D", DENSE_DIMS)
def test_dense_hyper_marginalised_sweep_against_the_oracle(hip, D):
    view = dense_view(N, M, D, seed=300 + D)
    check_hyper(view, run_hyper(view))


@pytest.mark.parametrize("D", DENSE_DIMS)
def test_dense_fp32_sweep_and_predict_do_against_the_oracle(hip, D):
    view = dense_view(N, M, D, seed=400 + D)
    check_fit(view, run_fit(view, "f32"), "f32")
    check_predict_do(view, run_predict_do(view))


@pytest.mark.parametrize("n", [N, 300])
@pytest.mark.parametrize("D", DENSE_DIMS)
def test_dense_likelihood_gradients_against_long_double(hip, D, n):
    """mid_lml_body<D> (n = 130) and lml_grad_tile_kernel<D> (n = 300) by tests/test_accuracy_gpu.py's criterion: the fp64
    oracle and the long-double truth both on the device's fitted factor, |HIP - truth| <= 8 |oracle - truth| + 4 eps mag."""
    from cbo_with_oop_amd.GaussianProcessFactory import lml_gradients_batch
    view = dense_view(n, M, D, seed=500 + D + n)
    m = view.model()
    dv, dls, dn = m.log_likelihood_gradients()
    lml = m._last_lml
    L, alpha = m.posterior_state()
    ls = m.lengthscale
    truth, mag = T.lml_and_gradients(L, view.X, view.y, None, None, m.variance, ls)
    post = O.Posterior(view.X, view.y, None, None, m.variance, ls, m.noise_var, L, alpha, 0.0, 0, False)
    o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
    vec = lambda a, b, c, dd: np.concatenate([[a, b, c], np.atleast_1d(np.asarray(dd, dtype=np.longdouble))])
    tv = vec(truth["lml"], truth["d_variance"], truth["d_noise"], truth["d_lengthscale"])
    mv = vec(mag["lml"], mag["d_variance"], mag["d_noise"], mag["d_lengthscale"])
    ov = np.concatenate([[O.log_marginal_likelihood(post), o_dv, o_dn], o_dls])
    g = check_gradients(np.concatenate([[lml, dv, dn], dls]), ov, tv, mv, f"lml gradients D={D} n={n}")
    print(f"\nMEASURED lml D={D} n={n}: hip {g['hip_err']:.2e} oracle {g['oracle_err']:.2e} ratio {g['ratio']:.2f}")
    assert g["ok"], g
    if n <= 256:
        other = view.model(n - 3)
        b_lml, b_dv, b_dls, b_dn = lml_gradients_batch([other, m])[1]
        gb = check_gradients(np.concatenate([[b_lml, b_dv, b_dn], b_dls]), ov, tv, mv, f"batched D={D} n={n}")
        assert gb["ok"], gb
        other.close()
    m.close()


@pytest.mark.parametrize("D", DENSE_DIMS)
def test_dense_prediction_gradients_against_long_double(hip, D, one_strip_context):
    """pred_gradients_kernel with every inv_ls[k] in use, by tests/test_accuracy_gpu.py's criterion (dvar: floor 32 eps, its
    module docstring says why); the chunked call gives the same bits."""
    view = dense_view(N, M, D, seed=600 + D)
    out = run_pred_gradients(view, one_strip_context)
    m = view.model()
    L, alpha = m.posterior_state()
    ls = m.lengthscale
    t_mean, t_var, mag_mean, mag_var = T.prediction_gradients(L, alpha, view.X, view.Xs, None, None, m.variance, ls)
    post = O.Posterior(view.X, view.y, None, None, m.variance, ls, m.noise_var, L, alpha, 0.0, 0, False)
    o_mean, o_var = O.predict_gradients(post, view.Xs, None)
    gm = check_gradients(out["cols:dmean"], o_mean, t_mean, mag_mean, f"dmean D={D}")
    gv = check_gradients(out["cols:dvar"], o_var, t_var, mag_var, f"dvar D={D}", floor_eps=32.0)
    print(f"\nMEASURED pred grads D={D}: dmean ratio {gm['ratio']:.2f} dvar ratio {gv['ratio']:.2f}")
    assert gm["ok"], gm
    assert gv["ok"], gv
    assert np.array_equal(out["cols:chunked:dmean"], out["cols:dmean"])
    assert np.array_equal(out["cols:chunked:dvar"], out["cols:dvar"])
    m.close()
