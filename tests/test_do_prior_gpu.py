"""GPU tests of the device-resident do-calculus prior: cbo_do_prior_create / _eval / _destroy and DoPrior.

References: the numpy oracle's row-by-row do_prior and the library's own cbo_gp_predict_do, both at the value bars of
tests/test_parity_gpu.py (rtol 1e-6, atol 1e-12).  Graph GPs have variance and lengthscales of order 1 and the reference's
noise 1e-2 (utils.py:43); n_g runs over the edges of the 16-row tile, the 64-lane wave, the 128-column Gram tile and the
256-lane group (1, 15, 16, 17, 64, 65, 129, 300), N_obs over {1, 37, 130} (one row, a partial 16-row stage, more than one
128-row tile of b), d_in over 1..4 with one lengthscale and ARD, the intervened indices permuted, all columns intervened and
one column of several."""
import warnings

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

VALUE_BAR = dict(rtol=1e-6, atol=1e-12)
UNSUPPORTED = -6

#        n_g d_in n_obs intervened_index   ard
CASES = [(1, 1, 1, [0], False),
         (15, 2, 37, [0, -1], False),
         (16, 2, 37, [-1, 0], True),
         (17, 3, 130, [1, -1, 0], True),
         (64, 3, 37, [0, 1, 2], False),              # all columns intervened: b = 1
         (65, 4, 37, [-1, -1, 0, -1], True),         # one column of several
         (129, 4, 130, [2, 0, -1, 1], True),
         (300, 2, 130, [0, -1], False),
         (300, 3, 1, [1, 0, -1], True)]


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def graph_gp(n_g, d_in, ard, noise=1e-2, seed=0, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(100 * n_g + 10 * d_in + seed)
    X = rng.uniform(-2.0, 2.0, (n_g, d_in))
    y = np.sin(1.1 * X[:, :1]) + 0.2 * (X ** 2).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n_g, 1))
    hyper = dict(variance=1.4, lengthscale=rng.uniform(0.8, 1.6, d_in) if ard else 1.3, noise_var=noise)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        gp = HipGaussianProcess(X, y, ard=ard, fix_noise=True, **hyper, **kw)
    return gp, X, y, hyper, rng


@pytest.mark.parametrize("n_g,d_in,n_obs,idx,ard", CASES, ids=[f"n{c[0]} d{c[1]} obs{c[2]} {c[3]}" for c in CASES])
def test_eval_matches_the_oracle_and_predict_do(lib, n_g, d_in, n_obs, idx, ard):
    from cbo_with_oop_amd.DoCalculus import DoPrior
    gp, X, y, hyper, rng = graph_gp(n_g, d_in, ard)
    observed = rng.uniform(-2.0, 2.0, (n_obs, d_in))
    n_iv = max(idx) + 1
    values = rng.uniform(-2.2, 2.2, (7, n_iv))
    values[0] = X[0, [idx.index(k) for k in range(n_iv)]]            # a point ON a row of the graph GP: a_0 = 1
    prior = DoPrior(gp, observed, idx)
    again = DoPrior(gp, observed, idx)
    mean, var = prior.evaluate(values)
    assert mean.shape == var.shape == (7, 1)
    post = O.fit(X, y, **hyper)
    np.testing.assert_allclose(mean, O.do_prior(post, observed, idx, values, 0), **VALUE_BAR)
    np.testing.assert_allclose(var, O.do_prior(post, observed, idx, values, 1), **VALUE_BAR)
    pm, pv = gp.predict_do(observed, idx, values)
    np.testing.assert_allclose(mean, pm, **VALUE_BAR)
    np.testing.assert_allclose(var, pv, **VALUE_BAR)
    # two evaluations, and two creations, give the same bits; so does a point alone against the point in a batch
    m2, v2 = prior.evaluate(values)
    m3, v3 = again.evaluate(values)
    m4, v4 = prior.evaluate(values[3:4])
    assert np.array_equal(mean, m2) and np.array_equal(var, v2)
    assert np.array_equal(mean, m3) and np.array_equal(var, v3)
    assert m4[0, 0] == mean[3, 0] and v4[0, 0] == var[3, 0]
    prior.close()
    again.close()
    prior.close()                                                    # (closing twice is harmless)
    with pytest.raises(ValueError, match="closed"):
        prior.evaluate(values)
    gp.close()


def test_many_points_take_several_turns_per_workgroup(lib):
    """More points than the launch has workgroups (512): a workgroup's later turns reuse its scratch."""
    from cbo_with_oop_amd.DoCalculus import DoPrior
    gp, X, y, hyper, rng = graph_gp(17, 2, False)
    observed = rng.uniform(-2.0, 2.0, (5, 2))
    prior = DoPrior(gp, observed, [0, -1])
    values = rng.uniform(-2.0, 2.0, (1100, 1))
    mean, var = prior.evaluate(values)
    post = O.fit(X, y, **hyper)
    np.testing.assert_allclose(mean, O.do_prior(post, observed, [0, -1], values, 0), **VALUE_BAR)
    np.testing.assert_allclose(var, O.do_prior(post, observed, [0, -1], values, 1), **VALUE_BAR)
    m1, v1 = prior.evaluate(values[1050:1051])
    assert m1[0, 0] == mean[1050, 0] and v1[0, 0] == var[1050, 0]
    prior.close()
    gp.close()


def test_refusals_name_their_reason(lib):
    from cbo_with_oop_amd.DoCalculus import DoPrior

    def refused(gp, observed, idx, word):
        with pytest.raises(lib.CboHipError) as e:
            DoPrior(gp, observed, idx)
        assert e.value.code == UNSUPPORTED and word in str(e.value), str(e.value)
        gp.close()

    obs = np.zeros((3, 2))
    refused(graph_gp(20, 2, False, dtype="f32")[0], obs, [0, -1], "fp32")
    refused(graph_gp(20, 2, False, mean_function=lambda x: np.zeros((len(x), 1)),
                     variance_adjustment=lambda x: np.full((len(x), 1), 0.1))[0], obs, [0, -1], "causal")
    refused(graph_gp(1025, 2, False)[0], obs, [0, -1], "CBO_DO_PRIOR_MAX_N")
    refused(graph_gp(300, 2, False, noise=1e-10)[0], obs, [0, -1], "clip")
    # (1024 rows are taken)
    gp = graph_gp(1024, 2, False)[0]
    DoPrior(gp, obs, [0, -1]).close()
    gp.close()


def test_the_graph_gp_is_untouched(lib):
    from cbo_with_oop_amd import CausalExpectedImprovement
    from cbo_with_oop_amd.DoCalculus import DoPrior
    from cbo_with_oop_amd.utils_functions.causal_acquisition_functions import CandidateGrid
    gp, X, y, hyper, rng = graph_gp(200, 2, True)
    Xs = rng.uniform(-2.0, 2.0, (300, 2))
    kept, plain = CandidateGrid(Xs, gp, keep_solution=True), CandidateGrid(Xs, gp)
    acq = CausalExpectedImprovement(float(y.min()), "min", gp)
    before = [acq.sweep(g, cost=2.0, want_acq=True, want_posterior=True) for g in (kept, plain)]
    L0, a0 = gp.posterior_state()
    prior = DoPrior(gp, rng.uniform(-2.0, 2.0, (37, 2)), [-1, 0])
    prior.evaluate(rng.uniform(-2.0, 2.0, (5, 1)))
    assert not gp.stale
    L1, a1 = gp.posterior_state()
    assert np.array_equal(L0, L1) and np.array_equal(a0, a1)
    for g, b in zip((kept, plain), before):
        after = acq.sweep(g, cost=2.0, want_acq=True, want_posterior=True)
        assert all(np.array_equal(after[k], b[k]) for k in ("mean", "var", "acq"))
    # the handle does not refer to the model afterwards
    values = rng.uniform(-2.0, 2.0, (5, 1))
    m0, v0 = prior.evaluate(values)
    gp.close()
    m1, v1 = prior.evaluate(values)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    prior.close()
