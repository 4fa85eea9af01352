"""Host tests of the hyper-parameter priors: ``utils_functions.priors`` against ``scipy.stats`` and against
central differences, csrc/hyper_prior.h compiled by g++ (tests/support/hyper_prior_sim.cpp) against both, the draw order of
``mle_restart_starts`` with priors, and everything that is refused before a device is touched.

The rounding bar.  ``ulp`` is 2^-52 and S the sum of the absolute values of the terms an evaluation adds up, the two terms of
every constant (``a log b`` and ``lgamma a``; ``log(2 pi sigma^2) / 2``) and of the Jacobian (``log(expm1 theta)``,
``theta``) counted separately.  A term comes out of at most one library call (<= 1 ulp) and three arithmetic operations
(<= 1/2 ulp each): <= 2.5 ulp of the term; the <= 3 additions that join the terms add <= 1/2 ulp of a partial sum <= S each:
<= 1.5 ulp of S.  One evaluation is therefore within 4 ulp of S of the exact value, and two evaluations by different
formulas (ours and scipy's, numpy's and the header's) within ``BAR_ULPS`` = 8 ulp of S of each other.  The LogGaussian
squares u = log theta - mu, a difference that cancels near the mode: the rounding of u (<= 1 ulp of |log theta| + |mu|)
reaches the density through d(u^2 / 2 sigma^2) = |u| / sigma^2, so S carries that product as one more term."""
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import stats

from conftest import ROOT
from cbo_with_oop_amd import _lib
from cbo_with_oop_amd.utils_functions import priors as PR
import importlib

F = importlib.import_module("cbo_with_oop_amd.GaussianProcessFactory")

ULP = 2.0 ** -52
BAR_ULPS = 8.0
THETAS = np.array([1e-3, 3.7e-3, 2e-2, 0.11, 0.5, 1.0, 1.9, 7.3, 35.0, 36.5, 140.0, 1e3])

PRIORS = [PR.Gaussian(1.5, 0.7), PR.Gaussian(-2.0, 30.0), PR.LogGaussian(0.3, 1.1), PR.LogGaussian(-1.0, 0.25),
          PR.Gamma(2.5, 1.7), PR.Gamma.from_EV(1.0, 10.0), PR.InverseGamma(3.0, 2.0), PR.InverseGamma(0.6, 11.0)]


def scipy_logpdf(p, t):
    if type(p) is PR.Gaussian:
        return stats.norm(loc=p.mu, scale=p.sigma).logpdf(t)
    if type(p) is PR.LogGaussian:
        return stats.lognorm(s=p.sigma, scale=math.exp(p.mu)).logpdf(t)
    if type(p) is PR.Gamma:
        return stats.gamma(p.a, scale=1.0 / p.b).logpdf(t)
    return stats.invgamma(p.a, scale=p.b).logpdf(t)


def abs_terms(p, t):
    """S of the module's docstring for ``p.lnpdf(t)``."""
    t = np.asarray(t, dtype=np.float64)
    L = np.abs(np.log(t))
    if isinstance(p, PR.Gaussian):
        s2 = p.sigma * p.sigma
        const = 0.5 * abs(math.log(2.0 * math.pi)) + abs(math.log(p.sigma))
        if type(p) is PR.Gaussian:
            return const + (t - p.mu) ** 2 / (2.0 * s2)
        u = np.abs(np.log(t) - p.mu)
        return const + u * u / (2.0 * s2) + L + u / s2 * (L + abs(p.mu))
    const = abs(p.a * math.log(p.b)) + abs(math.lgamma(p.a))
    if type(p) is PR.Gamma:
        return const + abs(p.a - 1.0) * L + p.b * t
    return const + (p.a + 1.0) * L + p.b / t


def jac_terms(t):
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.where(t > 36.0, 0.0, np.abs(np.log(np.expm1(np.minimum(t, 700.0)))) + np.abs(t))


def third_derivative(p, t):
    """d^3 lnpdf / d theta^3, for the central difference's truncation bound h^2 / 6 max |f'''|."""
    t = np.asarray(t, dtype=np.float64)
    if type(p) is PR.Gaussian:
        return np.zeros_like(t)
    if type(p) is PR.LogGaussian:
        return (3.0 - 2.0 * (np.log(t) - p.mu)) / (p.sigma ** 2 * t ** 3) - 2.0 / t ** 3
    if type(p) is PR.Gamma:
        return 2.0 * (p.a - 1.0) / t ** 3
    return -2.0 * (p.a + 1.0) / t ** 3 + 6.0 * p.b / t ** 4


@pytest.mark.parametrize("p", PRIORS, ids=repr)
def test_densities_against_scipy(p):
    ours, ref = p.lnpdf(THETAS), scipy_logpdf(p, THETAS)
    bar = BAR_ULPS * ULP * abs_terms(p, THETAS)
    assert np.all(np.isfinite(ours)) and np.all(np.abs(ours - ref) <= bar), (ours - ref, bar)
    assert p.lnpdf(1.9).shape == () and float(p.lnpdf(1.9)) == ours[6]          # scalars in, scalars out, the same bits


@pytest.mark.parametrize("p", PRIORS, ids=repr)
def test_density_gradients_against_central_differences(p):
    """|quotient - f'| <= h^2 / 6 max |f'''| over [theta - h, theta + h] (f''' is a sum of theta^-3, theta^-4 and
    log(theta) theta^-3 terms: over h = 1e-4 theta it moves by less than 5e-4 of itself, hence the factor on the largest
    of the three values taken) + the quotient's rounding, twice the density's 4 ulp of S over 2 h."""
    h = 1e-4 * THETAS
    quotient = (p.lnpdf(THETAS + h) - p.lnpdf(THETAS - h)) / (2.0 * h)
    m3 = np.max(np.abs([third_derivative(p, THETAS - h), third_derivative(p, THETAS), third_derivative(p, THETAS + h)]), axis=0)
    bar = h * h / 6.0 * m3 * 1.0005 + 4.0 * ULP * np.maximum(abs_terms(p, THETAS - h), abs_terms(p, THETAS + h)) / h
    got = p.lnpdf_grad(THETAS)
    assert np.all(np.abs(got - quotient) <= bar + 4.0 * ULP * np.abs(got)), (got - quotient, bar)


def test_from_EV_and_descriptors():
    g = PR.Gamma.from_EV(2.0, 8.0)
    assert (g.a, g.b) == (0.5, 0.25)
    d = g.descriptor()
    assert (d.kind, d.p0, d.p1, d.constant) == (_lib.PRIOR_GAMMA, 0.5, 0.25, 0.5 * math.log(0.25) - math.lgamma(0.5))
    d = PR.LogGaussian(0.3, 1.1).descriptor()
    assert (d.kind, d.p0, d.p1, d.constant) == (_lib.PRIOR_LOGGAUSSIAN, 0.3, 1.1, -0.5 * math.log(2.0 * math.pi * (1.1 * 1.1)))
    assert [PR.Gaussian(0, 1).kind, PR.InverseGamma(1, 1).kind] == [_lib.PRIOR_GAUSSIAN, _lib.PRIOR_INVGAMMA]
    assert ctypes_size() == 32


def ctypes_size():
    import ctypes
    return ctypes.sizeof(_lib.CboHyperPrior)


def test_rvs_use_the_global_generator_with_gpys_formulas():
    for p, replay in ((PR.Gaussian(1.5, 0.7), lambda: np.random.randn(4) * 0.7 + 1.5),
                      (PR.LogGaussian(0.3, 1.1), lambda: np.exp(np.random.randn(4) * 1.1 + 0.3)),
                      (PR.Gamma(2.5, 1.7), lambda: np.random.gamma(shape=2.5, scale=1.0 / 1.7, size=4)),
                      (PR.InverseGamma(3.0, 2.0), lambda: 1.0 / np.random.gamma(shape=3.0, scale=1.0 / 2.0, size=4))):
        np.random.seed(11)
        got, after = p.rvs(4), np.random.rand()
        np.random.seed(11)
        want, after_want = replay(), np.random.rand()
        assert np.array_equal(got, want) and after == after_want and got.shape == (4,)


# ---- the header on the host --------------------------------------------------------------------------------------------

def hexes(v):
    return " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).reshape(-1))


def sim_input(row_priors, rows):
    """The simulator's stdin (also what a stand-alone sanitizer run of it reads)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    lines = [f"{len(row_priors)} {rows.shape[0]}"]
    for p in row_priors:
        lines.append("0 0x0p+0 0x0p+0 0x0p+0" if p is None else f"{p.kind} {hexes([p.p0, p.p1, p.constant])}")
    lines += [hexes(r) for r in rows]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """run(row_priors, rows) -> (lp (n_rows,), dlp (n_rows, P)) by hyper_prior_at compiled with g++."""
    exe = tmp_path_factory.mktemp("prior_sim") / "hyper_prior_sim"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbo_with_oop_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "hyper_prior_sim.cpp"), "-o", str(exe)])

    def run(row_priors, rows):
        out = subprocess.run([str(exe)], input=sim_input(row_priors, rows), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.returncode, out.stderr)
        vals = np.array([[float.fromhex(w) for w in line.split()[1:]] for line in out.stdout.splitlines()])
        return vals[:, 0], vals[:, 1:]
    return run


def test_header_agrees_with_the_python_priors(sim):
    """Every kind alone over the dozen thetas: the header's value against ``lnpdf`` + ``log_jacobian`` within the module's bar
    (the Jacobian's two terms in S), its gradient against ``lnpdf_grad`` + ``log_jacobian_grad`` within 8 ulp of the sum of
    the absolute values of that sum's terms."""
    for p in PRIORS:
        lp, dlp = sim([p], THETAS[:, None])
        want = p.lnpdf(THETAS) + PR.log_jacobian(THETAS)
        assert np.all(np.abs(lp - want) <= BAR_ULPS * ULP * (abs_terms(p, THETAS) + jac_terms(THETAS))), (p, lp - want)
        g, dj = p.lnpdf_grad(THETAS), PR.log_jacobian_grad(THETAS)
        gterms = {PR.Gaussian: np.abs(g), PR.LogGaussian: (np.abs(np.log(THETAS) - p.p0) / p.p1 ** 2 + 1.0) / THETAS,
                  PR.Gamma: abs(p.p0 - 1.0) / THETAS + p.p1, PR.InverseGamma: p.p1 / THETAS ** 2 + (p.p0 + 1.0) / THETAS}[type(p)]
        assert np.all(np.abs(dlp[:, 0] - (g + dj)) <= BAR_ULPS * ULP * (gterms + np.abs(dj))), (p, dlp[:, 0] - (g + dj))


def test_header_rows_sum_in_index_order_and_skip_entries_without_a_prior(sim):
    row_priors = [PR.Gamma(2.5, 1.7), None, PR.LogGaussian(0.3, 1.1), PR.Gaussian(1.5, 0.7), None, PR.InverseGamma(3.0, 2.0)]
    rng = np.random.default_rng(3)
    rows = np.exp(rng.uniform(-3.0, 3.0, (7, 6)))
    lp, dlp = sim(row_priors, rows)
    for r in range(rows.shape[0]):
        want, grad = PR.log_prior_host(row_priors, rows[r])
        S = sum(float(abs_terms(p, t) + jac_terms(t)) for p, t in zip(row_priors, rows[r]) if p is not None)
        assert abs(lp[r] - want) <= BAR_ULPS * ULP * S
        assert np.allclose(dlp[r], grad, rtol=64 * ULP, atol=0.0)
    # an entry without a prior: exactly 0 gradient, and the row's value is the one of the row without that entry, bit for bit
    assert np.all(dlp[:, [1, 4]] == 0.0) and not np.any(np.signbit(dlp[:, [1, 4]]))
    keep = [0, 2, 3, 5]
    lp_dense, dlp_dense = sim([row_priors[k] for k in keep], rows[:, keep])
    assert np.array_equal(lp, lp_dense) and np.array_equal(dlp[:, keep], dlp_dense)
    # ... whatever stands there, a value no density could take included
    odd = rows.copy()
    odd[:, 1], odd[:, 4] = -5.0, 0.0
    lp_odd, dlp_odd = sim(row_priors, odd)
    assert np.array_equal(lp_odd, lp) and np.array_equal(dlp_odd, dlp)
    # no prior at all: 0 and zeros
    lp0, dlp0 = sim([None] * 3, rows[:, :3])
    assert np.all(lp0 == 0.0) and np.all(dlp0 == 0.0)


def test_header_jacobian_is_exactly_zero_above_the_limit(sim):
    above = np.array([36.000000001, 37.0, 140.0, 1e3])
    for p in PRIORS:
        lp, dlp = sim([p], above[:, None])
        assert np.all(np.abs(lp - p.lnpdf(above)) <= BAR_ULPS * ULP * abs_terms(p, above))
        if type(p) is PR.Gaussian:            # no library call in this density: numpy's IEEE arithmetic gives the header's bits,
            assert np.array_equal(lp, p.lnpdf(above)) and np.array_equal(dlp[:, 0], p.lnpdf_grad(above))   # so nothing was added
        # the very doubles of the density: what the row [p, p] adds is twice the same two values in index order
        lp2, dlp2 = sim([p, p], np.column_stack([above, above]))
        assert np.array_equal(lp2, (0.0 + lp) + lp) and np.array_equal(dlp2[:, 0], dlp[:, 0]) and np.array_equal(dlp2[:, 1], dlp[:, 0])
        g = p.lnpdf_grad(above)
        assert np.all(np.abs(dlp[:, 0] - g) <= 8 * ULP * np.maximum(np.abs(g), 1e-300) + 8 * ULP * (np.abs(p.p1) + 1.0) / above)
    # at and below the limit the Jacobian is there (tiny but not zero): exp(-36) = 2.3e-16
    lp_at, dlp_at = sim([PR.Gaussian(36.0, 1.0)], [[36.0]])
    assert dlp_at[0, 0] == 1.0 / math.expm1(36.0) and dlp_at[0, 0] > 0.0


def test_header_derivative_along_x_matches_a_central_difference(sim):
    """d log_prior(theta(x)) / d x = dlp (1 - exp(-theta)) against (F(x + h) - F(x - h)) / 2h of the header's own value F.
    The bar is the quotient's own error: its truncation, estimated from the quotient alone as |D(h) - D(h / 2)| (the
    leading term c h^2 makes that difference 3/4 c h^2, three times D(h / 2)'s truncation c h^2 / 4), plus its rounding,
    twice 4 ulp of S over 2 (h / 2)."""
    row_priors = [PR.Gamma.from_EV(1.0, 10.0), PR.LogGaussian(0.3, 1.1), PR.Gaussian(1.5, 0.7), PR.InverseGamma(3.0, 2.0)]
    xs = np.array([[-3.0, -1.0, 0.5, 2.0], [0.0, 0.3, -0.7, 1.1], [4.0, 9.0, 20.0, 30.0], [-6.0, 2.5, 35.0, 0.1]])
    h = 1e-3
    for x in xs:
        theta = F.logexp_f(x)
        _, dlp = sim(row_priors, theta)
        analytic = dlp[0] * F.logexp_gradfactor(theta)
        for k in range(4):
            def D(step):
                xp, xm = x.copy(), x.copy()
                xp[k] += step
                xm[k] -= step
                lp, _ = sim(row_priors, np.array([F.logexp_f(xp), F.logexp_f(xm)]))
                return (lp[0] - lp[1]) / (2.0 * step)
            d1, d2 = D(h), D(h / 2.0)
            S = sum(float(abs_terms(p, t) + jac_terms(t)) for p, t in zip(row_priors, theta))
            bar = abs(d1 - d2) + 8.0 * ULP * S / h
            assert abs(analytic[k] - d2) <= bar, (x, k, analytic[k], d2, bar)


# ---- the restarts' draws -----------------------------------------------------------------------------------------------

def test_restart_draws_consume_the_generator_in_the_stated_order():
    priors = {"noise_var": PR.Gamma.from_EV(0.1, 1.0), "variance": PR.Gamma(2.0, 1.0), "lengthscale": PR.LogGaussian(0.0, 0.5)}
    P, n_ls = 5, 3
    np.random.seed(123)
    got = F.mle_restart_starts(P, 4, priors, True)
    after = np.random.rand()
    np.random.seed(123)
    want = []
    for _ in range(3):
        x = np.random.randn(P)
        x[0:1] = F.logexp_finv(np.random.gamma(shape=2.0, scale=1.0, size=1))
        x[1:1 + n_ls] = F.logexp_finv(np.exp(np.random.randn(n_ls) * 0.5 + 0.0))
        x[1 + n_ls:] = F.logexp_finv(np.random.gamma(shape=0.1 ** 2 / 1.0, scale=1.0 / (0.1 / 1.0), size=1))
        want.append(x)
    assert np.array_equal(got, np.array(want)) and after == np.random.rand() and got.shape == (3, P)
    assert np.all(np.isfinite(F.logexp_f(got))) and np.all(F.logexp_f(got) > 0.0)
    # a model whose noise is fixed: the last entry is a lengthscale, no noise draw
    np.random.seed(5)
    got = F.mle_restart_starts(3, 2, {"lengthscale": PR.LogGaussian(0.0, 0.5)}, False)
    np.random.seed(5)
    x = np.random.randn(3)
    x[1:3] = F.logexp_finv(np.exp(np.random.randn(2) * 0.5))
    assert np.array_equal(got, x[None])
    # a Gaussian prior may draw a value no parameter can take: the randn entry stays (the draw is consumed all the same)
    np.random.seed(7)
    got = F.mle_restart_starts(3, 6, {"variance": PR.Gaussian(-50.0, 1.0)}, True)
    after = np.random.rand()
    np.random.seed(7)
    rows = []
    for _ in range(5):
        rows.append(np.random.randn(3))
        assert np.random.randn(1) * 1.0 - 50.0 < 0.0
    assert np.array_equal(got, np.array(rows)) and after == np.random.rand()


def test_restart_draws_without_priors_are_todays():
    for priors in (None, {}):
        np.random.seed(99)
        got = F.mle_restart_starts(4, 5, priors)
        after = np.random.rand()
        np.random.seed(99)
        want = np.array([np.random.randn(4) for _ in range(4)])
        assert np.array_equal(got, want) and after == np.random.rand()
    np.random.seed(99)
    assert np.array_equal(F.mle_restart_starts(4, 5), want)
    state = np.random.get_state()[1].copy()
    assert F.mle_restart_starts(4, 1, {"variance": PR.Gamma(2.0, 1.0)}).shape == (0, 4)       # one start draws nothing
    assert np.array_equal(state, np.random.get_state()[1])


# ---- refusals without a device -----------------------------------------------------------------------------------------

def test_refusals_before_any_device_call():
    for make in (lambda: PR.Gaussian(0.0, 0.0), lambda: PR.Gaussian(0.0, -1.0), lambda: PR.LogGaussian(0.0, 0.0),
                 lambda: PR.Gamma(0.0, 1.0), lambda: PR.Gamma(-2.0, 1.0), lambda: PR.Gamma(1.0, 0.0),
                 lambda: PR.InverseGamma(0.0, 1.0), lambda: PR.InverseGamma(1.0, -3.0),
                 lambda: PR.Gaussian(float("nan"), 1.0), lambda: PR.LogGaussian(0.0, float("inf")),
                 lambda: PR.Gamma(float("nan"), 1.0), lambda: PR.InverseGamma(1.0, float("inf")),
                 lambda: PR.Gamma.from_EV(0.0, 1.0)):
        with pytest.raises(ValueError):
            make()
    # an unknown kind, an unknown parameter, a prior on a fixed noise
    unknown = PR.Prior()
    unknown.p0 = unknown.p1 = unknown.constant = 1.0
    unknown.kind = 9
    for bad in ({"variance": unknown}, {"variance": PR.Prior()}, {"variance": "Gamma"}, {"variance": None},
                {"period": PR.Gamma(1.0, 1.0)}):
        with pytest.raises(ValueError):
            PR.checked_priors(bad)
    with pytest.raises(ValueError, match="fixed"):
        PR.checked_priors({"noise_var": PR.Gamma(1.0, 1.0)}, fix_noise=True)
    assert list(PR.checked_priors({"noise_var": PR.Gamma(1.0, 1.0), "variance": PR.Gamma(2.0, 1.0)})) == ["variance", "noise_var"]
    assert PR.checked_priors(None) == {} and PR.per_parameter(None, 2) == [None] * 4
    # the agent's and the path's constructors check them before anything else touches a device
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    with pytest.raises(ValueError):
        CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, [["X"]], None, "min", [None], [None], [None], comm=None,
                           hyper_priors={"period": PR.Gamma(1.0, 1.0)})
    # transform="log" with priors: the objective, the optimiser's start and optimize_together refuse on the host
    m = SimpleNamespace(variance=1.0, lengthscale=np.ones(1), noise_var=0.1, fix_noise=False, small=True,
                        _priors={"variance": PR.Gamma(2.0, 1.0)})
    with pytest.raises(ValueError, match="logexp"):
        F.HipGaussianProcess._objective(m, np.zeros(3), "log")
    with pytest.raises(ValueError, match="logexp"):
        F._optimizer_start(m, "log")
    with pytest.raises(ValueError, match="logexp"):
        F.HipGaussianProcess.optimize(m, transform="log")
    with pytest.raises(ValueError, match="logexp"):
        F.optimize_together([m], transform="log")
    m._priors = {}
    assert F._optimizer_start(m, "log")[0].size == 3                                  # no priors: as before
    # the library itself: a NULL handle is refused without a device
    lib = _lib.load()
    assert lib.cbo_gp_set_priors(None, 3, None) == _lib.CBO_ERR_INVALID
    assert lib.cbo_gp_get_priors(None, 3, None) == _lib.CBO_ERR_INVALID
    assert lib.cbo_gp_log_prior_batch(0, None, None, None, None, None) == _lib.CBO_ERR_INVALID
