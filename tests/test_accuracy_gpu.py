"""Absolute accuracy of the fp64 fit and sweep, one device stage at a time, against long-double restatements on the
device's OWN fp64 inputs (oracle/gp_linalg_ld.c through tests/accuracy_support.py):

  a. the factor by size class: backward error max |L L^T - Ky|_ij / sqrt(Ky_ii Ky_jj) over sampled rows, against LAPACK's
     factor of the same exported Ky (<= 8 x), alpha through the residual of Ky alpha = r (<= 8 x cho_solve's), the
     jitter ladder's level against the oracle's;
  b. the same criterion at the conditioning and hyper-parameter edges (1e-10 noise with duplicated rows, a forced
     ladder, lengthscales 1e-3 and 50, variances 1e-6 and 1e6, ARD over 100x, the causal term, coordinates at 2475);
  c. the factor grown by ``append`` against the grown data's Ky (accumulated drift);
  d. the sweep's substitution (q = sum V^2, mu = V^T z) on the device's own L, sampled candidates at strip and chunk edges;
  e. the likelihood and its gradients (one-workgroup, two-block and general paths) and f. the prediction gradients:
     |HIP - truth| <= 8 |fp64 oracle on the same L - truth| + 4 eps x (the contraction's magnitude);
  g. K(X, X) assembly across tiles, d = 1 .. 8, at the golden test's 1e-12 relative.

The same-bits tests of tests/test_parity_gpu.py pin every launch form and schedule to each other; these pin the shared
device functions (register Cholesky, diagonal inverses, panel TRSM, MFMA update, strip/pair substitution) to the maths.

Sizes of (a), against launch_cholesky (kernels_chol.hip; n_pad = round_up(n, 128), pairs of 128-row panels, a group of
G pairs opens while n3_pair - 512 (G = 4: - 1024) >= 6144 (G = 4: and >= 10240) rows lie below it, a pair's bulk update
takes the GEMM form while n3 - 256 >= 6144):
  1, 2, 16, 17, 127, 128        one panel (the lone diagonal block)
  129, 255, 256                 one pair, no bulk update
  257, 383                      a pair and a lone last panel (383: three panels, odd)
  640, 1025, 2049, 4097         plain pairs with bulk updates on the side stream, 1025 / 2049 / 4097 odd panel counts
  7169                          n_pad 7296, 57 panels: one group of two pairs (r0 = 0: 7040 - 512 >= 6144), one GEMM-form
                                pair (r0 = 512: 6528 - 512 < 6144 opens no group, 6528 - 256 >= 6144), plain pairs, a lone
                                last panel; 127 padding rows.  Any n in 7169 .. 7296 does this; 6913 (n_pad 7040) and
                                7297 (n_pad 7424: two groups, then 6144 - 256 < 6144) have no GEMM-form pair
  11521                         n_pad 11648, 91 panels: a group of four, eight groups of two, plain pairs, a lone last panel

Measured on an MI355X (each test prints a MEASURED line under -s).  Factor: dev / LAPACK backward error; alpha: dev /
cho_solve residual; sweep: dev / scipy error against the long-double substitution; gradients: |HIP - truth| over
max(|oracle - truth|, eps x magnitude), largest over the outputs of a case:
  factor   n <= 128          ratio 0.46 - 4.24 (n = 127: 1.13e-15 against 2.67e-16)     alpha 0.10 - 0.18
           129 - 383         1.09 - 3.01                                                 0.09 - 0.20
           640 - 4097        0.72 - 1.01 (backward errors 1.1e-15 - 1.4e-15)             0.04 - 0.08
           7169, 11521       1.23, 1.14 (2.2e-15, 2.1e-15)                               0.03, 0.02
  edges    1025 / 4097       lengthscale 50: 2.75 / 2.47; ARD d = 8: 1.78 / 1.95; the others 0.11 - 0.93;
                             ladder with duplicates: one jitter step, 0.78 / 0.79; alpha <= 0.07
  grown    130 + 126, 1100 + 20: <= 1.45 against the device-assembled Ky of the grown data
  sweep    var dev 1.0e-14 - 1.8e-14 of k** against scipy's 6e-16 - 4e-15 (3 - 17x: the floor 4 eps sqrt(n) carries it);
           mean dev / max|y| 3e-15 - 1.6e-13 against 8e-16 - 5e-14 (at most 4x)
  lml      every path, scalar / ARD / causal: <= 1.72
  dmean    <= 1.23
  dvar     8.4 - 17.3, at every n from 150 to 4097: the device forms W = L^-T (L^-1 k*) with two strip TRSMs that multiply
           by explicit inverses of the 16 x 16 diagonal blocks (invDt, and invT of the reversed factor); LAPACK's dpotrs
           substitutes.  The error does not grow with n or with cond(Ky), so it is that algorithm's, not a defect; dvar
           is held to 8 x the oracle's error plus 32 eps of its magnitude instead of 4.  The sweep's var carries the same
           3 - 17x against scipy, inside its floor.
  Kxx      worst relative entry error 5.7e-14 (bound 1e-12)
The whole module takes about 30 s on an MI355X with 16 CPU cores for the reference work.
"""
import os
import warnings

import numpy as np
import pytest
import scipy.linalg

from accuracy_support import (EPS, check_alpha, check_factor, check_gradients, check_solves, lapack_factor,
                              sample_rows)
from oracle import gp_oracle as O
from oracle import truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def _model(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def _mean_fn(a):
    return 0.3 * np.sin(a[:, :1]) + 0.1 * a[:, -1:]


def _var_adj(a):
    return 0.2 + 0.1 * np.cos(a[:, :1]) ** 2


CAUSAL = dict(mean_function=_mean_fn, variance_adjustment=_var_adj)


def _data(n, d, seed, box=5.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-box, box, (n, d))
    y = (np.sin(X[:, :1]) + 0.5 * np.cos(X[:, -1:]) + 0.05 * rng.standard_normal((n, 1)))
    return X, y


def _residual(m):
    r = m.Y[:, 0].copy()
    if m.causal:
        r -= _mean_fn(m.X)[:, 0]
    return r


def _gate_factor(m, seed, max_boundaries=64):
    """check_factor and check_alpha of a fitted model against LAPACK on the exported Ky (+ the ladder's jitter)."""
    n = m.X.shape[0]
    L, alpha = m.posterior_state()
    Ky = m.assembled_Ky()
    Ky[np.diag_indices(n)] += m.jitter
    rows = sample_rows(n, np.random.default_rng(seed), max_boundaries=max_boundaries)
    L_ref = lapack_factor(Ky)
    f = check_factor(L, Ky, rows, L_ref)
    a = check_alpha(alpha, Ky, _residual(m), L_ref)
    return f, a


# ------------------------------------------------------------------------------------------ a. factor by size class
FACTOR_SIZES = [1, 2, 16, 17, 127, 128, 129, 255, 256, 257, 383, 640, 1025, 2049, 4097, 7169, 11521]


@pytest.mark.parametrize("n", FACTOR_SIZES)
def test_factor_backward_error_by_size_class(hip, n):
    X, y = _data(n, 3, seed=n)
    m = _model(X, y, noise_var=1e-2)
    f, a = _gate_factor(m, seed=n)
    print(f"\nMEASURED factor n={n}: dev {f['dev']:.2e} lapack {f['lapack']:.2e} ratio {f['ratio']:.2f}; "
          f"alpha residual {a['dev']:.2e} / {a['lapack']:.2e} ratio {a['ratio']:.2f}")
    assert f["ok"], f
    assert a["ok"], a
    Ky = O.causal_K(X, X, None, None, 1.0, 1.0, zero_diag=True)
    Ky[np.diag_indices(n)] += 1e-2 + O.GPY_DIAG_JITTER
    assert m.jitter_tries == O.jitchol(Ky)[2]
    m.close()


# ------------------------------------------------------------------------------ b. conditioning and hyper edges
EDGES = {
    "noise_1e-10_duplicates": dict(kw=dict(noise_var=1e-10), dup=True),
    # The reference's 1e-10 noise with duplicated rows factors at level 0 here (measured: no retry at 1025 or 4097, the
    # 1.01e-8 diagonal add keeps Ky positive definite).  A negative noise variance, which no caller passes, makes the
    # diagonal add -1e-9, so level 0 must fail and the gate sees a factor from the jitchol ladder (as the golden
    # fixture jitter_ladder does).
    "ladder_duplicates": dict(kw=dict(noise_var=-1.1e-8), dup=True),
    "lengthscale_1e-3": dict(kw=dict(noise_var=1e-10, lengthscale=1e-3)),
    "lengthscale_50": dict(kw=dict(noise_var=1e-10, lengthscale=50.0)),
    "variance_1e-6": dict(kw=dict(noise_var=1e-10, variance=1e-6)),
    "variance_1e6": dict(kw=dict(noise_var=1e-10, variance=1e6)),
    "ard_d8_100x": dict(kw=dict(noise_var=1e-10, ard=True, lengthscale=np.geomspace(0.3, 30.0, 8)), d=8),
    "causal": dict(kw=dict(noise_var=1e-10, **CAUSAL)),
    "offset_2475": dict(kw=dict(noise_var=1e-4), offset=2475.0),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("n", [1025, 4097])
def test_factor_backward_error_at_the_edges(hip, n, edge):
    e = EDGES[edge]
    X, y = _data(n, e.get("d", 3), seed=n + 7)
    if e.get("dup"):
        X[n - n // 8:] = X[:n // 8]                      # an eighth of the rows twice
    X[:, 0] += e.get("offset", 0.0)
    m = _model(X, y, **e["kw"])
    if edge == "ladder_duplicates":
        assert m.jitter_tries >= 1
    f, a = _gate_factor(m, seed=n)
    print(f"\nMEASURED edge {edge} n={n}: tries {m.jitter_tries} dev {f['dev']:.2e} lapack {f['lapack']:.2e} "
          f"ratio {f['ratio']:.2f}; alpha ratio {a['ratio']:.2f}")
    assert f["ok"], (edge, f)
    assert a["ok"], (edge, a)
    m.close()


# ------------------------------------------------------------------------------------------ c. the grown factor
@pytest.mark.parametrize("n0,steps", [(130, 126), (1100, 20)])
def test_grown_factor_against_the_grown_data(hip, n0, steps):
    """n0 = 130: 126 appends one at a time, across 16-row tiles, up to the 256-row padding; the backward error of the
    factor against the Ky of the grown data every 16 appends and at the end."""
    rng = np.random.default_rng(n0)
    X, y = _data(n0 + steps, 2, seed=n0)
    m = _model(X[:n0], y[:n0], noise_var=1e-4)
    worst = 0.0
    for k in range(n0, n0 + steps):
        assert m.append(X[k], y[k]), k                   # no jitter, padded size not exhausted: the shortcut applies
        grown = k + 1 - n0
        if grown % 16 == 0 or k == n0 + steps - 1:
            n = k + 1
            L, alpha = m.posterior_state()
            # the Ky of the grown resident data as the device assembles it: the host's GPy-form entries differ from it
            # by eps (|x|^2 + |x'|^2) (7e-15 here, measured), which test_kxx_assembly_across_tiles gates on its own
            Ky = m.assembled_Ky()
            host = O.causal_K(X[:n], X[:n], None, None, 1.0, 1.0, zero_diag=True)
            host[np.diag_indices(n)] += 1e-4 + O.GPY_DIAG_JITTER
            assert np.max(np.abs(Ky - host) / np.abs(host).clip(1e-300)) < 1e-12
            rows = np.union1d(sample_rows(n, rng), np.arange(n0, n))
            L_ref = lapack_factor(Ky)
            f = check_factor(L, Ky, rows, L_ref)
            a = check_alpha(alpha, Ky, y[:n, 0], L_ref)
            assert f["ok"], (n, f)
            assert a["ok"], (n, a)
            worst = max(worst, f["ratio"])
    print(f"\nMEASURED grown n0={n0} +{steps}: worst ratio {worst:.2f}")
    m.close()


# -------------------------------------------------------------------------------------------- d. sweep solves
def _sweep_columns(m_cands, rng, chunk=None, total=256):
    """Strip edges (64-column strips) thinned evenly, the last columns, chunk edges, random ones: about ``total``."""
    edges = [c for s in range(0, m_cands, 64) for c in (s, s + 63) if c < m_cands]
    if len(edges) > total // 2:
        edges = [edges[i] for i in np.unique(np.linspace(0, len(edges) - 1, total // 2).round().astype(int))]
    cols = set(edges) | {m_cands - 2, m_cands - 1}
    if chunk:
        cols |= {c for s in range(chunk, m_cands, chunk) for c in (s - 1, s)}
    extra = max(0, total - len(cols))
    cols |= set(rng.choice(m_cands, size=min(extra, m_cands), replace=False).tolist())
    return np.array(sorted(c for c in cols if 0 <= c < m_cands))


@pytest.mark.parametrize("n,m_cands,causal,ws_mb", [(129, 700, False, None), (1025, 2000, False, 4),
                                                    (1025, 1337, True, None), (4097, 16384 + 37, False, None),
                                                    (7169, 4096 + 13, False, None)])
def test_sweep_solves_on_the_device_factor(hip, monkeypatch, n, m_cands, causal, ws_mb):
    """The default schedule only: the same-bits tests of test_parity_gpu.py carry this bound to the other schedules
    (left- / right-looking / overlapped, pipe groups, workspace chunking).  ``ws_mb``: a context whose V workspace holds
    ws_mb MiB, so that the candidates run in several chunks (their edges are sampled)."""
    from cbo_with_oop_amd import CausalExpectedImprovement, _lib
    ctx, chunk = None, None
    if ws_mb:
        monkeypatch.setenv("CBO_HIP_WORKSPACE_MB", str(ws_mb))
        ctx = _lib.Context(0)
        n_pad = -(-n // 128) * 128
        chunk = (ws_mb << 20) // (8 * n_pad) // 64 * 64
    try:
        rng = np.random.default_rng(n + m_cands)
        X, y = _data(n, 3, seed=n + 1)
        Xs = rng.uniform(-5.5, 5.5, (m_cands, 3))
        kw = dict(noise_var=1e-2, lengthscale=1.2, **(CAUSAL if causal else {}))
        if ctx is not None:
            kw["context"] = ctx
        m = _model(X, y, **kw)
        res = CausalExpectedImprovement(float(y.min()), "min", m).sweep(Xs, cost=1.0, want_posterior=True)
        L, _ = m.posterior_state()
        r = _residual(m)
        m.close()
    finally:
        if ctx is not None:
            ctx.close()
    cols = _sweep_columns(m_cands, rng, chunk)
    Xc = Xs[cols]
    vX, vXs = (_var_adj(X)[:, 0], _var_adj(Xc)[:, 0]) if causal else (None, None)
    Kx = O.causal_K(X, Xc, vX, vXs, 1.0, 1.2)
    kss = 1.0 + (vXs if causal else 0.0)
    s = check_solves(L, Kx, r, kss * np.ones(len(cols)), 1e-2, res["var"][cols, 0], res["mean"][cols, 0],
                     mXs=_mean_fn(Xc)[:, 0] if causal else None, y_scale=float(np.max(np.abs(y))))
    print(f"\nMEASURED sweep n={n} m={m_cands}: var dev {s['var_dev']:.2e} scipy {s['var_scipy']:.2e}; "
          f"mean dev {s['mean_dev']:.2e} scipy {s['mean_scipy']:.2e} (floor {s['floor']:.1e})")
    assert s["ok"], s


# ------------------------------------------------------------------------------ e. likelihood and its gradients
def _oracle_on(L, m, X, ls, vX):
    """gp_oracle's fp64 gradients with the given factor (dpotrs / dpotri on it)."""
    r = _residual(m)[:, None]
    alpha = scipy.linalg.lapack.dpotrs(L, r, lower=1)[0]
    post = O.Posterior(X, m.Y, None if vX is None else _mean_fn(X), vX, m.variance, ls, m.noise_var, L, alpha, 0.0, 0, False)
    return post


def _grad_case(n, d, kind, seed):
    X, y = _data(n, d, seed=seed, box=3.0)
    kw = dict(noise_var=1e-3, variance=1.4)
    if kind == "ard":
        kw.update(ard=True, lengthscale=np.linspace(0.8, 2.0, d))
    else:
        kw.update(lengthscale=1.1)
    if kind == "causal":
        kw.update(CAUSAL)
    return X, y, kw


@pytest.mark.parametrize("kind", ["scalar", "ard", "causal"])
@pytest.mark.parametrize("n", [17, 128, 129, 256, 1023, 1025, 2049])
def test_likelihood_gradients_against_long_double(hip, n, kind):
    """n <= 128: the one-workgroup kernel, also through lml_gradients_batch; 129 / 256: the two-block form; above: the
    general path (right-looking inverse).  The fp64 oracle and the truth both use the device's fitted factor."""
    from cbo_with_oop_amd.GaussianProcessFactory import lml_gradients_batch
    d = 3
    X, y, kw = _grad_case(n, d, kind, seed=n)
    m = _model(X, y, **kw)
    dv, dls, dn = m.log_likelihood_gradients()
    lml = m._last_lml
    L, _ = m.posterior_state()
    ls = m.lengthscale if kind == "ard" else float(m.lengthscale[0])
    vX = _var_adj(X)[:, 0] if kind == "causal" else None
    truth, mag = T.lml_and_gradients(L, X, y, _mean_fn(X) if vX is not None else None, vX, m.variance, ls)
    post = _oracle_on(L, m, X, ls, vX)
    o_dv, o_dls, o_dn = O.log_marginal_likelihood_gradients(post)
    o_lml = O.log_marginal_likelihood(post)
    vec = lambda a, b, c, dd: np.concatenate([[a, b, c], np.atleast_1d(np.asarray(dd, dtype=np.longdouble))])
    tv = vec(truth["lml"], truth["d_variance"], truth["d_noise"], truth["d_lengthscale"])
    mv = vec(mag["lml"], mag["d_variance"], mag["d_noise"], mag["d_lengthscale"])
    ov = np.concatenate([[o_lml, o_dv, o_dn], np.atleast_1d(o_dls)])
    g = check_gradients(np.concatenate([[lml, dv, dn], dls]), ov, tv, mv, f"lml gradients n={n} {kind}")
    print(f"\nMEASURED lml n={n} {kind}: hip {g['hip_err']:.2e} oracle {g['oracle_err']:.2e} ratio {g['ratio']:.2f}")
    assert g["ok"], g
    if n <= 256:
        other = _model(*_grad_case(n, d, kind, seed=n + 1)[:2], **kw)
        out = lml_gradients_batch([other, m])
        b_lml, b_dv, b_dls, b_dn = out[1]
        gb = check_gradients(np.concatenate([[b_lml, b_dv, b_dn], b_dls]), ov, tv, mv, f"batched n={n} {kind}")
        assert gb["ok"], gb
        other.close()
    m.close()


# -------------------------------------------------------------------------------- f. prediction gradients
@pytest.mark.parametrize("kind", ["scalar", "ard", "causal"])
@pytest.mark.parametrize("n", [150, 1025, 4097])
def test_prediction_gradients_against_long_double(hip, n, kind):
    d = 3
    X, y, kw = _grad_case(n, d, kind, seed=2 * n)
    m = _model(X, y, **kw)
    rng = np.random.default_rng(n)
    Xs = np.vstack([rng.uniform(-3.3, 3.3, (40, d)), X[:8] + 1e-3 * rng.standard_normal((8, d))])
    dmean, dvar = m.get_prediction_gradients(Xs)
    L, alpha = m.posterior_state()
    ls = m.lengthscale if kind == "ard" else float(m.lengthscale[0])
    vX, vXs = (_var_adj(X)[:, 0], _var_adj(Xs)[:, 0]) if kind == "causal" else (None, None)
    t_mean, t_var, mag_mean, mag_var = T.prediction_gradients(L, alpha, X, Xs, vX, vXs, m.variance, ls)
    post = O.Posterior(X, m.Y, None, vX, m.variance, ls, m.noise_var, L, alpha, 0.0, 0, False)
    o_mean, o_var = O.predict_gradients(post, Xs, vXs)
    gm = check_gradients(dmean, o_mean, t_mean, mag_mean, f"dmean n={n} {kind}")
    # dvar: floor 32 eps, not 4 (see the module docstring: the device's W = L^-T L^-1 k* multiplies by explicit 16 x 16
    # diagonal-block inverses, measured 8 - 17 eps of the magnitude at every size, where LAPACK's dpotrs substitutes)
    gv = check_gradients(dvar, o_var, t_var, mag_var, f"dvar n={n} {kind}", floor_eps=32.0)
    print(f"\nMEASURED pred grads n={n} {kind}: dmean ratio {gm['ratio']:.2f} dvar ratio {gv['ratio']:.2f} "
          f"(hip {gv['hip_err']:.2e} oracle {gv['oracle_err']:.2e})")
    assert gm["ok"], gm
    assert gv["ok"], gv
    m.close()


# ---------------------------------------------------------------------------------- g. K(X, X) across tiles
@pytest.mark.parametrize("variant", ["scalar", "ard", "causal"])
@pytest.mark.parametrize("n", [65, 129, 1000, 4097])
def test_kxx_assembly_across_tiles(hip, n, variant):
    worst = 0.0
    dims = range(1, 9) if variant != "causal" else (1, 4, 8)
    for d in dims:
        rng = np.random.default_rng(n * 10 + d)
        X = rng.uniform(-3, 3, (n, d))
        y = rng.standard_normal((n, 1))
        ls = rng.uniform(0.5, 2.0, d) if variant == "ard" else 0.8
        kw = dict(noise_var=1e-3, variance=1.7, lengthscale=ls, ard=variant == "ard", fit=False,
                  **(CAUSAL if variant == "causal" else {}))
        m = _model(X, y, **kw)
        K = m.assembled_Ky()
        vX = _var_adj(X) if variant == "causal" else None
        Kref = O.causal_K(X, X, vX, vX, 1.7, ls, zero_diag=variant != "causal")
        Kref[np.diag_indices(n)] += 1e-3 + O.GPY_DIAG_JITTER
        assert np.array_equal(K, K.T), d
        err = float(np.max(np.abs(K - Kref) / np.abs(Kref).clip(1e-300)))
        assert err < 1e-12, (n, d, variant, err)
        worst = max(worst, err)
        m.close()
    print(f"\nMEASURED kxx n={n} {variant}: worst rel {worst:.2e}")
