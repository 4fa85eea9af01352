"""Zero-extension of a two-dimensional problem into D columns (tests/test_dims_host.py, tests/test_dims_gpu.py).

A problem with two live coordinates, placed at columns i < j of a D-column problem whose other columns are exact zeros
(training points, candidates and every other point set alike), is the same problem: every device path adds the dummy
coordinates' products or squared differences, which are exact zeros, to the live terms in a sequential chain, so each
output keeps the base problem's bits whatever (positive) lengthscale the dummy columns carry.  Two live coordinates and
not three, because squared_norm (cbo_device.h) sums a row's squares in a chain for D < 8 and by an 8-way pairwise tree at
D = 8: three non-zero squares would associate differently there.  With two, only the tree's fused pairs matter (see
BIT_EMBEDDINGS below).  DESIGN.md §2.
"""
import numpy as np

VARIANCE = 1.3
NOISE_VAR = 1e-2
LS_ISO = 0.9
LS_ARD = np.array([0.9, 1.4])
VARIANTS = ("iso", "ard", "causal")
DIMS = (3, 4, 5, 6, 7, 8)


def embed(A, D, pos):
    """(rows, 2) -> (rows, D): the two columns at ``pos``, exact zeros elsewhere."""
    A = np.asarray(A, dtype=np.float64)
    assert A.ndim == 2 and A.shape[1] == 2 and 0 <= pos[0] < pos[1] < D
    out = np.zeros((A.shape[0], D))
    out[:, pos[0]] = A[:, 0]
    out[:, pos[1]] = A[:, 1]
    return out


def embed_lengthscales(ls2, D, pos):
    """The live lengthscales at ``pos``, 0.7 + 0.1 k in every dummy column k."""
    ls2 = np.asarray(ls2, dtype=np.float64).reshape(2)
    out = 0.7 + 0.1 * np.arange(D)
    out[pos[0]], out[pos[1]] = ls2
    return out


def placements(D):
    """The anti-diagonal pairs (0, D-1), (1, D-2), ...; for odd D also (0, (D-1)/2), which makes the middle slot live.
    Every slot of every D is live at least once and the first live slot is sometimes 0 and sometimes not."""
    if D == 3:
        return [(0, 2), (1, 2), (0, 1)]
    out = [(i, D - 1 - i) for i in range(D // 2)]
    if D % 2:
        out.append((0, (D - 1) // 2))
    return out


def adjacent_placements(D):
    """(0, 1), (2, 3), ...: the pairs that squared_norm's tree at D = 8 (cbo_device.h) fuses."""
    return [(i, i + 1) for i in range(0, D - 1, 2)]


EMBEDDINGS = [(D, pos) for D in DIMS for pos in placements(D)]
# The one summation over k that is no sequential chain is squared_norm at D = 8: numpy's 8-way pairwise tree over the pairs
# fma(x1, x1, rn(x0^2)), fma(x3, x3, rn(x2^2)), ... (cbo_device.h), where the two-column problem has fma(b, b, rn(a^2)).  Two
# live coordinates keep the base problem's bits there in the adjacent slots (2k, 2k + 1) -- the prefix (0, 1) among them,
# every slot live once -- and in slots of two different pairs they give rn(rn(a^2) + rn(b^2)) whichever pairs: the
# anti-diagonal placements of D = 8 keep ONE set of bits among themselves.  So the base problem's bits are asked of
# BIT_EMBEDDINGS, and of TREE_EMBEDDINGS the bits of their first, which is itself held to the oracle.
BIT_EMBEDDINGS = [(D, pos) for D, pos in EMBEDDINGS if D < 8] + [(8, pos) for pos in adjacent_placements(8)]
TREE_EMBEDDINGS = [(8, pos) for pos in placements(8)]


def embedding_id(e):
    return f"D{e[0]}-{e[1][0]}{e[1][1]}"


def dummies(D, pos):
    return [k for k in range(D) if k not in pos]


def prior_mean(a):
    """The closed-form causal prior mean of tests/test_pointwise_gpu.py on the two live coordinates."""
    return 0.3 * (np.sin(a[:, :1]) + np.sin(a[:, 1:2]))


def prior_var(a):
    return 0.05 + 0.02 * (np.cos(a[:, :1]) + np.cos(a[:, 1:2])) ** 2


def lifted(fn, pos):
    """``fn`` of the two live columns of a D-column array: the prior is per point, the same bits for every embedding."""
    return lambda a: fn(np.ascontiguousarray(a[:, list(pos)]))


def base_problem(n, m, seed, variant):
    """X (n, 2), y (n, 1), Xs (m, 2) and the hyper-parameters of ``variant``; for ``causal`` also the prior functions."""
    assert variant in VARIANTS
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, 2))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.0, 2.0, (m, 2))
    p = dict(X=X, y=y, Xs=Xs, variant=variant, variance=VARIANCE, noise_var=NOISE_VAR, ard=variant != "iso",
             lengthscale=LS_ISO if variant == "iso" else LS_ARD.copy(), causal=variant == "causal")
    return p


def hip_kwargs(p, D=2, pos=(0, 1)):
    """HipGaussianProcess keyword arguments of the base problem (D = 2) or of its embedding."""
    ls = p["lengthscale"]
    if p["ard"] and D > 2:
        ls = embed_lengthscales(ls, D, pos)
    kw = dict(variance=p["variance"], lengthscale=ls, ard=p["ard"], noise_var=p["noise_var"])
    if p["causal"]:
        kw.update(mean_function=lifted(prior_mean, pos), variance_adjustment=lifted(prior_var, pos))
    return kw


def oracle_hyper(p, D=2, pos=(0, 1)):
    """The hyper-parameters of the same as oracle.gp_oracle.fit takes them."""
    ls = p["lengthscale"]
    if p["ard"] and D > 2:
        ls = embed_lengthscales(ls, D, pos)
    return dict(variance=p["variance"], lengthscale=ls, noise_var=p["noise_var"])


def oracle_kwargs(p, D=2, pos=(0, 1)):
    """oracle.gp_oracle.fit keyword arguments of the same: the hyper-parameters and, for ``causal``, the prior at X."""
    kw = oracle_hyper(p, D, pos)
    if p["causal"]:
        kw.update(mX=prior_mean(p["X"]), vX=prior_var(p["X"]))
    return kw


def oracle_priors(p, pts2):
    """(mXs, vXs) keyword values for the oracle at the two-column points ``pts2`` (None, None unless causal)."""
    return (prior_mean(pts2), prior_var(pts2)) if p["causal"] else (None, None)


def condition_bound(n, variance=VARIANCE, noise_var=NOISE_VAR, max_prior_var=0.0):
    """cond(Ky) <= n (variance + max v) / noise_var + 1: Ky's largest eigenvalue is at most its largest row sum,
    n (variance + max v) + noise_var, and its smallest at least noise_var.  A condition, not a measurement."""
    return n * (variance + max_prior_var) / noise_var + 1.0


def dense_problem(n, m, D, seed):
    """All D coordinates live: data uniform on [-2, 2]^D, ARD lengthscales sqrt(D) linspace(0.8, 1.2, D) (off-diagonal
    kernel values stay of order 0.1), variance 1.3, noise 1e-2."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, D))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.0, 2.0, (m, D))
    return dict(X=X, y=y, Xs=Xs, variance=VARIANCE, noise_var=NOISE_VAR, lengthscale=np.sqrt(D) * np.linspace(0.8, 1.2, D))
