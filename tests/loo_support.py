"""Leave-one-out cross-validation on the host, for the tests of cbo_gp_loo / cbo_gp_loo_batch: a numpy restatement of the
closed form (Rasmussen & Williams 5.4.2) and a brute-force version, n refits on n - 1 points.  Both start from the
oracle's kernel matrix (oracle/gp_oracle.py: GPy's operation order, the causal term, the zero-distance rule of the plain
RBF) and the prior mean, and both predict the left-out OBSERVATION: the noise and the 1e-8 GPy adds to the diagonal of Ky
are part of the predictive variance."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import gp_oracle as O

LOG_2PI = float(np.log(2.0 * np.pi))
FIXTURE_NAMES = ("graph_ard_d4", "coral_max_d3", "causal_d2", "toy_bo_d2")


def ky_and_residual(X, y, mX=None, vX=None, variance=1.0, lengthscale=1.0, noise_var=1e-10, jitter=0.0):
    """(Ky, r, y): Ky = K + (noise + 1e-8 + jitter) I as oracle.fit assembles it, r = y - m(X)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Ky = O.causal_K(X, X, vX, vX, variance, lengthscale, vX is None).copy()
    Ky[np.diag_indices_from(Ky)] += noise_var + O.GPY_DIAG_JITTER + jitter
    r = y if mX is None else y - np.asarray(mX, dtype=np.float64).reshape(-1)
    return Ky, r, y


def closed_form(Ky, r, y):
    """(mean, var, lpd), each (n,): c = diag(Ky^-1) and alpha = Ky^-1 r from one Cholesky factor."""
    cf = cho_factor(Ky, lower=True)
    c = np.diag(cho_solve(cf, np.eye(Ky.shape[0])))
    alpha = cho_solve(cf, r)
    return y - alpha / c, 1.0 / c, -0.5 * LOG_2PI + 0.5 * np.log(c) - 0.5 * alpha ** 2 / c


def brute_force(Ky, r, y):
    """The same three vectors from n models on n - 1 points each: the Gaussian predictive density of y_i given the rest."""
    n = Ky.shape[0]
    mean, var = np.zeros(n), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        k = Ky[keep, i]
        if n > 1:
            cf = cho_factor(Ky[np.ix_(keep, keep)], lower=True)
            mean[i] = (y[i] - r[i]) + k @ cho_solve(cf, r[keep])
            var[i] = Ky[i, i] - k @ cho_solve(cf, k)
        else:
            mean[i], var[i] = y[i] - r[i], Ky[i, i]
    return mean, var, -0.5 * LOG_2PI - 0.5 * np.log(var) - 0.5 * (y - mean) ** 2 / var


def gap(a, b, y):
    """The largest gap between two (mean, var, lpd) triples: mean relative to the scale of |y|, var relative, lpd absolute."""
    scale = max(float(np.max(np.abs(y))), 1e-300)
    return max(float(np.max(np.abs(a[0] - b[0]))) / scale, float(np.max(np.abs(a[1] - b[1]) / np.abs(b[1]))),
               float(np.max(np.abs(a[2] - b[2]))))


def fixture_system(f, rows=None):
    """Ky, r, y of a golden fixture (tests/conftest.py load_fixture), of its first `rows` observations when given."""
    s = slice(None) if rows is None else slice(0, rows)
    mX = None if f["mX"] is None else f["mX"][s]
    vX = None if f["vX"] is None else f["vX"][s]
    return ky_and_residual(f["X"][s], f["y"][s], mX, vX, float(f["variance"]), f["lengthscale_arg"], float(f["noise_var"]))


def synthetic(n, d=2, seed=0):
    """Well-conditioned data of the general-path tests: noise 1e-2, unit variance and lengthscale."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3.0, 3.0, (n, d))
    y = np.sin(X[:, :1]) + 0.3 * np.cos(2.0 * X[:, -1:]) + 0.1 * rng.standard_normal((n, 1))
    return X, y


SYNTHETIC_NOISE = 1e-2
