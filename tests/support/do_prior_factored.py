"""The factored do-calculus prior restated in numpy, for the tests: what cbo_do_prior_create snapshots from
an RBF graph GP and what do_prior_at evaluates, in plain linear algebra and without the device's summation orders.

    a_i(x) = exp(-1/2 sum_{c in I}     ((x_c  - X_g[i,c]) / l_c)^2)
    b_ri   = exp(-1/2 sum_{c not in I} ((O_rc - X_g[i,c]) / l_c)^2)
    m(x)   = sum_i w_i a_i(x),   w_i = sigma^2 alpha_i mean_r b_ri
    v(x)   = (sigma^2 + sigma_n^2) - a(x)^T M a(x),   M = sigma^4 (Ky^-1 o b^T b / N_obs)
"""
import numpy as np
import scipy.linalg


def factor(X_g, L, alpha, variance, lengthscale, noise_var, observed, intervened_index):
    """(w, M, vmax, columns, sources, lengthscales): ``L`` the lower Cholesky factor of Ky, ``alpha`` = Ky^-1 (y - m)."""
    X_g = np.asarray(X_g, dtype=np.float64)
    O = np.asarray(observed, dtype=np.float64)
    n, d = X_g.shape
    ls = np.broadcast_to(np.asarray(lengthscale, dtype=np.float64).reshape(-1), (d,)) if np.size(lengthscale) in (1, d) \
        else None
    idx = [int(v) for v in intervened_index]
    free = [c for c in range(d) if idx[c] < 0]
    cols = [c for c in range(d) if idx[c] >= 0]
    diff = (O[:, None, free] - X_g[None, :, free]) / ls[free]
    b = np.exp(-0.5 * np.sum(diff * diff, axis=2))                       # (N_obs, n)
    W = scipy.linalg.solve_triangular(L, np.eye(n), lower=True)
    Kinv = W.T @ W
    M = variance ** 2 * (Kinv * (b.T @ b / O.shape[0]))
    w = variance * np.asarray(alpha, dtype=np.float64).reshape(-1) * b.mean(axis=0)
    return w, M, variance + noise_var, cols, [idx[c] for c in cols], ls[cols]


def evaluate(X_g, factored, values):
    """(mean (M,), var (M,)) at the rows of ``values``."""
    w, M, vmax, cols, src, ls = factored
    X_g = np.asarray(X_g, dtype=np.float64)
    values = np.atleast_2d(np.asarray(values, dtype=np.float64))
    diff = (values[:, None, src] - X_g[None, :, cols]) / ls
    a = np.exp(-0.5 * np.sum(diff * diff, axis=2))                       # (M, n)
    return a @ w, vmax - np.einsum("mi,ij,mj->m", a, M, a)


def clip_ratio(n_g, variance, noise_var):
    """sn / (n_g sigma^2 + sn), sn = sigma_n^2 + 1e-8: the least latent variance over sigma^2 (every row at the point)."""
    sn = noise_var + 1e-8
    return sn / (n_g * variance + sn)
