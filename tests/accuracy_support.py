"""Decision helpers of the absolute-accuracy gates (tests/test_accuracy_gpu.py; their sharpness is shown on the CPU by
tests/test_accuracy_host.py).  Each one measures ONE stage of the device against the long-double restatements of
oracle/gp_linalg_ld.c on the device's own fp64 inputs, and against what an fp64 LAPACK / scipy computation of the same
stage achieves on the same inputs:

* ``check_factor``: backward error max |L L^T - Ky|_ij / sqrt(Ky_ii Ky_jj) over sampled rows, the device's factor
  against LAPACK's factor of the SAME exported Ky: dev <= 8 max(lapack, eps).  Backward error does not depend on the
  conditioning of Ky, so the gate stays sharp on ill-conditioned models.
* ``check_alpha``: the normwise residual ||Ky alpha - r|| / (||Ky|| ||alpha|| + ||r||) (formed in long double) of the
  device's alpha against cho_solve on LAPACK's factor: the same factor of 8.
* ``check_solves``: the sweep's substitution on the device's own L: max |var_dev - var_ld| / k** <= 8 max |var_scipy -
  var_ld| / k** + 4 eps sqrt(n), var_scipy from scipy's fp64 solve_triangular on that L, var_ld from solve_many; the
  mean the same way, normalised by max |y|.
* ``check_gradients``: conftest.assert_parity's rule on absolute errors: |hip - truth| <= 8 |fp64 oracle - truth| plus
  a floor of a few eps times the magnitude of the contraction (the sum of its terms in absolute value).

Every helper returns a dict of the measured numbers with ``ok``; tests ``assert r["ok"], r`` so that a failure shows them.
"""
import numpy as np
import scipy.linalg
from scipy.linalg import lapack

from oracle import truth as T

EPS = float(np.finfo(np.float64).eps)
SLACK = 8.0


def sample_rows(n, rng, n_random=32, max_boundaries=64):
    """Every panel boundary (128 k - 1 and 128 k; evenly thinned to about ``max_boundaries`` rows at large n), the
    first and the last row, and ``n_random`` random rows."""
    bounds = [r for k in range(1, (n - 1) // 128 + 1) for r in (128 * k - 1, 128 * k) if r < n]
    if len(bounds) > max_boundaries:
        keep = np.unique(np.linspace(0, len(bounds) // 2 - 1, max_boundaries // 2).round().astype(int))
        bounds = [bounds[2 * k + t] for k in keep for t in (0, 1)]
    rows = set(bounds) | {0, n - 1} | set(rng.choice(n, size=min(n, n_random), replace=False).tolist())
    return np.array(sorted(rows), dtype=np.int64)


def lapack_factor(A):
    """LAPACK's dpotrf of A (C order), factored in one copy: the lower triangle of the result holds L (the strict
    upper one is not cleaned; every reader here takes the lower triangle only)."""
    M = np.array(A, dtype=np.float64, order="C", copy=True)
    # M.T is Fortran-contiguous and equal to A: LAPACK's upper factor U of it (A = U^T U), in place, is L = U^T in the
    # lower triangle of the C-ordered M
    _, info = lapack.dpotrf(M.T, lower=0, clean=0, overwrite_a=1)
    if info != 0:
        raise np.linalg.LinAlgError(f"dpotrf info {info}")
    return M


def check_factor(L_dev, Ky, rows, L_ref=None):
    """Backward error of the device factor against LAPACK's of the same Ky (``L_ref`` if already computed)."""
    L_ref = lapack_factor(Ky) if L_ref is None else L_ref
    dev, where_dev = T.backward_error_rows(L_dev, Ky, rows)
    ref, where_ref = T.backward_error_rows(L_ref, Ky, rows)
    bound = SLACK * max(float(ref), EPS)
    return {"ok": bool(float(dev) <= bound), "dev": float(dev), "lapack": float(ref), "ratio": float(dev) / max(float(ref), EPS),
            "bound": bound, "at": where_dev, "lapack_at": where_ref, "rows": int(len(rows))}


def residual_norm(Ky, alpha, r, block=2048):
    """||Ky alpha - r||_2 / (||Ky||_F ||alpha||_2 + ||r||_2) with Ky alpha formed in long double."""
    a = np.asarray(alpha, dtype=np.float64).reshape(-1).astype(np.longdouble)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    res = np.empty(r.size, dtype=np.longdouble)
    for i in range(0, r.size, block):
        res[i:i + block] = Ky[i:i + block].astype(np.longdouble) @ a - r[i:i + block]
    den = np.linalg.norm(Ky) * np.linalg.norm(np.asarray(a, dtype=np.float64)) + np.linalg.norm(r)
    return float(np.sqrt(np.sum(res * res)) / den)


def check_alpha(alpha_dev, Ky, r, L_ref=None):
    """The device's alpha against cho_solve on LAPACK's factor, through the residual of Ky alpha = r."""
    L_ref = lapack_factor(Ky) if L_ref is None else L_ref
    alpha_ref = scipy.linalg.cho_solve((L_ref, True), np.asarray(r, dtype=np.float64).reshape(-1), check_finite=False)
    dev, ref = residual_norm(Ky, alpha_dev, r), residual_norm(Ky, alpha_ref, r)
    bound = SLACK * max(ref, EPS)
    return {"ok": bool(dev <= bound), "dev": dev, "lapack": ref, "ratio": dev / max(ref, EPS), "bound": bound}


def check_solves(L, Kx, r, kss, noise, var_dev, mean_dev, mXs=None, y_scale=1.0):
    """The sweep's substitution on the device's own factor ``L``: ``var_dev`` / ``mean_dev`` at the candidates whose
    cross-covariances are the columns of ``Kx`` (n, m), prior variances ``kss`` (m,), residual r = y - m(X)."""
    n = L.shape[0]
    Kx = np.ascontiguousarray(Kx, dtype=np.float64)
    kss = np.asarray(kss, dtype=np.float64).reshape(-1)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    off = 0.0 if mXs is None else np.asarray(mXs, dtype=np.float64).reshape(-1)
    q_ld, mu_ld = T.solve_many(L, Kx, r=r)
    var_ld = np.maximum(kss.astype(np.longdouble) - q_ld, np.longdouble(1e-15)) + np.longdouble(noise)
    mean_ld = mu_ld + off
    V = scipy.linalg.solve_triangular(L, Kx, lower=True, check_finite=False)
    z = scipy.linalg.solve_triangular(L, r, lower=True, check_finite=False)
    var_sc = np.clip(kss - np.sum(V * V, 0), 1e-15, None) + noise
    mean_sc = V.T @ z + off
    err = lambda a, ref, scale: float(np.max(np.abs(np.asarray(a, dtype=np.longdouble).reshape(-1) - ref) / scale))
    floor = 4 * EPS * np.sqrt(n)
    out = {"var_dev": err(var_dev, var_ld, kss), "var_scipy": err(var_sc, var_ld, kss),
           "mean_dev": err(mean_dev, mean_ld, y_scale), "mean_scipy": err(mean_sc, mean_ld, y_scale), "floor": floor}
    out["var_bound"] = SLACK * out["var_scipy"] + floor
    out["mean_bound"] = SLACK * out["mean_scipy"] + floor
    out["ok"] = bool(out["var_dev"] <= out["var_bound"] and out["mean_dev"] <= out["mean_bound"])
    return out


def check_gradients(hip, oracle, truth, mag, what, floor_eps=4.0):
    """|hip - truth| <= 8 |oracle - truth| + floor_eps * eps * mag, elementwise over the flattened arrays."""
    hip, oracle = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (hip, oracle))
    truth = np.asarray(truth, dtype=np.longdouble).reshape(-1)
    mag = np.asarray(mag, dtype=np.longdouble).reshape(-1)
    e_hip = np.asarray(np.abs(hip - truth), dtype=np.float64)
    e_orc = np.asarray(np.abs(oracle - truth), dtype=np.float64)
    floor = floor_eps * EPS * np.asarray(mag, dtype=np.float64)
    bound = SLACK * e_orc + floor
    scale = np.maximum(np.asarray(mag, dtype=np.float64), 1e-300)
    worst = int(np.argmax(e_hip / np.maximum(bound, 1e-300)))
    return {"ok": bool(np.all(e_hip <= bound)), "what": what, "hip_err": float(e_hip[worst] / scale[worst]),
            "oracle_err": float(e_orc[worst] / scale[worst]), "bound": float(bound[worst] / scale[worst]),
            "ratio": float(np.max(e_hip / np.maximum(e_orc, EPS * scale))), "index": worst}
