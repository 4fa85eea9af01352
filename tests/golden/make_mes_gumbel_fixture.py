"""Generates tests/golden/mes_gumbel_single.npz: what ``cbo_gp_mes_gumbel`` (the single-set Gumbel fit of max-value entropy
search) returned BEFORE its bisection kernel became the one-set case of the multi-set launch -- the three
quantiles, a and b of a few fitted models, as bit patterns to compare against (tests/test_sets_mes_gpu.py).  Needs an
MI355X and the library of the commit that precedes that change; run once, commit the .npz.

    python tests/golden/make_mes_gumbel_fixture.py [output.npz]

Every input the call read is stored next to its outputs (points, targets, hyper-parameters, the grid, the prior closures'
values at both), so the test rebuilds the models from the file alone.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

# n observations, grid points in all (the model's points on top), d, causal, ARD
CASES = [dict(n=50, m=113, d=2, causal=False, ard=False),
         dict(n=17, m=1024, d=1, causal=True, ard=False),
         dict(n=128, m=705, d=3, causal=False, ard=True),
         dict(n=1, m=65, d=2, causal=True, ard=False)]


def mean_f(a):
    return 0.3 * np.sin(a).sum(1, keepdims=True)


def var_f(a):
    return 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2


def inputs(case, index):
    n, m, d = case["n"], case["m"], case["d"]
    rng = np.random.default_rng(4242 + index)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))
    grid = np.vstack([X, rng.uniform(-2.5, 2.5, (m - n, d))])
    out = dict(X=X, y=y, grid=grid, variance=np.float64(1.3), noise_var=np.float64(1e-3),
               lengthscale=(0.7 + 0.2 * np.arange(d)) if case["ard"] else np.array([0.9]), ard=np.bool_(case["ard"]),
               causal=np.bool_(case["causal"]))
    if case["causal"]:
        out.update(mX=mean_f(X), vX=var_f(X), mG=mean_f(grid), vG=var_f(grid))
    return out


def model_of(inp):
    """The fitted model of one case from its stored inputs (prior closures as look-ups of the stored values)."""
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    ard = bool(inp["ard"])
    kw = dict(variance=float(inp["variance"]), lengthscale=np.asarray(inp["lengthscale"]) if ard else float(inp["lengthscale"][0]),
              ard=ard, noise_var=float(inp["noise_var"]))
    if bool(inp["causal"]):
        pts = np.vstack([inp["X"], inp["grid"]])
        lut_m = {tuple(r): v for r, v in zip(map(tuple, pts), np.vstack([inp["mX"], inp["mG"]])[:, 0])}
        lut_v = {tuple(r): v for r, v in zip(map(tuple, pts), np.vstack([inp["vX"], inp["vG"]])[:, 0])}
        kw["mean_function"] = lambda a: np.array([[lut_m[tuple(r)]] for r in a])
        kw["variance_adjustment"] = lambda a: np.array([[lut_v[tuple(r)]] for r in a])
    return HipGaussianProcess(inp["X"], inp["y"], **kw)


def single_fit(lib, model, inp):
    """cbo_gp_mes_gumbel on the case's grid: (quantiles (3,), a, b)."""
    grid = lib.as_f64(inp["grid"])
    causal = bool(inp["causal"])
    pm = lib.as_f64(inp["mG"]).reshape(-1) if causal else None
    pv = lib.as_f64(inp["vG"]).reshape(-1) if causal else None
    q = np.empty(3)
    a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
    model.ensure_fitted()
    lib.check(lib.load().cbo_gp_mes_gumbel(model._handle, grid.shape[0], lib.dptr(grid), lib.dptr(pm), lib.dptr(pv),
                                           lib.dptr(q), ctypes.byref(a), ctypes.byref(b), None, None))
    return q, a.value, b.value


def main():
    from cbo_with_oop_amd import _lib
    out = {"n_cases": np.int64(len(CASES))}
    for i, case in enumerate(CASES):
        inp = inputs(case, i)
        model = model_of(inp)
        q, a, b = single_fit(_lib, model, inp)
        model.close()
        for k, v in inp.items():
            out[f"c{i}_{k}"] = v
        out[f"c{i}_quantiles"], out[f"c{i}_a"], out[f"c{i}_b"] = q, np.float64(a), np.float64(b)
        print(f"case {i} {case}: quantiles {q.tolist()} a {a!r} b {b!r}")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mes_gumbel_single.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
