"""GPU tests of the constrained acquisition (cbo_acq_sweep_constrained: constrained_acq_kernel of kernels_con.hip):
acq = (((EI pof_0) pof_1) ...) / cost with the arg-max, one pass over the q, mu of n_con + 1 (model, candidate set) pairs.

The EI term must be cbo_acq_sweep's bits at cost 1, the product and the division are IEEE operations on the call's own
terms (bit for bit against numpy), and each probability of feasibility is checked against a restatement of emukit 0.4's
ProbabilityOfFeasibility with scipy, fed the device's own cbo_gp_predict mean and variance:
    pof = scipy.stats.norm.cdf((value - (mean + jitter)) / sqrt(var))          ('>=': of the negated argument)

Tolerance of that check, c1 eps pof + c2 eps |u| phi(u) with eps = 2.2e-16, c1 = c2 = 8 (argued as the EI bound of
tests/test_parity_gpu.py::test_expected_improvement_over_the_whole_range_of_u is: ulps of the parts, not measured):
  * c1: the device's ndtr is cephes' rational functions with FMA Horner steps (within 5e-16 = 2.3 ulp of scipy's,
    cbo_device.h), one lean exponential (4.7e-16 = 2.1 ulp), a Newton reciprocal (1-2 ulp) and two roundings of the closing
    products: 8 ulp of pof.
  * c2: u itself.  value - (mean + jitter) is the same two IEEE operations on both sides; the device's quotient by the
    IEEE square root is within an ulp of numpy's two-step one (half an ulp each): 2 ulp of u, carried through Phi' = phi.
    The exponential's argument -u^2 / 2 is rounded once more on the device than in scipy's erfc (|u^2| half-ulps of
    exp(-u^2 / 2), cbo_device.h): in the lower tail, where Phi ~ phi / |u|, that is another eps |u| phi / 2 per
    half-ulp.  8 covers both with the margin c1 has."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from scipy.stats import norm

from conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu

INVALID, NOT_FITTED = -1, -5
EPS = 2.2e-16
C1, C2 = 8.0, 8.0
LE, GE = 0, 1


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def model(X, y, dtype="f64", **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, dtype=dtype, **kw)


def fixture_model(name):
    f = load_fixture(name)
    assert f["mX"] is None
    ls = f["lengthscale_arg"]
    return model(f["X"], f["y"], variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls),
                 noise_var=float(f["noise_var"])), f


def causal_model(n=40, d=2, seed=3, nan_at=None):
    """A causal model whose mean_function / variance_adjustment are closed forms (any point can be asked).  nan_at: a point
    whose prior mean is NaN."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.cos(X).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1))

    def mf(a):
        out = 0.3 * np.sin(a).sum(1, keepdims=True)
        if nan_at is not None:
            out[np.all(a == nan_at[None, :], axis=1)] = np.nan
        return out

    va = lambda a: 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2
    return model(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-4, mean_function=mf, variance_adjustment=va)


def random_model(n=30, d=2, seed=0, dtype="f64", fn=None):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    fn = fn or (lambda a: np.sin(2 * a).sum(1, keepdims=True))
    y = fn(X) + 0.1 * rng.standard_normal((n, 1))
    return model(X, y, dtype=dtype, variance=1.0, lengthscale=0.7, noise_var=1e-3)


def points(m, d=2, seed=1):
    return np.random.default_rng(seed).uniform(-2.5, 2.5, (m, d))


def grid_for(g, pts, **kw):
    from cbo_with_oop_amd import CandidateGrid
    return CandidateGrid(pts, g, **kw)


def constrained(lib, obj, cons, cost=1.0, want=True):
    """cbo_acq_sweep_constrained.  obj: (model, grid, y_best, task, jitter) or None; cons: [(model, grid, value, jitter,
    sense)].  Returns (rc, acq (m,), ei (m,) or None, pof (n_con, m), best_val, best_idx)."""
    n = len(cons)
    m = len(obj[1]) if obj else len(cons[0][1])
    acq = np.empty(m) if want else None
    ei = np.empty(m) if want and obj else None
    pof = np.empty((n, m)) if want and n else None
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    gps = (ctypes.c_void_p * max(n, 1))(*[c[0]._handle for c in cons])
    cds = (ctypes.c_void_p * max(n, 1))(*[c[1]._handle for c in cons])
    val = np.array([float(c[2]) for c in cons] or [0.0])
    jit = np.array([float(c[3]) for c in cons] or [0.0])
    sen = (ctypes.c_int * max(n, 1))(*[int(c[4]) for c in cons])
    rc = lib.load().cbo_acq_sweep_constrained(
        obj[0]._handle if obj else None, obj[1]._handle if obj else None, float(obj[2]) if obj else 0.0,
        lib.TASK_CODE[obj[3]] if obj else 0, float(obj[4]) if obj else 0.0, float(cost), n, gps, cds, lib.dptr(val),
        lib.dptr(jit), sen, lib.dptr(acq), lib.dptr(ei), lib.dptr(pof), ctypes.byref(bv), ctypes.byref(bi))
    return rc, acq, ei, pof, bv.value, bi.value


def plain_sweep(lib, g, grid, y_best, task, jitter, cost):
    """cbo_acq_sweep: (acq, mean, var, best_val, best_idx)."""
    m = len(grid)
    acq, mean, var = np.empty(m), np.empty(m), np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                       float(cost), lib.dptr(acq), lib.dptr(mean), lib.dptr(var), ctypes.byref(bv),
                                       ctypes.byref(bi)))
    return acq, mean, var, bv.value, bi.value


def pof_restated(g, pts, value, jitter, sense):
    """(restated pof, tolerance) from the device's own cbo_gp_predict (noise included)."""
    mean, var = g.predict(pts)
    u = (value - (mean[:, 0] + jitter)) / np.sqrt(var[:, 0])
    if sense == GE:
        u = -u
    ref = norm.cdf(u)
    with np.errstate(invalid="ignore"):
        tol = C1 * EPS * ref + C2 * EPS * np.abs(u) * norm.pdf(u)
    return ref, tol


def check_call(lib, obj, cons, pts, cost, offset=0):
    """Every per-candidate output and the winner of one call; returns (acq, ei, pof, best_idx)."""
    rc, acq, ei, pof, bv, bi = constrained(lib, obj, cons, cost)
    lib.check(rc)
    if obj:
        np.testing.assert_array_equal(ei, plain_sweep(lib, obj[0], obj[1], obj[2], obj[3], obj[4], 1.0)[0])
    for k, (g, _, value, jitter, sense) in enumerate(cons):
        ref, tol = pof_restated(g, pts, value, jitter, sense)
        err = np.abs(pof[k] - ref)
        ok = np.isnan(ref) & np.isnan(pof[k]) | (err <= tol)
        worst = np.nanmax(err / np.maximum(tol, 1e-320))
        print(f"pof[{k}] sense {sense}: worst error {np.nanmax(err):.3e}, worst error / tolerance {worst:.3f}")
        assert np.all(ok), (k, worst)
    terms = ([ei] if obj else []) + [pof[k] for k in range(len(cons))]
    prod = terms[0]
    for t in terms[1:]:
        prod = prod * t
    np.testing.assert_array_equal(acq, prod / cost)
    assert bi == int(np.argmax(acq)) + offset              # numpy's argmax: lowest index on ties, NaN maximal
    top = acq[bi - offset]
    assert (np.isnan(bv) and np.isnan(top)) or bv == np.nanmax(acq) == top
    # the winner alone (no per-candidate outputs: the kernel's other specialisation) is the same
    rc, _, _, _, bv2, bi2 = constrained(lib, obj, cons, cost, want=False)
    lib.check(rc)
    assert bi2 == bi and (bv2 == bv or (np.isnan(bv) and np.isnan(bv2)))
    return acq, ei, pof, bi


def binding_value(g, pts, q=0.5):
    """A bound in the middle of the model's predictive means: the constraint cuts the grid in two."""
    return float(np.quantile(g.predict(pts)[0][:, 0], q))


def assert_binds(g, pts, value, jitter, sense, unconstrained_idx, constrained_idx):
    ref, _ = pof_restated(g, pts, value, jitter, sense)
    frac = np.mean((ref > 0.1) & (ref < 0.9))
    assert frac >= 0.2, f"vacuous constraint: only {frac:.3f} of the candidates have 0.1 < pof < 0.9"
    assert constrained_idx != unconstrained_idx, "the constraint does not move the winner"


# ---- values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy_bo_d2", "complete_bo_d3", "graph_ard_d4"])
def test_golden_fixture_objective_with_one_binding_constraint(lib, name):
    g, f = fixture_model(name)
    pts = np.ascontiguousarray(f["Xs"])
    d = pts.shape[1]
    con = random_model(n=35, d=d, seed=5, fn=lambda a: a[:, :1] + 0.5 * np.cos(a).sum(1, keepdims=True))
    y_best, task = float(f["y_best"]), f["task"]
    go, gc = grid_for(g, pts), grid_for(con, pts)
    base = plain_sweep(lib, g, go, y_best, task, 0.0, 2.0)
    # n_con = 0: cbo_acq_sweep's own bits with the same cost
    rc, acq0, ei0, _, bv0, bi0 = constrained(lib, (g, go, y_best, task, 0.0), [], 2.0)
    lib.check(rc)
    np.testing.assert_array_equal(acq0, base[0])
    assert (bv0, bi0) == (base[3], base[4])
    # a bound through the constraint model's mean AT the unconstrained winner's side of the grid: it binds there
    mean_c = con.predict(pts)[0][:, 0]
    sd_c = np.sqrt(con.predict(pts)[1][:, 0])
    value = float(mean_c[bi0] - 1.5 * sd_c[bi0])         # pof at the unconstrained winner = Phi(-1.5) = 0.07
    _, _, _, bi = check_call(lib, (g, go, y_best, task, 0.0), [(con, gc, value, 0.0, LE)], pts, 2.0)
    if task == "min":                                    # ('max' keeps the reference's sign quirk: -EI, the product flips)
        ref, _ = pof_restated(con, pts, value, 0.0, LE)
        print(f"{name}: fraction with 0.1 < pof < 0.9: {np.mean((ref > 0.1) & (ref < 0.9)):.3f}; winner {bi0} -> {bi}")
    for x in (go, gc):
        x.close()


def test_binding_constraints_move_the_winner(lib):
    """Two cases (a non-causal and a causal objective) in which the constraint demonstrably binds: the restated feasibility
    lies strictly between 0.1 and 0.9 on at least 20 % of the candidates and the constrained winner is another candidate."""
    pts = points(3001, seed=4)
    for obj_model, con in ((random_model(seed=0), random_model(n=40, seed=7, fn=lambda a: a[:, :1] * 0.4)),
                           (causal_model(), random_model(n=40, seed=8, fn=lambda a: -0.4 * a[:, 1:2]))):
        go, gc = grid_for(obj_model, pts), grid_for(con, pts)
        y_best = float(obj_model.Y.min())
        base = plain_sweep(lib, obj_model, go, y_best, "min", 0.0, 1.0)
        mean_c, var_c = (a[:, 0] for a in con.predict(pts))
        # the bound sits 1.2 predictive sd below the constraint model's mean at the unconstrained winner (pof there
        # Phi(-1.2) = 0.12) and, the model's range being about +-1 with sd >= 0.03, inside the grid's spread of means
        value = float(mean_c[base[4]] - 1.2 * np.sqrt(var_c[base[4]]))
        _, _, _, bi = check_call(lib, (obj_model, go, y_best, "min", 0.0), [(con, gc, value, 0.0, LE)], pts, 1.0)
        assert_binds(con, pts, value, 0.0, LE, base[4], bi)
        go.close(); gc.close()


def test_three_constraints_of_mixed_sense_over_causal_and_plain_models(lib):
    pts = points(2049, seed=2)
    obj_model = causal_model(seed=3)
    c0 = random_model(seed=10, fn=lambda a: a[:, :1] * 0.5)
    c1 = causal_model(n=30, seed=11)
    c2 = random_model(n=50, seed=12, dtype="f32")
    grids = [grid_for(x, pts) for x in (obj_model, c0, c1, c2)]
    cons = [(c0, grids[1], binding_value(c0, pts), 0.0, LE), (c1, grids[2], binding_value(c1, pts, 0.4), 0.05, GE),
            (c2, grids[3], binding_value(c2, pts, 0.6), -0.1, LE)]
    y_best = float(obj_model.Y.min())
    for task in ("min", "max"):
        check_call(lib, (obj_model, grids[0], y_best, task, 0.01), cons, pts, 3.0)
    # no objective: the product of the three, and one alone (ProbabilityOfFeasibility.evaluate)
    acq, _, pof, _ = check_call(lib, None, cons, pts, 1.0)
    np.testing.assert_array_equal(acq, (pof[0] * pof[1]) * pof[2])
    acq1, _, pof1, _ = check_call(lib, None, cons[1:2], pts, 1.0)
    np.testing.assert_array_equal(acq1, pof1[0])
    np.testing.assert_array_equal(pof1[0], pof[1])
    for x in grids:
        x.close()


def test_fp32_objective_and_constraint(lib):
    pts = points(1500, seed=6)
    g, con = random_model(n=60, seed=1, dtype="f32"), random_model(n=45, seed=2, dtype="f32", fn=lambda a: 0.5 * a[:, 1:2])
    go, gc = grid_for(g, pts), grid_for(con, pts)
    check_call(lib, (g, go, float(g.Y.min()), "min", 0.0), [(con, gc, binding_value(con, pts), 0.0, GE)], pts, 1.5)
    go.close(); gc.close()


@pytest.mark.parametrize("m", [1, 7, 511, 513, 1000, 2 * 2048 * 256 + 3, (1 << 20) + 1])
def test_sizes(lib, m):
    """Odd m, m below one workgroup's span (512), m not a multiple of it, more candidates than one pass of the grid
    (2048 workgroups x 512), and m >= 2^20."""
    pts = points(m, seed=m % 97)
    g, con = random_model(seed=0), causal_model(n=25, seed=4)
    go, gc = grid_for(g, pts, index_offset=1000), grid_for(con, pts, index_offset=5)
    check_call(lib, (g, go, float(g.Y.min()), "min", 0.0), [(con, gc, binding_value(con, pts), 0.0, LE)], pts, 1.0,
               offset=1000)
    check_call(lib, None, [(con, gc, binding_value(con, pts), 0.0, GE)], pts, 1.0, offset=5)
    go.close(); gc.close()


def test_ties_and_nan(lib):
    base = points(300, seed=9)
    pts = np.vstack([base, base, base[:50]])             # every candidate twice or three times: ties everywhere
    g, con = random_model(seed=0), random_model(seed=3, fn=lambda a: 0.3 * a[:, :1])
    go, gc = grid_for(g, pts), grid_for(con, pts)
    acq, _, _, bi = check_call(lib, (g, go, float(g.Y.min()), "min", 0.0), [(con, gc, binding_value(con, pts), 0.0, LE)],
                               pts, 1.0)
    assert bi < 300 and np.sum(acq == acq[bi]) >= 2      # the first of the tied copies
    go.close(); gc.close()
    # NaN: the prior mean of one candidate of a causal constraint's set
    bad = 123
    cm = causal_model(seed=5, nan_at=pts[bad].copy())
    go, gc = grid_for(g, pts), grid_for(cm, pts)
    with np.errstate(invalid="ignore"):
        acq, _, pof, bi = check_call(lib, (g, go, float(g.Y.min()), "min", 0.0), [(cm, gc, 0.5, 0.0, LE)], pts, 1.0)
    dup = [i for i in range(len(pts)) if np.array_equal(pts[i], pts[bad])]
    assert bi == dup[0] and np.isnan(acq[dup]).all() and np.isnan(pof[0][dup]).all()
    assert np.isnan(acq).sum() == len(dup)
    go.close(); gc.close()


# ---- same bits ---------------------------------------------------------------------------------------------------------
def reference_case():
    pts = points(2500, seed=21)
    g = causal_model(seed=3)
    c0 = random_model(seed=10, fn=lambda a: a[:, :1] * 0.5)
    c1 = random_model(n=50, seed=12, dtype="f32")
    return pts, g, c0, c1


def run_reference_case(lib):
    pts, g, c0, c1 = reference_case()
    grids = [grid_for(x, pts) for x in (g, c0, c1)]
    cons = [(c0, grids[1], 0.1, 0.0, LE), (c1, grids[2], -0.2, 0.02, GE)]
    out = constrained(lib, (g, grids[0], float(g.Y.min()), "min", 0.0), cons, 2.5)
    lib.check(out[0])
    return out[1:], (g, grids, cons)


def test_two_calls_and_a_cached_and_a_fresh_sweep_give_the_same_bits(lib):
    first, (g, grids, cons) = run_reference_case(lib)                # fresh: every pair is substituted
    again = constrained(lib, (g, grids[0], float(g.Y.min()), "min", 0.0), cons, 2.5)[1:]      # every pair cached
    fresh, _ = run_reference_case(lib)                               # new models, new sets
    for a, b, c in zip(first, again, fresh):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    # one pair cached by cbo_acq_sweep, the others not
    pts, g2, c0, c1 = reference_case()
    grids2 = [grid_for(x, pts) for x in (g2, c0, c1)]
    plain_sweep(lib, g2, grids2[0], 0.0, "min", 0.0, 1.0)
    cons2 = [(c0, grids2[1], 0.1, 0.0, LE), (c1, grids2[2], -0.2, 0.02, GE)]
    mixed = constrained(lib, (g2, grids2[0], float(g2.Y.min()), "min", 0.0), cons2, 2.5)[1:]
    for a, b in zip(first, mixed):
        np.testing.assert_array_equal(a, b)


CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import test_constrained_gpu as t
from cbo_with_oop_amd import _lib
(acq, ei, pof, bv, bi), keep = t.run_reference_case(_lib)
(acq2, ei2, pof2, bv2, bi2) = t.constrained(_lib, (keep[0], keep[1][0], float(keep[0].Y.min()), "min", 0.0), keep[2], 2.5)[1:]
assert np.array_equal(acq, acq2) and bi == bi2
np.savez({out!r}, acq=acq, ei=ei, pof=pof, bv=bv, bi=bi)
"""


def test_sweep_cache_off_gives_the_same_bits(lib, tmp_path):
    """CBO_HIP_SWEEP_CACHE is read by cbo_init: the cache-off run is a child process of its own."""
    first, _ = run_reference_case(lib)
    out = str(tmp_path / "off.npz")
    env = dict(os.environ, CBO_HIP_SWEEP_CACHE="0")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    off = np.load(out)
    np.testing.assert_array_equal(first[0], off["acq"])
    np.testing.assert_array_equal(first[1], off["ei"])
    np.testing.assert_array_equal(first[2], off["pof"])
    assert first[3] == float(off["bv"]) and first[4] == int(off["bi"])


def test_appended_constraint_model_extends_its_kept_solution(lib):
    """cbo_gp_append on a constraint model whose set keeps its solution: the call reaches q, mu by the one-row extension,
    as cbo_acq_sweep does.  The pof bits are those of the mean and variance cbo_acq_sweep reports for the same pair on the
    refit path's side -- a second model given the same history (fit, sweep, append) and swept by cbo_acq_sweep alone --
    checked bit for bit through the call on that second pair once cbo_acq_sweep has extended it."""
    pts = points(1200, seed=31)
    g = random_model(seed=0)
    x_new, y_new = np.array([[0.3, -0.7]]), np.array([[0.25]])
    results = []
    for via_plain_sweep in (False, True):
        con = random_model(n=40, seed=13, fn=lambda a: 0.5 * a[:, :1])
        go, gc = grid_for(g, pts), grid_for(con, pts, keep_solution=True)
        cons = [(con, gc, 0.1, 0.0, LE)]
        lib.check(constrained(lib, (g, go, float(g.Y.min()), "min", 0.0), cons, 1.0)[0])       # V stays with the set
        n0 = int(lib.load().cbo_gp_n(con._handle))
        con.append(x_new, y_new)
        assert int(lib.load().cbo_gp_n(con._handle)) == n0 + 1
        if via_plain_sweep:
            _, mean, var, _, _ = plain_sweep(lib, con, gc, 0.0, "min", 0.0, 1.0)              # extends the row itself
            results.append((mean, var))
        out = constrained(lib, (g, go, float(g.Y.min()), "min", 0.0), cons, 1.0)
        lib.check(out[0])
        results.append(out[1:])
        # the extended vectors are the appended model's: the pof agrees with the restatement on ITS predictions
        ref, tol = pof_restated(con, pts, 0.1, 0.0, LE)
        mean_r, var_r = (a[:, 0] for a in con.predict(pts))
        if via_plain_sweep:
            # extension against substitution: the same posterior to rounding (cbo_gp_append: "up to rounding")
            np.testing.assert_allclose(mean, mean_r, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(var, var_r, rtol=1e-9, atol=1e-12)
            u = (0.1 - mean) / np.sqrt(var)
            err = np.abs(out[3][0] - norm.cdf(u))
            assert np.all(err <= C1 * EPS * norm.cdf(u) + C2 * EPS * np.abs(u) * norm.pdf(u)), err.max()
        go.close(); gc.close()
    direct, (_, _), after_plain = results[0], results[1], results[2]
    for a, b in zip(direct, after_plain):
        np.testing.assert_array_equal(a, b)


def test_models_are_left_untouched(lib):
    pts, g, c0, c1 = reference_case()
    before = [[np.array(a, copy=True) for a in x.posterior_state()] for x in (g, c0, c1)]
    stale = [x.stale for x in (g, c0, c1)]
    grids = [grid_for(x, pts) for x in (g, c0, c1)]
    cons = [(c0, grids[1], 0.1, 0.0, LE), (c1, grids[2], -0.2, 0.02, GE)]
    for _ in range(2):
        lib.check(constrained(lib, (g, grids[0], float(g.Y.min()), "min", 0.0), cons, 2.5)[0])
    after = [x.posterior_state() for x in (g, c0, c1)]
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            np.testing.assert_array_equal(x, y)
    assert stale == [x.stale for x in (g, c0, c1)]
    assert all(lib.load().cbo_gp_jitter(x._handle, None, None) == 0 for x in (g, c0, c1))      # still fitted


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_invalid_and_unfitted(lib):
    from cbo_with_oop_amd import CandidateGrid
    pts = points(100, seed=41)
    g, con, cm = random_model(seed=0), random_model(seed=1), causal_model(seed=2)
    go, gc = grid_for(g, pts), grid_for(con, pts)
    obj = (g, go, 0.0, "min", 0.0)
    ok = [(con, gc, 0.0, 0.0, LE)]
    assert constrained(lib, obj, ok)[0] == 0
    assert constrained(lib, obj, ok * 9)[0] == INVALID                                  # n_con > CBO_MAX_CONSTRAINTS
    assert constrained(lib, obj, [(con, gc, np.nan, 0.0, LE)])[0] == INVALID
    assert constrained(lib, obj, [(con, gc, np.inf, 0.0, LE)])[0] == INVALID
    assert constrained(lib, obj, [(con, gc, 0.0, np.nan, LE)])[0] == INVALID
    assert constrained(lib, obj, [(con, gc, 0.0, 0.0, 2)])[0] == INVALID
    assert constrained(lib, obj, [(con, gc, 0.0, 0.0, -1)])[0] == INVALID
    for cost in (0.0, -1.0, np.nan):
        assert constrained(lib, obj, ok, cost=cost)[0] == INVALID
    L = lib.load()
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    one = lambda *h: (ctypes.c_void_p * 1)(*h)
    val, sen = np.zeros(1), (ctypes.c_int * 1)(0)
    raw = lambda gp, cd, task, n, gps, cds, v, j, s, ei=None: L.cbo_acq_sweep_constrained(
        gp, cd, 0.0, task, 0.0, 1.0, n, gps, cds, v, j, s, None, ei, None, ctypes.byref(bv), ctypes.byref(bi))
    dv = lib.dptr(val)
    assert raw(g._handle, go._handle, 7, 1, one(con._handle), one(gc._handle), dv, dv, sen) == INVALID       # bad task
    assert raw(None, None, 7, 1, one(con._handle), one(gc._handle), dv, dv, sen) == 0   # ... unused without objective
    assert raw(g._handle, None, 0, 1, one(con._handle), one(gc._handle), dv, dv, sen) == INVALID
    assert raw(None, go._handle, 0, 1, one(con._handle), one(gc._handle), dv, dv, sen) == INVALID
    assert raw(None, None, 0, 0, None, None, None, None, None) == INVALID               # nothing to score
    assert raw(None, None, 0, 1, one(con._handle), one(gc._handle), dv, dv, sen, ei=lib.dptr(np.empty(100))) == INVALID
    assert raw(g._handle, go._handle, 0, 1, one(None), one(gc._handle), dv, dv, sen) == INVALID
    assert raw(g._handle, go._handle, 0, 1, one(con._handle), one(None), dv, dv, sen) == INVALID
    assert raw(g._handle, go._handle, 0, 1, None, one(gc._handle), dv, dv, sen) == INVALID
    assert raw(g._handle, go._handle, 0, 1, one(con._handle), one(gc._handle), None, dv, sen) == INVALID
    assert raw(g._handle, go._handle, 0, 1, one(con._handle), one(gc._handle), dv, None, sen) == INVALID
    assert raw(g._handle, go._handle, 0, 1, one(con._handle), one(gc._handle), dv, dv, None) == INVALID
    assert raw(g._handle, go._handle, 0, -1, None, None, None, None, None) == INVALID
    # sets whose m differ, dimensions that differ, a causal model whose set carries no prior, one set with two models
    short = grid_for(con, pts[:50])
    assert constrained(lib, obj, [(con, short, 0.0, 0.0, LE)])[0] == INVALID
    g3 = random_model(d=3, seed=4)
    assert constrained(lib, obj, [(g3, gc, 0.0, 0.0, LE)])[0] == INVALID
    assert constrained(lib, obj, [(cm, gc, 0.0, 0.0, LE)])[0] == INVALID
    assert constrained(lib, (cm, go, 0.0, "min", 0.0), ok)[0] == INVALID
    assert constrained(lib, obj, [(con, go, 0.0, 0.0, LE)])[0] == INVALID
    assert constrained(lib, obj, [(g, go, 0.0, 0.0, LE)])[0] == 0                       # the same pair twice is one pair
    # pairs on different contexts
    other = lib.Context(go._ctx.device_id)
    try:
        far = CandidateGrid(pts, context=other)
        assert constrained(lib, obj, [(con, far, 0.0, 0.0, LE)])[0] == INVALID
        far.close()
    finally:
        other.close()
    # unfitted models
    u = model(g.X, g.Y, variance=1.0, lengthscale=0.7, noise_var=1e-3, fit=False)
    gu = grid_for(u, pts)
    assert constrained(lib, obj, [(u, gu, 0.0, 0.0, LE)])[0] == NOT_FITTED
    assert constrained(lib, (u, gu, 0.0, "min", 0.0), ok)[0] == NOT_FITTED
    assert constrained(lib, None, [(u, gu, 0.0, 0.0, LE)])[0] == NOT_FITTED
    # the refusals left the valid call working
    assert constrained(lib, obj, ok)[0] == 0


# ---- the Python layer --------------------------------------------------------------------------------------------------
def restated_product(obj_model, y_best, cons, pts, cost):
    from cbo_with_oop_amd import CausalExpectedImprovement
    val = CausalExpectedImprovement(y_best, "min", obj_model).evaluate(pts)[:, 0]
    for c in cons:
        ref, _ = pof_restated(c.model, pts, float(c.max_value), float(c.jitter), GE if c.sense == ">=" else LE)
        val = val * ref
    return val / cost


def test_find_next_y_point_with_constraints(lib):
    from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility, find_next_y_point
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    g, c0, c1 = random_model(seed=0), random_model(n=40, seed=7, fn=lambda a: a[:, :1] * 0.4), causal_model(seed=9)
    bounds = [(-2.5, 2.5)] * 2
    pts = meshgrid_candidates(bounds, [40, 30])
    y_best = float(g.Y.min())
    free_y, free_x = find_next_y_point(bounds, g, y_best, ["a", "b"], {"a": lambda c: 1.0, "b": lambda c: 1.0},
                                       grid_shape=[40, 30])
    mean_c, var_c = (a[:, 0] for a in c0.predict(pts))
    at = int(np.argmin(np.abs(pts - free_x).sum(1)))
    cons = [ProbabilityOfFeasibility(c0, 0.0, float(mean_c[at] - 1.2 * np.sqrt(var_c[at]))),
            ProbabilityOfFeasibility(c1, 0.01, binding_value(c1, pts), sense=">=")]
    for costs in ({"a": lambda c: 1.0, "b": lambda c: 1.0}, {"a": lambda c: 1.0 + np.sum(np.abs(c)), "b": lambda c: 2.0}):
        y, x = find_next_y_point(bounds, g, y_best, ["a", "b"], costs, grid_shape=[40, 30], constraints=cons)
        assert y.shape == (1, 1) and x.shape == (1, 2)
        batch_cost = sum(costs[k](pts[:, j]) for j, k in enumerate(("a", "b")))
        ref = restated_product(g, y_best, cons, pts, batch_cost)
        win = int(np.argmax(ref))
        near = np.abs(ref - ref[win]) <= 1e-12 * abs(ref[win])
        got = int(np.argmin(np.abs(pts - x).sum(1)))
        assert np.array_equal(pts[got], x[0]) and near[got], (got, win)
        point_cost = sum(costs[k](x[:, j]) for j, k in enumerate(("a", "b")))
        np.testing.assert_allclose(y[0, 0], restated_product(g, y_best, cons, x, point_cost)[0], rtol=1e-12)
    assert not np.array_equal(x, free_x)                 # the constraints bind: another point than the free optimum


def test_optimizer_refines_a_product_over_a_cost(lib):
    from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost,
                                                  ProbabilityOfFeasibility)
    g, c0 = random_model(seed=0), random_model(n=40, seed=7, fn=lambda a: a[:, :1] * 0.4)
    acq = (CausalExpectedImprovement(float(g.Y.min()), "min", g) * ProbabilityOfFeasibility(c0, 0.0, 0.1)
           / Cost({"a": lambda c: 1.5, "b": lambda c: 0.5}, ["a", "b"]))
    opt = CausalGradientAcquisitionOptimizer([(-2.5, 2.5)] * 2, grid_shape=[24, 24])
    x0, f0 = opt.optimize(acq)
    np.testing.assert_allclose(f0[0, 0], acq.evaluate(x0)[0, 0], rtol=1e-12)
    for starts in (1, 4):
        x1, f1 = opt.optimize(acq, refine=True, num_starts=starts)
        assert f1[0, 0] >= f0[0, 0]
        np.testing.assert_allclose(acq.evaluate(x1)[0, 0], f1[0, 0], rtol=1e-9)
        assert np.all(x1 >= -2.5) and np.all(x1 <= 2.5)
    acq.numerator.close()
