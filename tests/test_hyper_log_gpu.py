"""GPU tests of the hyper-marginalised EI in log space (cbo_acq_sweep_hyper_log, cbo_acq_sweep_sets_hyper_log, cbo_lse_rows;
hyper_avg_kernel<true>, hyper_sets_kernel<*, true>, hyper_lse_accumulate_kernel / hyper_lse_finish_kernel).

    acq_i = log((1 / H) sum_h EI_h,i) - log cost = LSE_h(l_h,i) - log H - log cost

The contract is stated in three steps.  (1) With one sample at the model's own hyper-parameters the call is
cbo_acq_sweep_logei, bit for bit.  (2) With H samples it is, bit for bit, cbo_lse_rows over the terms cbo_acq_sweep_logei
writes at cost 1 on H fitted twins: the sweep's terms are those calls' terms and its reduction is the stated one.  (3) What
cbo_lse_rows computes is the log-sum-exp of its terms: against mpmath (60 digits) of the same doubles the error stays below
4 * 2^-53 * (H + |ref|) -- H terms of a few ulp of relative error in S, one log, three roundings at the result's magnitude.
Worst values measured on the MI355X, in units of 2^-53 (H + |ref|), bar 4: cbo_lse_rows on random terms (H up to 50) 2.41;
the sweep and cbo_lse_rows alike on the dead fixture 1.39 (H = 2), 1.33 (H = 3), 1.54 (H = 10) at cost 3.7 and 1.16, 0.95, 0.83
at cost 1.  exp(acq) against the marginalised EI where that is >= 1e-290 (58 candidates): 3.1e-13 relative; the bar measured
on the ten single-sample twins is twice 8.7e-13.

The dead fixture is DESIGN.md 4x's: 50 observations with noise 1e-10, 200 grid points, ten samples; the marginalised EI is an
exact 0.0 over most of the grid and the log form orders all of it.

Shapes: n in {1, 16, 17, 50, 64, 128, 129}, m in {1, 63, 64, 65, 130, 200, 257, 704, 768}, d in {1, 2, 3, 8}, ARD and not,
causal and plain, both tasks, H in {1, 2, 3, 10}, both schedules."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import load_fixture
from test_hyper_log_host import lse_error_in_bar_units, lse_reference
from test_sets_hyper_gpu import (SHAPES, Set, factory_model, handles, make_model, prior_mean, prior_var, problem, same_value,
                                 samples_for, toy_problem)

pytestmark = pytest.mark.gpu

BAR = 4.0                         # in units of 2^-53 (H + |ref|)


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def logei_single(model, grid, y_best, task, cost, jitter=0.0):
    """cbo_acq_sweep_logei: (acq (m,), value, index)."""
    from cbo_with_oop_amd import _lib
    acq = np.empty(len(grid))
    val, idx = ctypes.c_double(), ctypes.c_int64()
    model.ensure_fitted()
    _lib.check(_lib.load().cbo_acq_sweep_logei(model._handle, grid._handle, float(y_best), _lib.TASK_CODE[task], jitter,
                                               float(cost), _lib.dptr(acq), None, None, ctypes.byref(val), ctypes.byref(idx)))
    return acq, val.value, idx.value


def ei_single(model, grid, y_best, task, cost=1.0):
    from cbo_with_oop_amd import _lib
    acq = np.empty(len(grid))
    model.ensure_fitted()
    _lib.check(_lib.load().cbo_acq_sweep(model._handle, grid._handle, float(y_best), _lib.TASK_CODE[task], 0.0, float(cost),
                                         _lib.dptr(acq), None, None, None, None))
    return acq


def hyper_single(name, model, grid, rows, y_best, task, cost, jitter=0.0, rc_only=False):
    """cbo_acq_sweep_hyper_log (or cbo_acq_sweep_hyper): (acq (m,), value, index)."""
    from cbo_with_oop_amd import _lib
    acq = np.full(len(grid), -7.0)
    val, idx = ctypes.c_double(-7.0), ctypes.c_int64(-7)
    rows = np.ascontiguousarray(rows)
    rc = getattr(_lib.load(), name)(model._handle, grid._handle, rows.shape[0], _lib.dptr(rows), float(y_best),
                                    _lib.TASK_CODE[task], jitter, float(cost), _lib.dptr(acq), ctypes.byref(val),
                                    ctypes.byref(idx))
    if rc_only:
        return rc, acq, val.value, idx.value
    _lib.check(rc)
    return acq, val.value, idx.value


def hyper_log(model, grid, rows, y_best, task, cost, jitter=0.0):
    return hyper_single("cbo_acq_sweep_hyper_log", model, grid, rows, y_best, task, cost, jitter)


def sets_hyper_log(sets, y_best, task, costs, jitter=0.0, rc_only=False, rows=None):
    from cbo_with_oop_amd import _lib
    s = len(sets)
    rows = [np.ascontiguousarray(st.rows) for st in sets] if rows is None else rows
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    counts = (ctypes.c_int * s)(*[r.shape[0] for r in rows])
    ptrs = (ctypes.c_void_p * s)(*[r.ctypes.data for r in rows])
    rc = _lib.load().cbo_acq_sweep_sets_hyper_log(
        s, handles([st.model for st in sets]), handles([st.grid for st in sets]), counts, ptrs,
        _lib.dptr(np.asarray(y_best, dtype=np.float64)), _lib.TASK_CODE.get(task, task), jitter,
        _lib.dptr(np.asarray(costs, dtype=np.float64)), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p))
    if rc_only:
        return rc, vals, idxs
    _lib.check(rc)
    return vals, idxs


def lse_rows(ctx, terms, cost):
    from cbo_with_oop_amd import _lib
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    out = np.full(terms.shape[1], -7.0)
    _lib.check(_lib.load().cbo_lse_rows(ctx.handle, terms.shape[0], terms.shape[1], _lib.dptr(terms), float(cost),
                                        _lib.dptr(out)))
    return out


def gp(X, y, row, ard=False, causal=False, dtype=None, context=None, fit=True):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    kw = dict(variance=float(row[0]), lengthscale=np.array(row[1:-1], dtype=np.float64) if ard else float(row[1]), ard=ard,
              noise_var=float(row[-1]), fit=fit)
    if causal:
        kw.update(mean_function=prior_mean, variance_adjustment=prior_var)
    if dtype:
        kw["dtype"] = dtype
    if context is not None:
        kw["context"] = context
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def twin_terms(hip, X, y, Xs, rows, y_best, task, ard=False, causal=False, dtype=None, jitter=0.0, with_ei=False):
    """Per row a fitted twin carrying the row's hyper-parameters: cbo_acq_sweep_logei at cost 1 over Xs -> (H, m) terms
    (with_ei: cbo_acq_sweep's values beside them)."""
    terms, eis = [], []
    for row in rows:
        twin = gp(X, y, row, ard, causal, dtype)
        grid = hip.CandidateGrid(Xs, twin)
        with np.errstate(invalid="ignore"):
            terms.append(logei_single(twin, grid, y_best, task, 1.0, jitter)[0])
            if with_ei:
                eis.append(ei_single(twin, grid, y_best, task))
        grid.close(); twin.close()
    return (np.array(terms), np.array(eis)) if with_ei else np.array(terms)


def first_max(v):
    """The library's tie rule: the lowest index of the maximum, NaN maximal."""
    v = np.asarray(v)
    return int(np.argmax(np.isnan(v))) if np.isnan(v).any() else int(np.argmax(v))


# ---- 1. one sample at the model's own hyper-parameters is the log EI -----------------------------------------------------------
# (n, m, d, ard, causal)
OWN_SHAPES = [(1, 1, 1, False, False), (16, 63, 3, False, False), (17, 257, 1, False, True), (128, 200, 3, True, False)]


@pytest.fixture(scope="module")
def own_sets(hip):
    sets = []
    for n, m, d, ard, causal in OWN_SHAPES:
        st = Set.__new__(Set)
        st.X, st.y, st.Xs = problem(n, m, d, seed=n + m)
        st.rows = samples_for(d, ard, 1, seed=n, own_first=True)
        st.model = make_model(st.X, st.y, st.rows[0], ard, causal, fit=False)          # the call's own model: never fitted
        st.grid = hip.CandidateGrid(st.Xs, st.model, index_offset=5 * n)
        st.twin = make_model(st.X, st.y, st.rows[0], ard, causal)
        st.twin_grid = hip.CandidateGrid(st.Xs, st.twin, index_offset=5 * n)
        sets.append(st)
    yield sets
    for st in sets:
        st.grid.close(); st.model.close(); st.twin_grid.close(); st.twin.close()


@pytest.mark.parametrize("task", ["min", "max"])
def test_one_sample_at_the_models_own_hyper_parameters_is_the_log_ei(hip, own_sets, task):
    from cbo_with_oop_amd import _lib
    s = len(own_sets)
    y_best = np.array([float(np.median(st.y)) for st in own_sets])
    costs = np.array([1.0, 3.7, 0.3, 2.0])
    for i, st in enumerate(own_sets):
        want = logei_single(st.twin, st.twin_grid, y_best[i], task, costs[i], jitter=0.01)
        got = hyper_log(st.model, st.grid, st.rows, y_best[i], task, costs[i], jitter=0.01)
        print(OWN_SHAPES[i], task, got[1], got[2], want[1], want[2])
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
        assert st.model.stale
    vals, idxs = sets_hyper_log(own_sets, y_best, task, costs, jitter=0.01)
    want_v, want_i = np.empty(s), np.empty(s, dtype=np.int64)
    _lib.check(_lib.load().cbo_acq_sweep_sets_logei(s, handles([st.twin for st in own_sets]),
                                                    handles([st.twin_grid for st in own_sets]), _lib.dptr(y_best),
                                                    _lib.TASK_CODE[task], 0.01, _lib.dptr(costs), _lib.dptr(want_v),
                                                    want_i.ctypes.data_as(_lib.c_int64_p)))
    assert same_bits(vals, want_v) and np.array_equal(idxs, want_i)


# ---- the dead fixture and its ten samples: shared by 2, 3 and 4 ------------------------------------------------
@pytest.fixture(scope="module")
def dead(hip):
    class Dead:
        pass
    d = Dead()
    d.X = np.random.default_rng(7).uniform(-5, 20, (50, 1))
    d.y = np.cos(d.X) - np.exp(-d.X / 20)
    d.y_best = float(d.y.min())
    d.points = np.linspace(-5, 20, 200)[:, None]
    d.rows = np.array([(v, l, 1e-10) for l in (0.85, 1.0, 1.15, 1.3) for v in (0.5, 1.0, 2.0)][:10])
    d.model = gp(d.X, d.y, (1.0, 1.0, 1e-10), fit=False)
    d.grid = hip.CandidateGrid(d.points, d.model)
    # the per-sample terms: cbo_acq_sweep_logei at cost 1 on ten fitted twins (and cbo_acq_sweep beside it), computed once
    d.terms, d.eis = twin_terms(hip, d.X, d.y, d.points, d.rows, d.y_best, "min", with_ei=True)
    d.terms.setflags(write=False); d.eis.setflags(write=False)
    yield d
    d.grid.close(); d.model.close()


def orders(terms):
    """The samples in orders that meet every branch of the push, chosen from the terms: the pair (a, b) that shares the grid
    most evenly -- b leads in one part and a in the other, so b raises the maximum for some candidates and not for others;
    with three samples a comes again (equal terms: l == M where a leads); with ten, the others follow (the last one giving
    way to the repeated a)."""
    m = terms.shape[1]
    share = lambda a, b: min(int(np.sum(terms[b] > terms[a])), int(np.sum(terms[b] < terms[a])))          # noqa: E731
    a, b = max(((a, b) for a in range(len(terms)) for b in range(len(terms)) if a < b), key=lambda p: share(*p))
    assert 0 < share(a, b) <= m // 2
    rest = [h for h in range(len(terms)) if h not in (a, b)]
    return {2: [a, b], 3: [a, b, a], 10: [a, b, a] + rest[:-1]}


def push_branches(terms):
    """How often each branch of lse_push is taken over (H, m) terms, per sample: (raised, met, below), and the arguments
    the two exps receive."""
    M = terms[0].copy()
    counts, args = [], []
    for l in terms[1:]:
        up, eq = l > M, l == M
        counts.append((int(up.sum()), int(eq.sum()), int((~up & ~eq).sum())))
        args.append(np.where(up, M - l, l - M)[~eq])
        M = np.where(up, l, M)
    return counts, np.concatenate(args)


@pytest.mark.parametrize("H", [2, 3, 10])
def test_the_reduction_is_the_pinned_one(hip, dead, H):
    order = orders(dead.terms)[H]
    terms, rows = dead.terms[order], dead.rows[order]
    counts, args = push_branches(terms)
    print("H", H, "order", order, "branches (raised, met, below) per sample", counts, "smallest exp argument", args.min())
    if H == 2:
        assert counts[0][0] > 0 and counts[0][2] > 0      # the second sample raises the maximum for some candidates, not for others
    else:
        assert sum(c[1] for c in counts) > 0              # the repeated sample meets its own maximum
        assert any(c[0] > 0 and c[2] > 0 for c in counts)
    assert np.any(args < -746.0) and np.all(np.exp(args[args < -746.0]) == 0.0)        # some exp underflows to 0
    for cost in (1.0, 3.7):
        want = lse_rows(dead.model._ctx, terms, cost)
        acq, val, idx = hyper_log(dead.model, dead.grid, rows, dead.y_best, "min", cost)
        assert same_bits(acq, want), (H, cost, np.flatnonzero(bits(acq) != bits(want))[:8])
        assert idx == first_max(want) and same_bits(val, want[idx])
    assert dead.model.stale


# ---- 3. accuracy against mpmath ----------------------------------------------------------------------------------------------
def test_accuracy_of_the_reduction_on_random_terms(hip, dead):
    rng = np.random.default_rng(5)
    worst = 0.0
    for H in (1, 2, 3, 10, 50):
        m = 257
        for terms in (rng.normal(-20.0, 3.0, (H, m)), rng.uniform(-700.0, 5.0, (H, m)),
                      rng.normal(0.0, 1.0, (H, m)) + 1e8 * rng.integers(-4, 1, (H, m))):
            for cost in (1.0, 3.7):
                err = lse_error_in_bar_units(lse_rows(dead.model._ctx, terms, cost), lse_reference(terms, cost), H)
                worst = max(worst, err)
                assert err <= BAR, (H, cost, err)
    print("cbo_lse_rows on random terms: worst error", worst, "in units of 2^-53 (H + |ref|), bar", BAR)
    # the contracts: -inf is an ordinary value, NaN propagates, one row is the row itself
    inf, nan = np.inf, np.nan
    got = lse_rows(dead.model._ctx, np.array([[-inf, -inf, -2.0, nan, -1.0], [-inf, -2.0, -inf, -1.0, nan],
                                              [-inf, -inf, -inf, -1.0, -1.0]]), 1.0)
    assert got[0] == -inf and same_bits(got[1:3], np.array([-2.0, -2.0]) - np.log(3.0)) and np.all(np.isnan(got[3:]))
    one = np.array([[-4.9e8, -1.25, 0.0, 700.0, -inf]])
    assert same_bits(lse_rows(dead.model._ctx, one, 1.0), one[0])


@pytest.mark.parametrize("H", [2, 3, 10])
def test_accuracy_of_the_sweep_on_the_dead_fixture(hip, dead, H):
    order = orders(dead.terms)[H] if H < 10 else list(range(10))
    terms, rows = dead.terms[order], dead.rows[order]
    for cost in (1.0, 3.7):
        ref = lse_reference(terms, cost)
        acq = hyper_log(dead.model, dead.grid, rows, dead.y_best, "min", cost)[0]
        err = lse_error_in_bar_units(acq, ref, H)
        err_rows = lse_error_in_bar_units(lse_rows(dead.model._ctx, terms, cost), ref, H)
        print("dead fixture, H", H, "cost", cost, "worst error: sweep", err, "cbo_lse_rows", err_rows, "bar", BAR)
        assert err <= BAR and err_rows <= BAR


# ---- 4. the dead region is ordered ------------------------------------------------------------------------------------------
def test_the_dead_region_is_ordered(hip, dead):
    ei = hyper_single("cbo_acq_sweep_hyper", dead.model, dead.grid, dead.rows, dead.y_best, "min", 1.0)
    zeros = int(np.sum(ei[0] == 0.0))
    print("marginalised EI: exact zeros", zeros, "of 200, arg-max", ei[2])
    assert zeros >= 100                                              # the precondition: most of the grid is dead for the EI
    acq, val, idx = hyper_log(dead.model, dead.grid, dead.rows, dead.y_best, "min", 1.0)
    assert np.all(np.isfinite(acq)) and len(np.unique(acq)) == 200
    print("log form: range", acq.min(), acq.max(), "arg-max", idx, "per-sample terms down to", dead.terms.min())
    assert idx == ei[2] and same_bits(val, acq[idx])
    # the order over the dead candidates is the reference's
    ref = np.array([float(r) for r in lse_reference(dead.terms, 1.0)])
    is_dead = ei[0] == 0.0
    assert np.array_equal(np.argsort(acq[is_dead], kind="stable"), np.argsort(ref[is_dead], kind="stable"))
    # where the marginalised EI is representable, exp(acq) is that EI.  The bar is measured on the parent's code: the worst
    # relative deviation of exp(cbo_acq_sweep_logei) from cbo_acq_sweep over the ten single-sample twins, twice, at most 1e-10
    seen = dead.eis >= 1e-290
    measured = float(np.max(np.abs(np.exp(dead.terms[seen]) - dead.eis[seen]) / dead.eis[seen]))
    bar = min(2.0 * measured, 1e-10)
    alive = ei[0] >= 1e-290
    assert alive.any()
    rel = float(np.max(np.abs(np.exp(acq[alive]) - ei[0][alive]) / ei[0][alive]))
    print("exp(acq) against the marginalised EI over", int(alive.sum()), "candidates: worst relative deviation", rel,
          "| single-sample twins measured", measured, "bar", bar)
    assert rel <= bar


# ---- 5. one launch equals the per-set calls, either schedule -------------------------------------------------------------------
def build_sets(hip, shapes, context=None, seed=0):
    sets = []
    for n, m, d, ard, causal, H, offset in shapes:
        st = Set.__new__(Set)
        st.shape = (n, m, d, ard, causal, H, offset)
        st.X, st.y, st.Xs = problem(n, m, d, seed=n + m + seed)
        st.rows = samples_for(d, ard, H, seed=n + seed)
        st.ard, st.causal = ard, causal
        st.model = gp(st.X, st.y, st.rows[0], ard, causal, context=context, fit=False)
        st.grid = hip.CandidateGrid(st.Xs, st.model, index_offset=offset)
        sets.append(st)
    return sets


def close_sets(sets):
    for st in sets:
        st.grid.close(); st.model.close()


def per_set(sets, y_best, task, costs, jitter=0.0):
    got = [hyper_log(st.model, st.grid, st.rows, y_best[i], task, costs[i], jitter) for i, st in enumerate(sets)]
    return np.array([g[1] for g in got]), np.array([g[2] for g in got], dtype=np.int64), [g[0] for g in got]


ZOO_COSTS = [3.0, 1.0, 0.5, 2.0, 1.5, 4.0, 0.25, 7.0, 1.0]
THRESHOLD_SHAPES = {704: [(17, 704, 3, True, True, 3, 11), (17, 65, 3, False, False, 3, 0)],
                    768: [(17, 768, 3, True, True, 3, 11), (17, 65, 3, False, False, 3, 0)]}


@pytest.fixture(scope="module")
def zoo_answers(hip):
    """The per-set calls on the default context, once: what every schedule must reproduce."""
    out = {}
    zoo = build_sets(hip, SHAPES)
    nine = zoo + [zoo[1], zoo[3], zoo[5]]
    for task in ("min", "max"):
        y_best = [float(st.y.min() if task == "min" else st.y.max()) for st in nine]
        out["zoo", task] = (y_best,) + per_set(nine, y_best, task, ZOO_COSTS, jitter=0.01)
        vals, idxs = sets_hyper_log(nine, y_best, task, ZOO_COSTS, jitter=0.01)
        assert same_bits(vals, out["zoo", task][1]) and np.array_equal(idxs, out["zoo", task][2]), ("default schedule", task)
        three = sets_hyper_log(nine[:3], y_best[:3], task, ZOO_COSTS[:3], jitter=0.01)       # (descriptors by value)
        assert same_bits(three[0], vals[:3]) and np.array_equal(three[1], idxs[:3])
    close_sets(zoo)
    for m, shapes in THRESHOLD_SHAPES.items():
        pair = build_sets(hip, shapes)
        for task in ("min", "max"):
            y_best = [float(pair[0].y.min()), float(pair[1].y.max())]
            out[m, task] = (y_best,) + per_set(pair, y_best, task, [2.0, 3.0])
            vals, idxs = sets_hyper_log(pair, y_best, task, [2.0, 3.0])
            assert same_bits(vals, out[m, task][1]) and np.array_equal(idxs, out[m, task][2]), ("default schedule", m, task)
        close_sets(pair)
    return out


@pytest.mark.parametrize("schedule", ["1", "2"])
def test_one_launch_equals_the_per_set_calls_under_either_schedule(hip, zoo_answers, schedule, monkeypatch):
    from cbo_with_oop_amd import _lib
    monkeypatch.setenv("CBO_HIP_HYPER_SCHEDULE", schedule)
    ctx = _lib.Context(_lib.Context.get().device_id)                # (the schedule is read when a context is made)
    try:
        zoo = build_sets(hip, SHAPES, context=ctx)
        nine = zoo + [zoo[1], zoo[3], zoo[5]]
        for task in ("min", "max"):
            y_best, want_v, want_i, want_acq = zoo_answers["zoo", task]
            vals, idxs = sets_hyper_log(nine, y_best, task, ZOO_COSTS, jitter=0.01)
            assert same_bits(vals, want_v) and np.array_equal(idxs, want_i), (schedule, task)
            got_v, got_i, got_acq = per_set(zoo, y_best[:6], task, ZOO_COSTS[:6], jitter=0.01)
            assert same_bits(got_v, want_v[:6]) and np.array_equal(got_i, want_i[:6])
            assert all(same_bits(a, b) for a, b in zip(got_acq, want_acq))
        close_sets(zoo)
        for m, shapes in THRESHOLD_SHAPES.items():
            pair = build_sets(hip, shapes, context=ctx)
            for task in ("min", "max"):
                y_best, want_v, want_i, want_acq = zoo_answers[m, task]
                vals, idxs = sets_hyper_log(pair, y_best, task, [2.0, 3.0])
                assert same_bits(vals, want_v) and np.array_equal(idxs, want_i), (schedule, m, task)
                back = sets_hyper_log(pair[::-1], y_best[::-1], task, [3.0, 2.0])
                assert same_bits(back[0], want_v[::-1]) and np.array_equal(back[1], want_i[::-1])
                assert same_bits(hyper_log(pair[0].model, pair[0].grid, pair[0].rows, y_best[0], task, 2.0)[0], want_acq[0])
            close_sets(pair)
    finally:
        ctx.close()


# ---- 6. mixed routing and untouched models -----------------------------------------------------------------------------------
def test_mixed_routing_and_untouched_models(hip):
    """A model of 129 observations, an fp32 model and the jitter fixture under a sample that is not positive definite as
    assembled take the general path between small neighbours: each general-path set's answer is cbo_lse_rows over its twins'
    terms, each small set's its own call's bits, and nothing of the small models is touched."""
    from cbo_with_oop_amd import _lib
    f = load_fixture("jitter_ladder")
    own = samples_for(3, True, 1, seed=8)[0]

    def custom(X, y, Xs, rows, ard, causal, dtype=None, offset=0, fit=True, keep_solution=False):
        st = Set.__new__(Set)
        st.X, st.y, st.Xs, st.rows, st.ard, st.causal, st.dtype = X, y, Xs, np.ascontiguousarray(rows), ard, causal, dtype
        st.model = gp(X, y, own if ard else (1.0, 1.0, 1e-2), ard, causal, dtype, fit=fit)
        st.grid = hip.CandidateGrid(Xs, st.model, index_offset=offset, keep_solution=keep_solution)
        return st
    large = custom(*problem(129, 130, 3, seed=21), samples_for(3, True, 2, seed=21), True, True, offset=3)
    single = custom(*problem(40, 65, 2, seed=22), samples_for(2, False, 3, seed=22), False, False, dtype="f32")
    ladder = custom(f["X"], f["y"], f["Xs"], np.array([[1.0, 1.0, 1e-2], [1e12, 1.0, 0.0]]), False, False)
    warm = custom(*problem(40, 130, 3, seed=23), samples_for(3, True, 3, seed=23), True, True, keep_solution=True)
    cold = custom(*problem(17, 65, 3, seed=24), samples_for(3, True, 2, seed=24), True, True, offset=1000, fit=False)
    last = custom(*problem(64, 64, 1, seed=25), samples_for(1, False, 10, seed=25), False, True, fit=False)
    sets = [warm, large, single, cold, ladder, last]
    y_best = [float(st.y.min()) for st in sets]
    y_best[4] = float(f["y_best"])
    costs = [2.0, 3.0, 1.5, 0.5, 1.0, 3.7]
    ei = hip.CausalExpectedImprovement(y_best[0], "min", warm.model)
    before = ei.sweep(warm.grid, cost=2.0, want_acq=True, want_posterior=True)
    state = [np.array(v) for v in warm.model.posterior_state()]
    large_before = hip.CausalExpectedImprovement(y_best[1], "min", large.model).sweep(large.grid, cost=3.0, want_acq=True)
    with np.errstate(invalid="ignore"):
        vals, idxs = sets_hyper_log(sets, y_best, "min", costs)
    print(vals.tolist(), idxs.tolist())
    # the small sets: their own calls' bits; untouched -- an unfitted model stays unfitted
    for i in (0, 3, 5):
        acq, val, idx = hyper_log(sets[i].model, sets[i].grid, sets[i].rows, y_best[i], "min", costs[i])
        assert idxs[i] == idx and same_bits(vals[i], val), i
    for st in (cold, last):
        assert st.model.stale
        rc = _lib.load().cbo_acq_sweep(st.model._handle, st.grid._handle, 0.0, 0, 0.0, 1.0, None, None, None,
                                       ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int64()))
        assert rc == _lib.CBO_ERR_NOT_FITTED
    after = ei.sweep(warm.grid, cost=2.0, want_acq=True, want_posterior=True)
    for key in ("acq", "mean", "var"):
        assert np.array_equal(after[key], before[key])
    assert (after["best_val"], after["best_idx"]) == (before["best_val"], before["best_idx"])
    for u, v in zip(warm.model.posterior_state(), state):
        assert np.array_equal(np.array(u), v)
    assert not warm.model.stale
    assert warm.model.append(np.array([0.25, -0.5, 1.0]), 0.7)             # the kept solution still grows by one row
    # the general-path sets: cbo_lse_rows over the twins' terms, with the arg-max's tie rule
    for i in (1, 2, 4):
        st = sets[i]
        with np.errstate(invalid="ignore"):
            terms = twin_terms(hip, st.X, st.y, st.Xs, st.rows, y_best[i], "min", st.ard, st.causal, st.dtype)
            want = lse_rows(st.model._ctx, terms, costs[i])
            acq, val, idx = hyper_log(st.model, st.grid, st.rows, y_best[i], "min", costs[i])
        w = first_max(want)
        print("general path, set", i, "winner", w, want[w], "call", idxs[i], vals[i])
        assert np.array_equal(bits(acq), bits(want)) or (np.array_equal(np.isnan(acq), np.isnan(want))
                                                         and same_bits(acq[~np.isnan(acq)], want[~np.isnan(want)]))
        assert idxs[i] == w + st.grid.index_offset == idx and same_value(vals[i], want[w]) and same_value(val, want[w])
    # the large model is restored: hyper-parameters back, fitted again, the same answers
    large_after = hip.CausalExpectedImprovement(y_best[1], "min", large.model).sweep(large.grid, cost=3.0, want_acq=True)
    assert np.array_equal(large_after["acq"], large_before["acq"]) and not large.model.stale
    for st in sets:
        st.grid.close(); st.model.close()


# ---- 7. error returns ---------------------------------------------------------------------------------------------------------
def test_error_returns(hip):
    from cbo_with_oop_amd import _lib
    invalid = _lib.CBO_ERR_INVALID
    a, b = build_sets(hip, [(12, 20, 2, False, False, 2, 0), (17, 65, 3, True, True, 2, 0)])
    a.rows = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 0.0]])
    sets = [a, b]
    first = sets_hyper_log(sets, [0.0, 0.0], "min", [1.0, 2.0])
    nan, inf = float("nan"), float("inf")

    def refused(y_best=(0.0, 0.0), task="min", costs=(1.0, 2.0), jitter=0.0, rows=None):
        rc, vals, idxs = sets_hyper_log(sets, y_best, task, costs, jitter, rc_only=True, rows=rows)
        assert rc == invalid, (y_best, task, costs, jitter)
        assert np.all(vals == -7.0) and np.all(idxs == -7) and a.model.stale and b.model.stale
    # cbo_acq_sweep_sets_hyper's, and the log EI's scalars
    refused(task=2); refused(task=-1); refused(costs=(1.0, 0.0)); refused(costs=(-1.0, 1.0)); refused(costs=(1.0, nan))
    for bad in (nan, inf, -inf):
        refused(jitter=bad)
        refused(y_best=(0.0, bad))
        refused(y_best=(bad, 0.0))
    refused(rows=[a.rows, np.tile(b.rows[:1], (257, 1))])
    for col, bad in ((0, 0.0), (1, -1.0), (0, nan), (1, inf), (2, -1e-12), (2, nan)):
        rows = a.rows.copy()
        rows[1, col] = bad
        refused(rows=[rows, np.ascontiguousarray(b.rows)])
    plain_grid = hip.CandidateGrid(b.Xs)                             # a causal model needs the prior closures
    keep = b.grid
    b.grid = plain_grid
    refused()
    b.grid = keep
    # the single-set call
    for kw in (dict(jitter=nan), dict(jitter=inf), dict(y_best=nan), dict(y_best=-inf), dict(cost=0.0), dict(cost=nan)):
        args = dict(y_best=0.0, cost=1.0, jitter=0.0)
        args.update(kw)
        rc, acq, val, idx = hyper_single("cbo_acq_sweep_hyper_log", a.model, a.grid, a.rows, args["y_best"], "min", args["cost"],
                                         args["jitter"], rc_only=True)
        assert rc == invalid and np.all(acq == -7.0) and (val, idx) == (-7.0, -7) and a.model.stale, kw
    rows = a.rows.copy()
    rows[0, 1] = 0.0
    assert hyper_single("cbo_acq_sweep_hyper_log", a.model, a.grid, rows, 0.0, "min", 1.0, rc_only=True)[0] == invalid
    lib = _lib.load()
    out = np.full(3, -7.0)
    terms = np.zeros((2, 3))
    for n_rows, m, cost in ((0, 3, 1.0), (257, 3, 1.0), (2, 0, 1.0), (2, 3, 0.0), (2, 3, nan)):
        assert lib.cbo_lse_rows(a.model._ctx.handle, n_rows, m, _lib.dptr(terms), cost, _lib.dptr(out)) == invalid
    assert lib.cbo_lse_rows(a.model._ctx.handle, 2, 3, None, 1.0, _lib.dptr(out)) == invalid and np.all(out == -7.0)
    # nothing was left behind: the good call answers as before
    again = sets_hyper_log(sets, [0.0, 0.0], "min", [1.0, 2.0])
    assert same_bits(again[0], first[0]) and np.array_equal(again[1], first[1])
    plain_grid.close()
    close_sets(sets)


# ---- 8. the Python layer ------------------------------------------------------------------------------------------------------
def three_rows(model, s):
    """Three (variance, lengthscale, noise) rows for a factory model of the toy graph: a function of the set and of the
    model's row count alone (no draw from numpy's global generator), so that a twin of the same data gets the same rows."""
    return samples_for(1, False, 3, seed=17 * s + model.X.shape[0])


@pytest.mark.parametrize("cost_type", [1, 4])
def test_find_next_y_points_with_logmei_is_find_next_y_point_per_set(hip, cost_type):
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import find_next_y_point, find_next_y_points
    es, targets, xs, table = toy_problem(cost_type)
    ys = [t(x) for t, x in zip(targets, xs)]
    best = min(float(y.min()) for y in ys)
    models = [factory_model(xs[s], ys[s]) for s in range(2)]
    rows = [three_rows(models[s], s) for s in range(2)]
    grids = [CandidateGrid(meshgrid_candidates(ToyGraph.bounds(es[s]), [200]), models[s]) for s in range(2)]
    cache = {}
    for task in ("min", "max"):
        a_x, a_y = find_next_y_points(models, best, es, table, task, grids, cache=cache, hyper_samples=rows,
                                      acquisition="LOGMEI")
        ei_x, ei_y = find_next_y_points(models, best, es, table, task, grids, cache=cache, hyper_samples=rows)
        for s in range(2):
            twin = factory_model(xs[s], ys[s])
            y, x = find_next_y_point(ToyGraph.bounds(es[s]), twin, best, es[s], table, task=task, grid_shape=[200],
                                     hyper_samples=rows[s], acquisition="LOGMEI")
            print(task, s, a_y[s].tolist(), y.tolist(), a_x[s].tolist(), x.tolist(), "EI form", ei_y[s].tolist())
            assert np.array_equal(a_x[s], x) and same_bits(a_y[s], y)
            if task == "min" and cost_type == 1 and ei_y[s][0, 0] > 1e-290:       # (the logarithm of what the EI form averages)
                assert np.isclose(np.exp(a_y[s][0, 0]), ei_y[s][0, 0], rtol=1e-10)
            twin.close()
    assert cache["sweep_sets"]["kind"] == ("EI", None)
    for g in grids:
        g.close()
    for m in models:
        m.close()


def test_path_trials_with_logmei_pick_what_the_per_set_calls_pick(hip):
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import find_next_y_point
    es, targets, xs, table = toy_problem(4)
    ys = [t(x) for t, x in zip(targets, xs)]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys, [ToyGraph.bounds(s) for s in es],
                              grid_shapes=[[200], [200]], comm=None, hyper_samples=three_rows, acquisition="LOGMEI")
    path.update_all_gaussian_processes()
    for trial in range(3):
        best = min(float(ys[0].min()), float(ys[1].min()))
        a_x, a_y, (a_set, a_idx) = path.trial_step(best)
        b_x, b_y = [], []
        for s in range(2):
            twin = factory_model(xs[s], ys[s])
            y, x = find_next_y_point(ToyGraph.bounds(es[s]), twin, best, es[s], table, task="min", grid_shape=[200],
                                     hyper_samples=three_rows(twin, s), acquisition="LOGMEI")
            b_x.append(x); b_y.append(y)
            twin.close()
        b_idx = int(np.argmax([float(y[0, 0]) for y in b_y]))
        print("trial", trial, [y.tolist() for y in a_y], [y.tolist() for y in b_y])
        assert a_idx == b_idx and a_set == es[b_idx]
        assert all(np.array_equal(p, q) for p, q in zip(a_x, b_x))
        assert all(same_bits(p, q) for p, q in zip(a_y, b_y))
        assert "trial_args" not in path._call_cache["sweep_sets"]               # the three-call route
        xs[a_idx] = np.vstack([xs[a_idx], a_x[a_idx]])
        ys[a_idx] = np.vstack([ys[a_idx], targets[a_idx](a_x[a_idx])])


def test_the_agent_runs_with_logmei_and_chooses_what_a_path_with_the_same_rows_chooses(hip):
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model

    class Toy(ToyGraph):
        """The toy graph with what an observe step needs: its manipulative variables and one graph GP per set."""
        manipulative_variables = ("X", "Z")
        _fit_dependencies = (("X",), ("Z",))
        _fit_parameters = ([1.0, 1.0, 10.0, False], [1.0, 1.0, 10.0, False])

    sem = Toy.define_sem()
    rng = np.random.default_rng(11)
    draws = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(60)]
    obs = {v: np.array([r[v] for r in draws]) for v in draws[0] if not v.startswith("U")}
    init = {k: v[:40] for k, v in obs.items()}
    es, targets, xs, _ = toy_problem(1, n=6)
    data = [(xs[s].copy(), targets[s](xs[s])) for s in range(2)]
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(Toy, init, obs, data, exploration_set=es, num_trials=4, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64]], target_functions=targets,
                    hyper_samples=three_rows, acquisition="LOGMEI")
        mon = agent.run()
    assert len(mon.type_trial) == 4 and 1 in mon.type_trial
    assert agent._kind == ("LOGMEI", 0.0) and all(r is not None and r.shape[0] == 3 for r in agent.hyper_rows)
    chosen = [c for c in mon.chosen if c is not None]
    assert len(chosen) == sum(mon.type_trial)
    px, py = [d[0].copy() for d in data], [d[1].copy() for d in data]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, agent.costs, "min", px, py, [Toy.bounds(s) for s in es],
                              grid_shapes=[[64], [64]], comm=None, hyper_samples=three_rows, acquisition="LOGMEI")
    for picked_set, picked_x in chosen:
        best = min(float(py[0].min()), float(py[1].min()))
        path.update_all_gaussian_processes()
        xs_new, ys_new = path.compute_best_acquisition_values(best)
        a_set, a_idx = path.select_next_intervention(ys_new)
        print(picked_set, picked_x.tolist(), a_set, xs_new[a_idx].tolist(), [y.tolist() for y in ys_new])
        assert a_set == picked_set and np.array_equal(xs_new[a_idx], picked_x)
        px[a_idx] = np.vstack([px[a_idx], xs_new[a_idx]])
        py[a_idx] = np.vstack([py[a_idx], targets[a_idx](xs_new[a_idx])])
