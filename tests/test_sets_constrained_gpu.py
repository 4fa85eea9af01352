"""GPU tests of the constrained acquisition in the one-launch multi-set sweep and the agent:
cbo_acq_sweep_sets_constrained (small_sets_con_kernel, kernels_sets_con.hip) and the Python layer on top.

Every comparison is exact -- values as bit patterns (NaN equals NaN), indices equal -- and the reference is always the
per-set cbo_acq_sweep_constrained on freshly FITTED twin models, never the code under test.  Equality is the contract: the
launch runs kernel_value, the decoupled-wave block factorisation, the tile solve, posterior_of, acquisition_of and
feasibility_of (the stages cbo_small_device.h shares with small_sets_kernel) -- the general path's own device functions in the general path's summation orders -- model after model of a
set inside one workgroup, which is why the shapes walk n up and down and mix causal with plain models inside one set."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

INVALID, NOT_FITTED = -1, -5
LE, GE = 0, 1


@pytest.fixture(scope="module")
def lib():
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return _lib


def gp(X, y, **kw):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def mean_f(a):
    return 0.3 * np.sin(a).sum(1, keepdims=True)


def var_f(a):
    return 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2


class Pair:
    """One (model, candidate set) pair twice: the model under test (never fitted unless asked) with its grid, and the fitted
    twin with its own.  (tests/test_sets_kind_gpu.py's idea, copied.)"""

    def __init__(self, n, cand, causal=False, ard=False, offset=0, seed=0, shift=0.0, kw=None, data=None, fit=False):
        from cbo_with_oop_amd import CandidateGrid
        m, d = cand.shape
        rng = np.random.default_rng(1000 * n + 10 * m + d + seed)
        X = rng.uniform(-2.0, 2.0, (n, d)) if data is None else data[0]
        y = shift + np.cos(X + 0.3 * seed).sum(1, keepdims=True) + 0.05 * rng.standard_normal((n, 1)) if data is None else data[1]
        if kw is None:
            kw = dict(variance=1.3, lengthscale=(0.7 + 0.2 * np.arange(d)) if ard else 0.9, ard=ard, noise_var=1e-3)
            if causal:
                kw.update(mean_function=mean_f, variance_adjustment=var_f)
        self.model, self.twin = gp(X, y, fit=fit, **kw), gp(X, y, **kw)
        self.grid = CandidateGrid(cand, self.model, index_offset=offset)
        self.twin_grid = CandidateGrid(cand, self.twin, index_offset=offset)

    def close(self):
        for o in (self.grid, self.twin_grid, self.model, self.twin):
            o.close()


class ConSet:
    """One exploration set: the objective's pair and the constraints' pairs over the same candidate points, with each
    constraint's (value, jitter, sense)."""

    def __init__(self, n, con_n, m, d, causal=False, con_causal=False, con_ard=False, ard=False, offset=0, seed=0, senses=None,
                 values=None, objective=None, constraints=None, cand=None):
        rng = np.random.default_rng(7919 * n + 31 * m + d + seed)
        self.cand = rng.uniform(-2.5, 2.5, (m, d)) if cand is None else cand
        self.obj = objective(self.cand) if objective else Pair(n, self.cand, causal=causal, ard=ard, offset=offset, seed=seed)
        if constraints:
            self.cons = [c(self.cand) for c in constraints]
        else:
            self.cons = [Pair(cn, self.cand, causal=con_causal, ard=con_ard, offset=offset, seed=seed + 1 + k)
                         for k, cn in enumerate(con_n)]
        k = len(self.cons)
        # bounds inside the constrained nodes' range (cos sums in [-d, d]): no probability of feasibility is 0 or 1 everywhere
        self.values = np.asarray(values if values is not None else [0.2 * d * np.cos(1.0 + c) for c in range(k)], dtype=np.float64)
        self.jitters = np.asarray([0.01 * (c % 2) for c in range(k)], dtype=np.float64)
        self.senses = np.asarray(senses if senses is not None else [c % 2 for c in range(k)], dtype=np.int32)

    def pairs(self):
        return [self.obj] + self.cons

    def close(self):
        for p in self.pairs():
            p.close()


def handles(objs):
    return (ctypes.c_void_p * max(len(objs), 1))(*[o._handle for o in objs])


def sweep_sets_constrained(lib, sets, y_best, task, costs, jitter=0.0, twins=False):
    """cbo_acq_sweep_sets_constrained: (rc, values, indices)."""
    s = len(sets)
    model = (lambda p: p.twin) if twins else (lambda p: p.model)
    grid = (lambda p: p.twin_grid) if twins else (lambda p: p.grid)
    yb = np.ascontiguousarray(np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)))
    cs = np.ascontiguousarray(np.broadcast_to(np.asarray(costs, dtype=np.float64), (s,)))
    n_con = np.array([len(st.cons) for st in sets], dtype=np.int32)
    cons = [c for st in sets for c in st.cons]
    values = np.concatenate([st.values for st in sets] + [np.zeros(0)])
    jitters = np.concatenate([st.jitters for st in sets] + [np.zeros(0)])
    senses = np.concatenate([st.senses for st in sets] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    none = len(cons) == 0
    rc = lib.load().cbo_acq_sweep_sets_constrained(
        s, handles([model(st.obj) for st in sets]), handles([grid(st.obj) for st in sets]), lib.dptr(yb),
        lib.TASK_CODE.get(task, task), float(jitter), lib.dptr(cs), n_con.ctypes.data_as(lib.c_int_p),
        None if none else handles([model(c) for c in cons]), None if none else handles([grid(c) for c in cons]),
        None if none else lib.dptr(values), None if none else lib.dptr(jitters),
        None if none else senses.ctypes.data_as(lib.c_int_p), lib.dptr(vals), idxs.ctypes.data_as(lib.c_int64_p))
    return rc, vals, idxs


def per_set(lib, sets, y_best, task, costs, jitter=0.0):
    """The reference: cbo_acq_sweep_constrained set by set on fitted twins."""
    s = len(sets)
    yb, cs = np.broadcast_to(np.asarray(y_best, dtype=np.float64), (s,)), np.broadcast_to(np.asarray(costs, float), (s,))
    vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
    for i, st in enumerate(sets):
        for p in st.pairs():
            p.twin.ensure_fitted()
        k = len(st.cons)
        senses = (ctypes.c_int * max(k, 1))(*[int(v) for v in st.senses])
        bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
        lib.check(lib.load().cbo_acq_sweep_constrained(
            st.obj.twin._handle, st.obj.twin_grid._handle, float(yb[i]), lib.TASK_CODE[task], float(jitter), float(cs[i]), k,
            handles([c.twin for c in st.cons]) if k else None, handles([c.twin_grid for c in st.cons]) if k else None,
            lib.dptr(np.ascontiguousarray(st.values)) if k else None, lib.dptr(np.ascontiguousarray(st.jitters)) if k else None,
            senses if k else None, None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
        vals[i], idxs[i] = bv.value, bi.value
    return vals, idxs


def assert_same(got, want, what=""):
    (gv, gi), (wv, wi) = got, want
    print(what, "values", gv.tolist(), "reference", wv.tolist(), "indices", gi.tolist(), "reference", wi.tolist())
    assert np.array_equal(gi, wi), (what, gi, wi)
    assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)), (what, gv, wv)


def check_call(lib, sets, y_best, task, costs, what="", jitter=0.0):
    rc, vals, idxs = sweep_sets_constrained(lib, sets, y_best, task, costs, jitter)
    lib.check(rc)
    assert_same((vals, idxs), per_set(lib, sets, y_best, task, costs, jitter), what)
    return vals, idxs


def fitted(lib, model):
    out = np.empty(1)
    rc = lib.load().cbo_gp_log_marginal(model._handle, lib.dptr(out))
    assert rc in (0, NOT_FITTED), rc
    return rc == 0


# ---- the kernel's edges ----------------------------------------------------------------------------------------------------
# (objective n; constraint n's; m; d).  n walks up and down across 16-row tile boundaries inside one workgroup, causal and
# plain models alternate inside a set; m: 64 candidates per workgroup; 704 / 705 candidates: 11 and 12 workgroups per set, the
# two sides of the one- / two-launch split (the widest set of a call decides for the call)
ONE_LAUNCH = [dict(n=1, con_n=[], m=1, d=1),
              dict(n=17, con_n=[128, 1], m=65, d=2, causal=True),
              dict(n=128, con_n=[15], m=63, d=3, con_causal=True, con_ard=True),
              dict(n=16, con_n=[16] * 8, m=64, d=8, offset=5000),
              dict(n=50, con_n=[50, 50], m=200, d=1, causal=True, con_causal=True),
              dict(n=128, con_n=[128], m=704, d=2)]
TWO_LAUNCHES = [dict(n=128, con_n=[17, 128, 1], m=705, d=3),
                dict(n=17, con_n=[50] * 8, m=1, d=1)]


@pytest.fixture(scope="module")
def zoo(lib):
    groups = {"one launch": [ConSet(**kw) for kw in ONE_LAUNCH], "two launches": [ConSet(**kw) for kw in TWO_LAUNCHES]}
    yield groups
    for sets in groups.values():
        for st in sets:
            st.close()


@pytest.mark.parametrize("task", ["min", "max"])
def test_shapes(lib, zoo, task):
    for what, sets in zoo.items():
        s = len(sets)
        # inside the targets' range; for 'max' (the reference's quirk: -EI with the same u) well above it, so that the
        # winner is the smallest of EIs that are all far from zero, not one of many zeros
        y_best = np.linspace(-0.4, 0.6, s) + (3.0 if task == "max" else 0.0)
        costs = 1.0 + np.arange(s) % 3
        vals, _ = check_call(lib, sets, y_best, task, costs, f"{task} {what}", jitter=0.01)
        assert np.all(np.isfinite(vals)) and np.any(vals != 0.0)
        # the launch needs no fit and leaves the models alone
        assert not any(fitted(lib, p.model) for st in sets for p in st.pairs()), "a model was fitted"


# ---- more than 8 pairs: the descriptors are read from the pinned array --------------------------------------------------------
def test_twenty_five_sets(lib):
    sets = [ConSet(50, [50] * (sidx % 4), 200, 1 + sidx % 2, causal=sidx % 3 == 1, con_causal=sidx % 5 == 2, seed=sidx)
            for sidx in range(25)]
    costs = [1.0 + s % 3 for s in range(25)]
    for task in ("min", "max"):
        check_call(lib, sets, 0.1, task, costs, f"25 sets {task}")
    assert not any(fitted(lib, p.model) for st in sets for p in st.pairs())
    for st in sets:
        st.close()


# ---- mixed routing, repeatability and re-arming ------------------------------------------------------------------------------
def fixture_kwargs(f):
    ls = f["lengthscale_arg"]
    kw = dict(variance=float(f["variance"]), lengthscale=ls, ard=not np.isscalar(ls), noise_var=float(f["noise_var"]))
    if f["mX"] is not None:
        lut_m = {**{tuple(r): v for r, v in zip(map(tuple, f["X"]), f["mX"][:, 0])},
                 **{tuple(r): v for r, v in zip(map(tuple, f["Xs"]), f["mXs"][:, 0])}}
        lut_v = {**{tuple(r): v for r, v in zip(map(tuple, f["X"]), f["vX"][:, 0])},
                 **{tuple(r): v for r, v in zip(map(tuple, f["Xs"]), f["vXs"][:, 0])}}
        kw["mean_function"] = lambda a: np.array([[lut_m[tuple(r)]] for r in a])
        kw["variance_adjustment"] = lambda a: np.array([[lut_v[tuple(r)]] for r in a])
    return kw


def mixed_sets():
    """A 200-observation objective; a small objective with a 200-observation constraint; a set one of whose constraint
    models has duplicate rows (its factorisation needs jitchol's jitter: the general path takes over for that set); a set
    with an fp32 model; two ordinary small sets.  Returns (sets, which of them the one launch keeps)."""
    fj = load_fixture("jitter_ladder")
    rng = np.random.default_rng(3)
    Xb = rng.uniform(-2, 2, (200, 3))
    yb = np.cos(Xb).sum(1, keepdims=True)
    Xf = rng.uniform(-2, 2, (60, 3))
    yf = np.sin(Xf).sum(1, keepdims=True)
    big = lambda cand: Pair(200, cand, kw=dict(noise_var=1e-3), data=(Xb, yb))                      # noqa: E731
    f32 = lambda cand: Pair(60, cand, kw=dict(noise_var=1e-2, dtype="f32"), data=(Xf, yf))          # noqa: E731
    small = lambda n, seed: (lambda cand: Pair(n, cand, seed=seed))                                # noqa: E731
    ladder = lambda cand: Pair(len(fj["X"]), cand, kw=fixture_kwargs(fj), data=(fj["X"], fj["y"]))  # noqa: E731
    dj = fj["X"].shape[1]
    sets = [ConSet(0, None, 300, 3, objective=big, constraints=[small(40, 1)]),
            ConSet(0, None, 300, 3, objective=small(33, 2), constraints=[small(20, 3), big]),
            ConSet(0, None, len(fj["Xs"]), dj, objective=small(25, 4), constraints=[small(31, 5), ladder], cand=fj["Xs"],
                   values=[0.1, float(np.median(fj["y"]))]),
            ConSet(0, None, 300, 3, objective=small(48, 6), constraints=[f32]),
            ConSet(50, [17, 64], 130, 2, causal=True, seed=7),
            ConSet(30, [], 90, 3, seed=8)]
    return sets, [False, False, False, False, True, True]


def test_mixed_routing_repeatability_and_rearming(lib):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sets, one_launch = mixed_sets()
        costs = [2.0, 1.0, 3.0, 3.0, 1.0, 2.0]
        rc, vals, idxs = sweep_sets_constrained(lib, sets, 0.1, "min", costs)
        lib.check(rc)
        want = per_set(lib, sets, 0.1, "min", costs)
        assert_same((vals, idxs), want, "mixed")
        assert sets[2].cons[1].twin.jitter_tries >= 1                               # that set did need the ladder
        for st, kept in zip(sets, one_launch):
            for p in st.pairs():
                assert fitted(lib, p.model) == (not kept), "one-launch models stay unfitted, general-path models are fitted"
        # the same call again: the same bits (the general-path sets now from fitted models)
        rc, vals2, idxs2 = sweep_sets_constrained(lib, sets, 0.1, "min", costs)
        lib.check(rc)
        assert_same((vals2, idxs2), want, "mixed, again")
        # right after a call that met the ladder (its status word was re-armed): small sets alone, twice
        fj = load_fixture("jitter_ladder")
        ladder_set = [ConSet(0, None, len(fj["Xs"]), fj["X"].shape[1], cand=fj["Xs"],
                             objective=lambda cand: Pair(25, cand, seed=4),
                             constraints=[lambda cand: Pair(len(fj["X"]), cand, kw=fixture_kwargs(fj), data=(fj["X"], fj["y"]))],
                             values=[float(np.median(fj["y"]))])]
        rc, lv, li = sweep_sets_constrained(lib, ladder_set, 0.1, "min", [1.0])      # meets the ladder in the launch
        lib.check(rc)
        assert_same((lv, li), per_set(lib, ladder_set, 0.1, "min", [1.0]), "the ladder set alone")
        smalls = sets[4:]
        first = sweep_sets_constrained(lib, smalls, 0.1, "min", costs[4:])
        second = sweep_sets_constrained(lib, smalls, 0.1, "min", costs[4:])
        assert first[0] == 0 and second[0] == 0
        assert_same(first[1:], (want[0][4:], want[1][4:]), "after the ladder")
        assert_same(second[1:], first[1:], "after the ladder, again")
    for st in sets + ladder_set:
        st.close()


# ---- fitted small models are not touched --------------------------------------------------------------------------------------
def plain_sweep(lib, g, grid, y_best, task, jitter, cost):
    bv, bi = ctypes.c_double(), ctypes.c_int64(-1)
    lib.check(lib.load().cbo_acq_sweep(g._handle, grid._handle, float(y_best), lib.TASK_CODE[task], float(jitter),
                                       float(cost), None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
    return bv.value, bi.value


def test_fitted_models_with_cached_sweeps_are_untouched(lib):
    sets = [ConSet(40, [23, 50], 150, 2, causal=True, seed=1), ConSet(64, [], 70, 2, seed=2)]
    # the twins are fitted: they serve as the models of the call here
    pairs = [p for st in sets for p in st.pairs()]
    before = [plain_sweep(lib, p.twin, p.twin_grid, 0.2, "min", 0.0, 2.0) for p in pairs]
    want = per_set(lib, sets, 0.1, "max", [1.0, 3.0])
    rc, vals, idxs = sweep_sets_constrained(lib, sets, 0.1, "max", [1.0, 3.0], twins=True)
    lib.check(rc)
    assert_same((vals, idxs), want, "fitted models")
    assert all(fitted(lib, p.twin) for p in pairs)
    after = [plain_sweep(lib, p.twin, p.twin_grid, 0.2, "min", 0.0, 2.0) for p in pairs]
    assert [(np.float64(v).view(np.uint64), i) for v, i in before] == [(np.float64(v).view(np.uint64), i) for v, i in after]
    for st in sets:
        st.close()


# ---- edges ----------------------------------------------------------------------------------------------------------------------
def test_nan_prior_mean_at_a_candidate_of_a_constraint(lib):
    """A NaN prior mean at two candidates of a constraint's set: the product is NaN there, NaN is maximal, the lowest index
    wins -- in the one launch and in the two."""
    for m in (150, 800):
        cand = np.random.default_rng(m).uniform(-2.5, 2.5, (m, 2))
        bad = cand[[37, 90]].copy()

        def mf(a):
            out = mean_f(a)
            out[np.all(a[:, None, :] == bad[None, :, :], axis=2).any(axis=1)] = np.nan
            return out
        kw = dict(variance=1.3, lengthscale=0.9, noise_var=1e-3, mean_function=mf, variance_adjustment=var_f)
        sets = [ConSet(0, None, m, 2, cand=cand, offset=11, objective=lambda c: Pair(40, c, offset=11, seed=1),
                       constraints=[lambda c: Pair(20, c, offset=11, seed=2), lambda c: Pair(30, c, offset=11, seed=3, kw=kw)]),
                ConSet(30, [30], 100, 2, seed=5)]
        for task in ("min", "max"):
            vals, idxs = check_call(lib, sets, 0.1, task, [2.0, 1.0], f"NaN prior mean {task} m={m}")
            assert np.isnan(vals[0]) and idxs[0] == 37 + 11 and np.isfinite(vals[1])
        for st in sets:
            st.close()


def test_a_bound_no_candidate_can_meet(lib):
    """Every probability of feasibility is exactly zero: every product is a zero -- whose sign the 'max' task's quirk flips --
    and the winner is the reference's, sign included."""
    sets = [ConSet(40, [25, 33], 150, 2, seed=1, values=[0.3, -1e6], senses=[LE, LE], offset=3),
            ConSet(40, [25], 800, 2, seed=2, values=[1e6], senses=[GE])]
    for group in (sets[:1], sets):                            # the one launch, then the two
        for task in ("min", "max"):
            k = len(group)
            vals, idxs = check_call(lib, group, 0.1, task, [3.0, 2.0][:k], f"all zeros {task} {k}")
            assert np.all(vals == 0.0)
            assert idxs.tolist() == [3, 0][:k]
    for st in sets:
        st.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_models_untouched(lib):
    from cbo_with_oop_amd import CandidateGrid
    L = lib.load()
    sets = [ConSet(20, [33], 100, 2, causal=True, con_causal=True), ConSet(33, [], 100, 2)]
    models = [p.model for st in sets for p in st.pairs()]

    def untouched():
        return [L.cbo_gp_n(m._handle) for m in models] == [20, 33, 33] and not any(fitted(lib, m) for m in models)

    s = 2
    yb, cs = np.full(s, 0.1), np.array([1.0, 2.0])
    n_con = np.array([1, 0], dtype=np.int32)
    value, jitter, sense = sets[0].values.copy(), sets[0].jitters.copy(), sets[0].senses.copy()
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    shorter = Pair(33, sets[0].cand[:99], causal=True)                   # a constraint's set of another size
    plain_grid = CandidateGrid(sets[0].cand, sets[1].obj.model)            # no prior: a causal model cannot use it

    def call(**over):
        a = dict(n_sets=s, gps=handles([st.obj.model for st in sets]), cands=handles([st.obj.grid for st in sets]),
                 y_best=lib.dptr(yb), task=0, ei_jitter=0.0, costs=lib.dptr(cs), n_con=n_con.ctypes.data_as(lib.c_int_p),
                 con_gps=handles([sets[0].cons[0].model]), con_cands=handles([sets[0].cons[0].grid]),
                 con_value=lib.dptr(value), con_jitter=lib.dptr(jitter), con_sense=sense.ctypes.data_as(lib.c_int_p),
                 best_vals=lib.dptr(vals), best_idxs=idxs.ctypes.data_as(lib.c_int64_p))
        a.update(over)
        return L.cbo_acq_sweep_sets_constrained(*a.values())

    def refused(what, **over):
        assert call(**over) == INVALID and L.cbo_last_error(), what
        assert np.all(vals == -7.0) and np.all(idxs == -7) and untouched(), what

    refused("n_sets", n_sets=0)
    for name in ("gps", "cands", "y_best", "costs", "n_con", "con_gps", "con_cands", "con_value", "con_jitter", "con_sense",
                 "best_vals", "best_idxs"):
        refused(name, **{name: None})
    for task in (2, -1):
        refused("task", task=task)
    for bad in ((0.0, 1.0), (1.0, -1.0), (1.0, np.nan)):
        refused("costs", costs=lib.dptr(np.array(bad)))
    for bad in ((9, 0), (-1, 0), (1, 9)):
        refused("n_con", n_con=np.array(bad, dtype=np.int32).ctypes.data_as(lib.c_int_p))
    for bad in (np.nan, np.inf):
        refused("con_value", con_value=lib.dptr(np.array([bad])))
        refused("con_jitter", con_jitter=lib.dptr(np.array([bad])))
    refused("con_sense", con_sense=np.array([2], dtype=np.int32).ctypes.data_as(lib.c_int_p))
    refused("a NULL handle", gps=(ctypes.c_void_p * 2)(sets[0].obj.model._handle, None))
    refused("a NULL constraint handle", con_cands=(ctypes.c_void_p * 1)(None))
    refused("sets whose m differ", con_gps=handles([shorter.model]), con_cands=handles([shorter.grid]))
    refused("a causal model without prior", con_cands=handles([plain_grid]))
    refused("one candidate set with two models", con_cands=handles([sets[0].obj.grid]))
    # the refusals left the valid call working
    assert call() == 0
    assert_same((vals, idxs), per_set(lib, sets, 0.1, "min", cs), "valid call")
    shorter.close(); plain_grid.close()
    for st in sets:
        st.close()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def toy_problem(cost_type, n=12, seed=4):
    """The toy graph's two exploration sets with the target's data and, as the constrained node, a smooth function of the
    intervention values (observed at the same rows)."""
    from cbo_with_oop_amd.graphs import ToyGraph
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    nodes = [lambda x: np.sin(0.7 * x) + 0.1 * x, lambda z: np.cos(0.3 * z) - 0.02 * z]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-5, 5, (n, 1)), rng.uniform(-5, 20, (n, 1))]
    return es, targets, nodes, xs, ToyGraph.get_cost_structure(cost_type)


def factory_model(x, y):
    from cbo_with_oop_amd import GaussianProcessType
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory as GPFactory
    return GPFactory.create(GaussianProcessType.NON_CAUSAL_GP, x, y, [None, None], emukit_wrapper=True)


@pytest.mark.parametrize("cost_type", [1, 4])
def test_find_next_y_points_with_constraints_is_find_next_y_point_per_set(lib, cost_type):
    """One call for both sets -- set 0 with two constraints, set 1 with one -- against find_next_y_point(constraints=[...])
    set by set on twin models: points and values exact; with the variable cost table (4) every winner is re-evaluated at its
    own cost."""
    from cbo_with_oop_amd import CandidateGrid, ProbabilityOfFeasibility
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import find_next_y_point, find_next_y_points
    es, targets, nodes, xs, table = toy_problem(cost_type)
    ys = [t(x) for t, x in zip(targets, xs)]
    best = min(float(y.min()) for y in ys)
    spec = [[("<=", 0.4, 0.0), (">=", -0.8, 0.01)], [("<=", 0.6, 0.0)]]

    def build():
        models = [factory_model(xs[s], ys[s]) for s in range(2)]
        cons = [[ProbabilityOfFeasibility(factory_model(xs[s], nodes[s](xs[s]) + 0.1 * c), jitter, value, sense=sense)
                 for c, (sense, value, jitter) in enumerate(spec[s])] for s in range(2)]
        return models, cons
    models, cons = build()
    grids = [CandidateGrid(meshgrid_candidates(ToyGraph.bounds(es[s]), [200]), models[s]) for s in range(2)]
    cache = {}
    for task in ("min", "max"):
        a_x, a_y = find_next_y_points(models, best, es, table, task, grids, cache=cache, constraints=cons)
        twins, twin_cons = build()
        for s in range(2):
            y, x = find_next_y_point(ToyGraph.bounds(es[s]), twins[s], best, es[s], table, task=task, grid_shape=[200],
                                     constraints=twin_cons[s])
            print(task, s, a_y[s].tolist(), y.tolist(), a_x[s].tolist(), x.tolist())
            assert np.array_equal(a_x[s], x)
            assert np.array_equal(a_y[s].view(np.uint64), y.view(np.uint64))
    # the constraint models' grids were built once and kept
    kept = cache["sweep_sets"]["con_grids"]
    assert sorted(kept) == [(0, 0), (0, 1), (1, 0)]
    before = {k: v[1] for k, v in kept.items()}
    find_next_y_points(models, best, es, table, "min", grids, cache=cache, constraints=cons)
    assert all(cache["sweep_sets"]["con_grids"][k][1] is g for k, g in before.items())


def test_path_trials_with_a_constraint_pick_what_the_per_set_calls_pick(lib):
    """Three trials of CBOAcquisitionPath.trial_step with one constraint against the loop composed of the per-set calls
    (find_next_y_point(constraints=[...]) on fresh models, then the first maximum): same pick, points and values."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType, ProbabilityOfFeasibility
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import find_next_y_point
    es, targets, nodes, xs, table = toy_problem(4)
    ys = [t(x) for t, x in zip(targets, xs)]
    cs = [[n(x)] for n, x in zip(nodes, xs)]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys, [ToyGraph.bounds(s) for s in es],
                              grid_shapes=[[200], [200]], comm=None, constraints=[("node", "<=", 0.5, 0.01)],
                              constraint_data_y=cs)
    path.update_all_gaussian_processes()
    with pytest.raises(ValueError, match="single process"):
        class Two:
            world, rank = 2, 0
        other = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys,
                                   [ToyGraph.bounds(s) for s in es], comm=Two(), constraints=[("node", "<=", 0.5)],
                                   constraint_data_y=cs)
        other.compute_best_acquisition_values(0.0)
    for trial in range(3):
        best = min(float(ys[0].min()), float(ys[1].min()))
        a_x, a_y, (a_set, a_idx) = path.trial_step(best)
        b_x, b_y = [], []
        for s in range(2):
            twin, con = factory_model(xs[s], ys[s]), factory_model(xs[s], cs[s][0])
            y, x = find_next_y_point(ToyGraph.bounds(es[s]), twin, best, es[s], table, task="min", grid_shape=[200],
                                     constraints=[ProbabilityOfFeasibility(con, 0.01, 0.5)])
            b_x.append(x); b_y.append(y)
            twin.close(); con.close()
        b_idx = int(np.argmax([float(y[0, 0]) for y in b_y]))
        print("trial", trial, [y.tolist() for y in a_y], [y.tolist() for y in b_y])
        assert a_idx == b_idx and a_set == es[b_idx]
        assert all(np.array_equal(p, q) for p, q in zip(a_x, b_x))
        assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(a_y, b_y))
        assert "trial_args" not in path._call_cache["sweep_sets"]               # the three-call route
        xs[a_idx] = np.vstack([xs[a_idx], a_x[a_idx]])
        ys[a_idx] = np.vstack([ys[a_idx], targets[a_idx](a_x[a_idx])])
        cs[a_idx][0] = np.vstack([cs[a_idx][0], nodes[a_idx](a_x[a_idx])])
    for s in range(2):
        assert [m.X.shape[0] for m in path.constraint_models[s]] == [path.models[s].X.shape[0]] == [xs[s].shape[0] - (s == a_idx)]


def test_the_agent_runs_with_a_constraint(lib):
    """CBO(CompleteGraph, ..., constraints={"C": ...}, num_trials=5).run(): every constraint model has as many rows as its
    objective, the monitor holds one ``feasible`` entry per trial (None for an observe)."""
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import compute_interventions, sample_from_model
    sem = CompleteGraph.define_sem()
    rng = np.random.default_rng(11)
    rows = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(60)]
    obs = {v: np.array([r[v] for r in rows]) for v in rows[0] if not v.startswith("U")}
    init = {k: v[:40] for k, v in obs.items()}
    es = [["B"], ["D"], ["B", "D"]]
    data = []
    for s in es:
        lo, hi = np.array(CompleteGraph.bounds(s)).T
        x = rng.uniform(lo, hi, (5, len(s)))
        data.append((x, compute_interventions(sem, {v: "" for v in s}, x, target_variable="Y")))
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        agent = CBO(CompleteGraph, init, obs, data, exploration_set=es, num_trials=5, initial_num_obs_samples=40,
                    num_additional_observations=10, grid_shapes=[[64], [64], [16, 16]],
                    constraints={"C": ("<=", 2.0), "A": (">=", -1.0, 0.01)})
        mon = agent.run()
    assert len(mon.type_trial) == 5 and 1 in mon.type_trial
    assert len(mon.feasible) == 5 and len(mon.constraint_values) == 5
    for kind, feasible, values in zip(mon.type_trial, mon.feasible, mon.constraint_values):
        assert (feasible is None) == (kind == 0) and (values is None) == (kind == 0)
        if kind == 1:
            assert sorted(values) == ["A", "C"] and feasible == (values["C"] <= 2.0 and values["A"] >= -1.0)
    for s in range(len(es)):
        assert len(agent.constraint_models[s]) == 2
        for c, model in enumerate(agent.constraint_models[s]):
            assert model.X.shape[0] == agent.models[s].X.shape[0] == agent.data_x[s].shape[0]
            assert agent.constraint_data_y[s][c].shape == (agent.data_x[s].shape[0], 1)
    assert sum(x.shape[0] for x in agent.data_x) == 15 + sum(mon.type_trial)
