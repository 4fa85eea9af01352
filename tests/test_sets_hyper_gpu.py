"""GPU tests of the hyper-parameter-marginalised causal EI in the one-launch multi-set sweep and the agent
(cbo_acq_sweep_sets_hyper, hyper_sets_kernel).

The contract is stated against the single-set call: for every set of a call, winner value and index are bit for bit what
cbo_acq_sweep_hyper returns for that set alone (tests/test_hyper_gpu.py ties that call to the per-sample route and to the
oracle).  Accuracy is judged once more, directly, by conftest.assert_parity against the mean over the samples of the fp64
oracle with the 80-bit arbiter.

Shapes: n in {1, 10, 17, 50, 64, 128} (17: two tiles, a ragged last one; 128: a full block; 1: one row), m in {1, 64, 65,
130, 200} (sets narrower than the call's widest: their spare workgroups only hand in an empty winner), 704 and 768 (11 and
12 candidate blocks: either side of the two-launch threshold), d in {1, 2, 3, 8}, ARD and not, causal and plain, both tasks,
index offsets, H in {1, 2, 3, 10}, three sets (descriptors by value) and nine (from the pinned array)."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import assert_parity, load_fixture
from oracle import gp_oracle as O
from oracle.truth import truth_predict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import cbo_with_oop_amd as pkg
    from cbo_with_oop_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: -m gpu tests need an MI355X"
    return pkg


def prior_mean(x):
    return 0.3 * np.sum(x, axis=1, keepdims=True)


def prior_var(x):
    return 0.2 + 0.1 * np.square(x[:, :1])


def problem(n, m, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.0, 2.0, (m, d))
    return X, y, Xs


def samples_for(d, ard, H, seed, own_first=False):
    """H rows of (variance, lengthscale x L, noise) spread by a factor of about 2 around (1.3, 0.8.., 2e-2); noise >= 1e-2."""
    rng = np.random.default_rng(1000 + seed)
    L = d if ard else 1
    base = np.concatenate([[1.3], np.linspace(0.8, 1.1, L), [2e-2]])
    rows = base * 2.0 ** rng.uniform(-1.0, 1.0, (H, L + 2))
    rows[:, -1] = np.maximum(rows[:, -1], 1e-2)
    if own_first:
        rows[0] = base
    return np.ascontiguousarray(rows)


def make_model(X, y, row, ard, causal, fit=True):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    kw = dict(variance=float(row[0]), lengthscale=row[1:-1].copy() if ard else float(row[1]), ard=ard,
              noise_var=float(row[-1]), fit=fit)
    if causal:
        kw.update(mean_function=prior_mean, variance_adjustment=prior_var)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return HipGaussianProcess(X, y, **kw)


def first_argmax(v):
    """numpy.argmax: the first maximum, NaN maximal."""
    return int(np.argmax(v))


class Set:
    """One exploration set of a call: an (unfitted unless said) model, its candidate grid, its samples."""

    def __init__(self, hip, n, m, d, ard, causal, H, offset, seed=0, fit=False, own_first=False, keep_solution=False):
        self.shape = (n, m, d, ard, causal, H, offset)
        self.X, self.y, self.Xs = problem(n, m, d, seed=n + m + seed)
        self.rows = samples_for(d, ard, H, seed=n + seed, own_first=own_first)
        self.ard, self.causal = ard, causal
        self.model = make_model(self.X, self.y, self.rows[0], ard, causal, fit=fit)
        self.grid = hip.CandidateGrid(self.Xs, self.model, index_offset=offset, keep_solution=keep_solution)

    def close(self):
        self.grid.close(); self.model.close()


def handles(objs):
    return (ctypes.c_void_p * len(objs))(*[o._handle for o in objs])


def sets_hyper(sets, y_best, task, costs, rows=None, jitter=0.0, rc_only=False):
    """cbo_acq_sweep_sets_hyper over `sets`: (values, indices)."""
    from cbo_with_oop_amd import _lib
    s = len(sets)
    rows = [st.rows for st in sets] if rows is None else rows
    vals, idxs = np.full(s, -7.0), np.full(s, -7, dtype=np.int64)
    counts = (ctypes.c_int * s)(*[r.shape[0] for r in rows])
    ptrs = (ctypes.c_void_p * s)(*[r.ctypes.data for r in rows])
    rc = _lib.load().cbo_acq_sweep_sets_hyper(
        s, handles([st.model for st in sets]), handles([st.grid for st in sets]), counts, ptrs,
        _lib.dptr(np.asarray(y_best, dtype=np.float64)), _lib.TASK_CODE[task], jitter,
        _lib.dptr(np.asarray(costs, dtype=np.float64)), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p))
    if rc_only:
        return rc
    _lib.check(rc)
    return vals, idxs


def single_hyper(st, y_best, task, cost, rows=None, jitter=0.0, want_acq=False):
    """cbo_acq_sweep_hyper for one set alone: (value, index[, acq])."""
    from cbo_with_oop_amd import _lib
    rows = st.rows if rows is None else rows
    acq = np.empty(st.Xs.shape[0]) if want_acq else None
    val, idx = ctypes.c_double(), ctypes.c_int64()
    _lib.check(_lib.load().cbo_acq_sweep_hyper(st.model._handle, st.grid._handle, rows.shape[0], _lib.dptr(rows), float(y_best),
                                               _lib.TASK_CODE[task], jitter, float(cost), _lib.dptr(acq), ctypes.byref(val),
                                               ctypes.byref(idx)))
    return (val.value, idx.value, acq) if want_acq else (val.value, idx.value)


def assert_per_set(sets, y_best, task, costs, what=""):
    """One call against the single-set calls, bit for bit; the same call again gives the same bits."""
    vals, idxs = sets_hyper(sets, y_best, task, costs)
    want = [single_hyper(st, y_best[i], task, costs[i]) for i, st in enumerate(sets)]
    want_v, want_i = np.array([w[0] for w in want]), np.array([w[1] for w in want], dtype=np.int64)
    print(what, task, "values", vals.tolist(), "indices", idxs.tolist())
    assert np.array_equal(idxs, want_i), (what, idxs, want_i)
    assert np.array_equal(vals.view(np.uint64), want_v.view(np.uint64)), (what, vals, want_v)
    again_v, again_i = sets_hyper(sets, y_best, task, costs)
    assert np.array_equal(again_v.view(np.uint64), vals.view(np.uint64)) and np.array_equal(again_i, idxs)
    return vals, idxs


# (n, m, d, ard, causal, H, index_offset)
SHAPES = [
    (10, 1, 1, False, False, 1, 0),
    (17, 65, 3, True, True, 2, 1000),
    (128, 200, 3, True, False, 3, 7),
    (64, 64, 1, False, True, 10, 0),
    (1, 130, 2, False, False, 2, 0),
    (50, 200, 8, True, True, 2, 5),
]


@pytest.fixture(scope="module")
def zoo(hip):
    sets = [Set(hip, *shape) for shape in SHAPES]
    yield sets
    for st in sets:
        st.close()


@pytest.mark.parametrize("task", ["min", "max"])
def test_every_set_of_a_mixed_call_is_its_single_set_call_bit_for_bit(hip, zoo, task):
    pick = (lambda st: float(st.y.min())) if task == "min" else (lambda st: float(st.y.max()))
    # three sets: the descriptors travel by value
    three = zoo[:3]
    assert_per_set(three, [pick(st) for st in three], task, [3.0, 1.0, 0.5], "three sets")
    # all six and three of them again: nine descriptors, read from the pinned array
    nine = zoo + [zoo[1], zoo[3], zoo[5]]
    assert_per_set(nine, [pick(st) for st in nine], task, [3.0, 1.0, 0.5, 2.0, 1.5, 4.0, 0.25, 7.0, 1.0], "nine sets")


@pytest.mark.parametrize("m", [704, 768], ids=["11-blocks", "12-blocks"])
def test_either_side_of_the_two_launch_threshold(hip, m):
    wide = Set(hip, 17, m, 3, True, True, 3, 11)
    narrow = Set(hip, 17, 65, 3, False, False, 3, 0, seed=1)
    for task in ("min", "max"):
        assert_per_set([wide, narrow], [float(wide.y.min()), float(narrow.y.max())], task, [2.0, 3.0], f"m={m}")
        assert_per_set([narrow, wide], [float(narrow.y.max()), float(wide.y.min())], task, [3.0, 2.0], f"m={m}, narrow first")
    wide.close(); narrow.close()


@pytest.mark.parametrize("task", ["min", "max"])
def test_one_sample_at_each_models_own_hyper_parameters_is_cbo_acq_sweep_sets(hip, task):
    from cbo_with_oop_amd import _lib
    sets = [Set(hip, *shape[:5], 1, shape[6], seed=3, own_first=True) for shape in SHAPES]
    s = len(sets)
    y_best = np.array([float(np.median(st.y)) for st in sets])
    costs = np.linspace(0.5, 3.0, s)
    vals, idxs = sets_hyper(sets, y_best, task, costs)
    plain_v, plain_i = np.empty(s), np.empty(s, dtype=np.int64)
    _lib.check(_lib.load().cbo_acq_sweep_sets(s, handles([st.model for st in sets]), handles([st.grid for st in sets]),
                                              _lib.dptr(y_best), _lib.TASK_CODE[task], 0.0, _lib.dptr(costs),
                                              _lib.dptr(plain_v), plain_i.ctypes.data_as(_lib.c_int64_p)))
    print(task, vals.tolist(), plain_v.tolist())
    assert np.array_equal(idxs, plain_i)
    assert np.array_equal(vals.view(np.uint64), plain_v.view(np.uint64))
    for st in sets:
        st.close()


def test_nothing_of_the_small_models_or_their_candidates_is_touched(hip):
    from cbo_with_oop_amd import _lib
    own = samples_for(3, True, 1, seed=9)[0]
    # an unfitted model stays unfitted, beside a fitted one in the same call
    cold = Set(hip, 40, 130, 3, True, True, 3, 0)
    y_best = float(cold.y.min())
    outs = []
    for call in (True, False):
        warm = Set(hip, 40, 130, 3, True, True, 3, 0, keep_solution=True)
        warm.model.close(); warm.grid.close()
        warm.model = make_model(warm.X, warm.y, own, True, True)
        warm.grid = hip.CandidateGrid(warm.Xs, warm.model, keep_solution=True)
        ei = hip.CausalExpectedImprovement(y_best, "min", warm.model)
        before = ei.sweep(warm.grid, cost=2.0, want_acq=True, want_posterior=True)
        state = [np.array(v) for v in warm.model.posterior_state()]
        if call:
            vals, _ = sets_hyper([cold, warm], [y_best, y_best], "min", [1.0, 2.0])
            assert np.all(np.isfinite(vals)) and cold.model.stale
            rc = _lib.load().cbo_acq_sweep(cold.model._handle, cold.grid._handle, y_best, 0, 0.0, 1.0, None, None, None,
                                           ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int64()))
            assert rc == _lib.CBO_ERR_NOT_FITTED
        after = ei.sweep(warm.grid, cost=2.0, want_acq=True, want_posterior=True)
        for key in ("acq", "mean", "var"):
            assert np.array_equal(after[key], before[key])
        assert (after["best_val"], after["best_idx"]) == (before["best_val"], before["best_idx"])
        for u, v in zip(warm.model.posterior_state(), state):
            assert np.array_equal(np.array(u), v)
        assert not warm.model.stale
        assert warm.model.append(np.array([0.25, -0.5, 1.0]), 0.7)          # the kept solution grows by one row
        outs.append(ei.sweep(warm.grid, cost=2.0, want_acq=True, want_posterior=True))
        warm.close()
    for key in ("acq", "mean", "var"):
        assert np.array_equal(outs[0][key], outs[1][key])
    cold.close()


def same_value(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_mixed_routing_in_one_call(hip):
    """A model of 130 observations (the general path, restored afterwards) and the jitter fixture under a sample that is not
    positive definite as assembled (it declines in the launch and takes the general path) beside two small sets."""
    f = load_fixture("jitter_ladder")
    own = samples_for(3, True, 1, seed=8)[0]
    large = Set(hip, 130, 130, 3, True, True, 2, 3, seed=21)
    large.model.close(); large.grid.close()
    large.model = make_model(large.X, large.y, own, True, True)
    large.grid = hip.CandidateGrid(large.Xs, large.model, index_offset=3)
    ladder = Set.__new__(Set)
    ladder.X, ladder.y, ladder.Xs = f["X"], f["y"], f["Xs"]
    ladder.rows = np.array([[1.0, 1.0, 1e-2], [1e12, 1.0, 0.0]])
    ladder.model = make_model(ladder.X, ladder.y, ladder.rows[0], False, False)
    ladder.grid = hip.CandidateGrid(ladder.Xs, ladder.model)
    small = [Set(hip, 17, 65, 3, True, True, 2, 1000), Set(hip, 64, 64, 1, False, True, 10, 0)]
    sets = [small[0], large, ladder, small[1]]
    y_best = [float(small[0].y.min()), float(large.y.min()), float(f["y_best"]), float(small[1].y.min())]
    costs = [2.0, 3.0, 1.0, 0.5]
    ei = hip.CausalExpectedImprovement(y_best[1], "min", large.model)
    before = ei.sweep(large.grid, cost=3.0, want_acq=True, want_posterior=True)
    state = [np.array(v) for v in large.model.posterior_state()]
    with np.errstate(invalid="ignore"):
        vals, idxs = sets_hyper(sets, y_best, "min", costs)
        want = [single_hyper(st, y_best[i], "min", costs[i]) for i, st in enumerate(sets)]
    print(vals.tolist(), idxs.tolist(), want)
    for i in (0, 3):                                               # the small sets: the launch's bits
        assert idxs[i] == want[i][1] and np.float64(vals[i]).view(np.uint64) == np.float64(want[i][0]).view(np.uint64)
    for i in (1, 2):                                               # the general path inside the call is the single call's
        assert idxs[i] == want[i][1] and same_value(vals[i], want[i][0])
    # the large model: hyper-parameters restored, fitted again, the same factor
    after = ei.sweep(large.grid, cost=3.0, want_acq=True, want_posterior=True)
    for key in ("acq", "mean", "var"):
        assert np.array_equal(after[key], before[key])
    for u, v in zip(large.model.posterior_state(), state):
        assert np.array_equal(np.array(u), v)
    assert not ladder.model.stale and small[0].model.stale and small[1].model.stale
    for st in sets:
        st.close()


# three of tests/test_hyper_gpu.py's oracle cases, as the sets of one call: (n, m, d, ard, causal, H)
ORACLE_SETS = [(17, 65, 3, True, True, 10), (64, 200, 1, False, False, 2), (128, 64, 3, False, True, 2)]


@pytest.mark.parametrize("task", ["min", "max"])
def test_against_the_mean_of_the_oracles_sweeps(hip, task):
    sets = [Set(hip, n, m, d, ard, causal, H, 0, seed=6 * n) for n, m, d, ard, causal, H in ORACLE_SETS]
    cost = 3.0
    y_best = [float(st.y.min() if task == "min" else st.y.max()) for st in sets]
    vals, idxs = sets_hyper(sets, y_best, task, [cost] * len(sets))
    for i, st in enumerate(sets):
        X, y, Xs, H = st.X, st.y, st.Xs, st.rows.shape[0]
        mX, vX, mXs, vXs = (prior_mean(X), prior_var(X), prior_mean(Xs), prior_var(Xs)) if st.causal else (None,) * 4
        oracle, truth = np.zeros(Xs.shape[0]), np.zeros(Xs.shape[0])
        for row in st.rows:
            ls = row[1:-1] if st.ard else float(row[1])
            post = O.fit(X, y, mX, vX, variance=float(row[0]), lengthscale=ls, noise_var=float(row[-1]))
            assert post.tries == 0                                 # (noise >= 1e-2: the oracle itself is well conditioned)
            oracle += O.acquisition_sweep(post, Xs, y_best[i], mXs, vXs, task=task, cost=cost)[0][:, 0]
            mt, vt, _ = truth_predict(X, y, Xs, mX, vX, mXs, vXs, float(row[0]), ls, diag_add=float(row[-1]) + 1e-8,
                                      noise_var=float(row[-1]))
            truth += O.expected_improvement(mt, vt, y_best[i], task)[:, 0] / cost
        oracle, truth = oracle / H, truth / H
        _, _, acq = single_hyper(st, y_best[i], task, cost, want_acq=True)
        w = first_argmax(acq)
        assert idxs[i] == w
        assert abs(oracle[w]) > 1e-6 * np.max(np.abs(oracle))     # (the winner's EI is not negligible: parity is meaningful)
        rel = assert_parity(vals[i:i + 1], oracle[w:w + 1], truth[w:w + 1], f"marginalised winner, set {st.shape} {task}",
                            rtol=1e-5, slack=8.0)
        print(task, st.shape, "winner", w, vals[i], oracle[w], truth[w], rel)
    for st in sets:
        st.close()


def test_error_returns(hip):
    from cbo_with_oop_amd import _lib
    lib = _lib.load()
    invalid = _lib.CBO_ERR_INVALID
    a = Set(hip, 12, 20, 2, False, False, 2, 0)
    b = Set(hip, 17, 65, 3, True, True, 2, 0)
    a.rows = np.array([[1.0, 1.0, 1e-2], [2.0, 0.5, 0.0]])
    other_d = hip.CandidateGrid(np.zeros((4, 3)))
    sets = [a, b]
    vals, idxs = np.full(2, -7.0), np.full(2, -7, dtype=np.int64)

    def call(n_sets=2, gps="ok", cands="ok", counts=None, rows="ok", y_best=(0.0, 0.0), task=0, costs=(1.0, 2.0),
             outputs=True):
        arr = lambda v: None if v is None else _lib.dptr(np.array(v, dtype=np.float64))                            # noqa: E731
        rows_ = [a.rows, b.rows] if isinstance(rows, str) else rows
        keep = None if rows_ is None else [None if r is None else np.ascontiguousarray(r) for r in rows_]
        ptrs = None if keep is None else (ctypes.c_void_p * len(keep))(*[None if r is None else r.ctypes.data for r in keep])
        cnt = counts if counts is not None else (None if keep is None else [0 if r is None else r.shape[0] for r in keep])
        cnt_arr = None if cnt is None or cnt == "null" else (ctypes.c_int * len(cnt))(*cnt)
        g = handles([st.model for st in sets]) if isinstance(gps, str) else gps
        k = handles([st.grid for st in sets]) if isinstance(cands, str) else cands
        return lib.cbo_acq_sweep_sets_hyper(n_sets, g, k, cnt_arr, ptrs, arr(y_best), task, 0.0, arr(costs),
                                            _lib.dptr(vals) if outputs else None,
                                            idxs.ctypes.data_as(_lib.c_int64_p) if outputs else None)

    def refused(**kw):
        stale = [st.model.stale for st in sets]
        assert call(**kw) == invalid, kw
        assert [st.model.stale for st in sets] == stale

    assert call() == _lib.CBO_OK
    # what needs no handle: refused also with NULL handle arrays
    for kw in (dict(n_sets=0), dict(n_sets=-2), dict(counts="null"), dict(rows=None, counts=[2, 2]), dict(y_best=None),
               dict(costs=None), dict(outputs=False), dict(rows=[a.rows, None], counts=[2, 2]), dict(counts=[0, 2]),
               dict(counts=[2, -1]), dict(counts=[2, 257]), dict(task=2), dict(task=-1), dict(costs=(1.0, 0.0)),
               dict(costs=(-1.0, 1.0)), dict(costs=(1.0, float("nan")))):
        refused(**kw)
        refused(gps=None, cands=None, **kw)
    assert call(rows=[a.rows, np.tile(b.rows[:1], (256, 1))]) == _lib.CBO_OK            # 256 samples pass
    refused(rows=[a.rows, np.tile(b.rows[:1], (257, 1))])                               # 257 are refused
    # the rows' values (their length is the model's)
    for col in (0, 1):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rows = a.rows.copy()
            rows[1, col] = bad
            refused(rows=[rows, b.rows])
    for bad in (-1e-12, float("nan"), float("inf")):
        rows = b.rows.copy()
        rows[0, -1] = bad
        refused(rows=[a.rows, rows])
    # the handles
    refused(gps=None); refused(cands=None)
    refused(gps=(ctypes.c_void_p * 2)(a.model._handle, None)); refused(cands=(ctypes.c_void_p * 2)(None, b.grid._handle))
    refused(cands=(ctypes.c_void_p * 2)(a.grid._handle, a.grid._handle))               # gp->d != cands->d
    refused(cands=(ctypes.c_void_p * 2)(other_d._handle, b.grid._handle))
    plain_grid = hip.CandidateGrid(b.Xs)                                                # a causal model needs the prior closures
    refused(cands=(ctypes.c_void_p * 2)(a.grid._handle, plain_grid._handle))
    # never CBO_ERR_NOT_FITTED; the refusals left nothing behind: a good call succeeds and answers as before
    assert a.model.stale and b.model.stale
    first = sets_hyper(sets, [0.0, 0.0], "min", [1.0, 2.0])
    assert call() == _lib.CBO_OK
    assert np.array_equal(vals.view(np.uint64), first[0].view(np.uint64)) and np.array_equal(idxs, first[1])
    plain_grid.close(); other_d.close(); a.close(); b.close()


def test_models_of_different_contexts_are_refused(hip):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    a = Set(hip, 12, 20, 2, False, False, 2, 0)
    ctx = _lib.Context(a.model._ctx.device_id)
    try:
        X, y, Xs = problem(12, 20, 2, seed=5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            other = HipGaussianProcess(X, y, context=ctx, fit=False)
        b = Set.__new__(Set)
        b.model, b.grid, b.rows = other, hip.CandidateGrid(Xs, other), a.rows
        assert sets_hyper([a, b], [0.0, 0.0], "min", [1.0, 1.0], rc_only=True) == _lib.CBO_ERR_INVALID
        assert b"context" in _lib.load().cbo_last_error()
        assert a.model.stale and other.stale
        b.grid.close(); other.close()
    finally:
        ctx.close()
    a.close()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def toy_problem(cost_type, n=12, seed=4):
    from cbo_with_oop_amd.graphs import ToyGraph
    es = ToyGraph.get_exploration_set("MIS")
    targets = [ToyGraph.target_do_x, ToyGraph.target_do_z]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-5, 5, (n, 1)), rng.uniform(-5, 20, (n, 1))]
    return es, targets, xs, ToyGraph.get_cost_structure(cost_type)


def factory_model(x, y):
    from cbo_with_oop_amd import GaussianProcessType
    from cbo_with_oop_amd.GaussianProcessFactory import GaussianProcessFactory as GPFactory
    return GPFactory.create(GaussianProcessType.NON_CAUSAL_GP, x, y, [None, None], emukit_wrapper=True)


def toy_sampler(model, s):
    """(H, 3) samples for a factory model of the toy graph: a function of the set and of the model's row count alone (and no
    draw from numpy's global generator), so that a twin model of the same data gets the same rows."""
    return samples_for(1, False, 2 + s, seed=17 * s + model.X.shape[0])


@pytest.mark.parametrize("cost_type", [1, 4])
def test_find_next_y_points_with_hyper_samples_is_find_next_y_point_per_set(hip, cost_type):
    """One call for both sets against find_next_y_point(hyper_samples=rows_s) set by set on twin models: points and values
    exact; with the variable cost table (4) every winner is re-evaluated at its own cost."""
    from cbo_with_oop_amd import CandidateGrid
    from cbo_with_oop_amd.graphs import ToyGraph, meshgrid_candidates
    from cbo_with_oop_amd.utils_functions import find_next_y_point, find_next_y_points
    es, targets, xs, table = toy_problem(cost_type)
    ys = [t(x) for t, x in zip(targets, xs)]
    best = min(float(y.min()) for y in ys)
    models = [factory_model(xs[s], ys[s]) for s in range(2)]
    rows = [toy_sampler(models[s], s) for s in range(2)]
    grids = [CandidateGrid(meshgrid_candidates(ToyGraph.bounds(es[s]), [200]), models[s]) for s in range(2)]
    cache = {}
    for task in ("min", "max"):
        a_x, a_y = find_next_y_points(models, best, es, table, task, grids, cache=cache, hyper_samples=rows)
        for s in range(2):
            twin = factory_model(xs[s], ys[s])
            y, x = find_next_y_point(ToyGraph.bounds(es[s]), twin, best, es[s], table, task=task, grid_shape=[200],
                                     hyper_samples=rows[s])
            print(task, s, a_y[s].tolist(), y.tolist(), a_x[s].tolist(), x.tolist())
            assert np.array_equal(a_x[s], x)
            assert np.array_equal(a_y[s].view(np.uint64), y.view(np.uint64))
            twin.close()
    entry = cache["sweep_sets"]
    assert entry["hyper_rows"] is not None and len(entry["hyper_args"]) == 2
    # back to None: today's call, on the same entry
    find_next_y_points(models, best, es, table, "min", grids, cache=cache)
    assert cache["sweep_sets"] is entry and entry["hyper_rows"] is None
    for g in grids:
        g.close()
    for m in models:
        m.close()


def test_path_trials_with_a_sampler_pick_what_the_per_set_calls_pick(hip):
    """Three trials of CBOAcquisitionPath.trial_step with a callable sampler against the loop composed of the per-set calls
    (find_next_y_point(hyper_samples=rows) on fresh models, then the first maximum): same pick, points and values.  The
    sampler is asked for every set when all models are built, and only for the set intervened on afterwards."""
    from cbo_with_oop_amd import CBOAcquisitionPath, GaussianProcessType
    from cbo_with_oop_amd.graphs import ToyGraph
    from cbo_with_oop_amd.utils_functions import find_next_y_point
    es, targets, xs, table = toy_problem(4)
    ys = [t(x) for t, x in zip(targets, xs)]
    asked = []

    def sampler(model, s):
        asked.append((s, model.X.shape[0]))
        return toy_sampler(model, s)
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys, [ToyGraph.bounds(s) for s in es],
                              grid_shapes=[[200], [200]], comm=None, hyper_samples=sampler)
    path.update_all_gaussian_processes()
    assert asked == [(0, 12), (1, 12)]
    with pytest.raises(ValueError, match="single process"):
        class Two:
            world, rank = 2, 0
        other = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, table, "min", xs, ys,
                                   [ToyGraph.bounds(s) for s in es], comm=Two(), hyper_samples=sampler)
        other.hyper_rows = list(path.hyper_rows)
        other.compute_best_acquisition_values(0.0)
    last = None
    for trial in range(3):
        del asked[:]
        best = min(float(ys[0].min()), float(ys[1].min()))
        a_x, a_y, (a_set, a_idx) = path.trial_step(best)
        assert asked == ([] if last is None else [(last, xs[last].shape[0])])
        b_x, b_y = [], []
        for s in range(2):
            twin = factory_model(xs[s], ys[s])
            y, x = find_next_y_point(ToyGraph.bounds(es[s]), twin, best, es[s], table, task="min", grid_shape=[200],
                                     hyper_samples=toy_sampler(twin, s))
            b_x.append(x); b_y.append(y)
            twin.close()
        b_idx = int(np.argmax([float(y[0, 0]) for y in b_y]))
        print("trial", trial, [y.tolist() for y in a_y], [y.tolist() for y in b_y])
        assert a_idx == b_idx and a_set == es[b_idx]
        assert all(np.array_equal(p, q) for p, q in zip(a_x, b_x))
        assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(a_y, b_y))
        assert "trial_args" not in path._call_cache["sweep_sets"]               # the three-call route
        xs[a_idx] = np.vstack([xs[a_idx], a_x[a_idx]])
        ys[a_idx] = np.vstack([ys[a_idx], targets[a_idx](a_x[a_idx])])
        last = a_idx


def test_the_agent_runs_with_a_sampler_and_chooses_what_a_path_with_the_same_rows_chooses(hip):
    """CBO(toy graph, hyper_samples=sampler, num_trials=4).run(): the sets its monitor records are those a
    CBOAcquisitionPath chooses when it is driven through the same interventions with the same sampler."""
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
                    hyper_samples=toy_sampler)
        mon = agent.run()
    assert len(mon.type_trial) == 4 and 1 in mon.type_trial
    assert agent.hyper_samples is toy_sampler and all(r is not None for r in agent.hyper_rows)
    chosen = [c for c in mon.chosen if c is not None]
    assert len(chosen) == sum(mon.type_trial)
    # the same interventions through a path: fresh models of the data so far, the same sampler, the first maximum
    px, py = [d[0].copy() for d in data], [d[1].copy() for d in data]
    path = CBOAcquisitionPath(GaussianProcessType.NON_CAUSAL_GP, es, agent.costs, "min", px, py, [Toy.bounds(s) for s in es],
                              grid_shapes=[[64], [64]], comm=None, hyper_samples=toy_sampler)
    for picked_set, picked_x in chosen:
        best = min(float(py[0].min()), float(py[1].min()))
        path.update_all_gaussian_processes()
        xs_new, ys_new = path.compute_best_acquisition_values(best)
        a_set, a_idx = path.select_next_intervention(ys_new)
        print(picked_set, picked_x.tolist(), a_set, xs_new[a_idx].tolist())
        assert a_set == picked_set and np.array_equal(xs_new[a_idx], picked_x)
        px[a_idx] = np.vstack([px[a_idx], xs_new[a_idx]])
        py[a_idx] = np.vstack([py[a_idx], targets[a_idx](xs_new[a_idx])])
