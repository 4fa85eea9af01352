"""Timing of the gradient refinement of every set in one launch (cbo_acq_refine_sets, kernels_sets_refine.hip; DESIGN.md
§4q) on one MI355X, at the reference's scale -- 50 observations and 200 candidates per exploration set, d = 1 and d = 3 --
for 2, 6 and 25 sets, beside what it replaces, on the same box and the same models:

  (a) refine_sets: ONE call refines every set's grid winner (one device launch for all sets, all rounds);
  (b) the per-set sequence of the same tree: CausalGradientAcquisitionOptimizer.optimize(acquisition, refine=True) set by
      set -- a grid sweep, then scipy's L-BFGS-B whose every evaluation is a predict plus a get_prediction_gradients device
      call with a synchronisation;
  (c) the grid sweeps alone (find_next_y_points), the part of a trial both share -- (a) runs behind it, (b) contains its own.

So the comparison that answers "is the one call faster than the sequence it replaces" is (c) + (a) against (b).
Every figure is the host's clock around one whole call: --warmup unrecorded calls per variant, then the variants ALTERNATE
for --reps rounds (the round's first variant rotating), and the median, quartiles, min and max per variant are reported in
microseconds.  The rounds every search of (a) took are reported beside them (min / median / max over the sets), and the
evaluations scipy made in (b).  Every (d, sets) shape is measured by a fresh child process under its own time limit; the
first child that fails or runs out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/sets_refine_timing.py --out profiles/sets_refine_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = [2, 6, 25]
DIMS = [1, 3]
N, M = 50, 200
A, B_, C = ("(a) one call (refine_sets)", "(b) per set (optimize(refine=True))", "(c) grid sweeps (find_next_y_points)")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "p25": float(np.percentile(v, 25)), "p75": float(np.percentile(v, 75)), "count": int(v.size)}


def measure(d, s, reps, warmup):
    """One shape, in this process: {variant: stats}, the rounds of the searches and the device's name."""
    import functools
    from cbo_with_oop_amd import CandidateGrid, _lib, graphs
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost
    from cbo_with_oop_amd.utils_functions import find_next_y_points
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    rng = np.random.default_rng(100 * d + s)
    shape = [M] if d == 1 else [6, 6, 6]                            # 200 candidates; 216 at d = 3: six per axis
    box = [(-5.0, 5.0)] * d
    names = [f"V{k}" for k in range(d)]
    table = {v: functools.partial(graphs.cost, 1, False) for v in names}
    pts = graphs.meshgrid_candidates(box, shape)
    models, grids, opts, acqs = [], [], [], []
    for _ in range(s):
        X = rng.uniform(-5.0, 5.0, (N, d))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
        models.append(HipGaussianProcess(X, y, noise_var=1e-2))
        grids.append(CandidateGrid(pts, models[-1]))
        opts.append(CausalGradientAcquisitionOptimizer(box, grid_shape=shape))
    y_best = float(np.median(models[0].Y))
    cost = Cost(table, names)
    acqs = [CausalExpectedImprovement(y_best, "min", m) / cost for m in models]
    evaluated = [names] * s
    cache = {}
    state = {}

    def sweeps():
        state["xs"], state["ys"] = find_next_y_points(models, y_best, evaluated, table, "min", grids, cache=cache)

    def one_call():
        state["res"] = refine_sets(models, state["xs"], [box] * s, y_best, "min", [cost] * s)

    def per_set():
        for o, a in zip(opts, acqs):
            o.optimize(a, refine=True)

    sweeps()
    variants = {A: one_call, B_: per_set, C: sweeps}
    for call in variants.values():
        for _ in range(warmup):
            call()
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(reps):
        for k in order[r % len(order):] + order[:r % len(order)]:
            t0 = time.perf_counter_ns()
            variants[k]()
            times[k].append((time.perf_counter_ns() - t0) * 1e-3)
    # the rounds the launch's searches took (the entry itself reports them), and scipy's evaluations in (b)
    import ctypes
    lib = _lib.load()
    fix, variable = np.ones(d), np.zeros(d, dtype=np.int32)
    lo, hi = np.full(d, -5.0), np.full(d, 5.0)
    sets = (_lib.CboRefineSet * s)()
    starts = [np.ascontiguousarray(x) for x in state["xs"]]
    for j in range(s):
        sets[j].k = 1
        sets[j].starts = starts[j].ctypes.data_as(_lib.c_double_p)
        sets[j].lo, sets[j].hi = lo.ctypes.data_as(_lib.c_double_p), hi.ctypes.data_as(_lib.c_double_p)
        sets[j].cost_fix, sets[j].cost_variable = fix.ctypes.data_as(_lib.c_double_p), variable.ctypes.data_as(_lib.c_int_p)
    x, g, v = np.zeros(s * d), np.zeros(s * d), np.zeros(s)
    rounds, status = np.zeros(s, dtype=np.int32), np.zeros(s, dtype=np.int32)
    _lib.check(lib.cbo_acq_refine_sets(s, (ctypes.c_void_p * s)(*[m._handle for m in models]), sets, 0,
                                       _lib.dptr(np.full(s, y_best)), 0, 0.0, 200, _lib.dptr(x), _lib.dptr(v), _lib.dptr(g),
                                       rounds.ctypes.data_as(_lib.c_int_p), status.ctypes.data_as(_lib.c_int_p)))
    evals = []
    for m, a, x0 in zip(models, acqs, starts):
        count = [0]
        inner = a.evaluate_with_gradients

        def counted(p, inner=inner, count=count):
            count[0] += 1
            return inner(p)
        a.evaluate_with_gradients = counted
        opts[0].refine(a, x0)
        a.evaluate_with_gradients = inner
        evals.append(count[0])
    name = _lib.Context.get().name()
    for o in grids + models:
        o.close()
    return {"device": name, "calls_us": {k: stats(t) for k, t in times.items()},
            "rounds": {"min": int(rounds.min()), "median": float(np.median(rounds)), "max": int(rounds.max())},
            "status": sorted(set(_lib.REFINE_STATUS_NAME[int(c)] for c in status)),
            "scipy_evaluations": {"min": int(min(evals)), "median": float(np.median(evals)), "max": int(max(evals))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_refine_timing.json"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", type=int, nargs=2, default=None, help="(child) measure this (d, sets) and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(a.shape[0], a.shape[1], a.reps, a.warmup)), flush=True)
        return 0
    report = {"n": N, "m": M, "warmup": a.warmup, "reps": a.reps,
              "clock": "time.perf_counter_ns around one whole call, variants alternating with a rotating start; one child process per shape",
              "calls_us": {}, "rounds": {}, "complete": False}
    ended = None
    for d in DIMS:
        for s in SETS:
            key = f"d = {d}, {s} sets"
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(d), str(s), "--reps", str(a.reps),
                   "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                ended = f"{key}: no result within {a.step_timeout} s"
                break
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                ended = f"{key}: exit status {r.returncode}: {r.stderr[-400:]}"
                break
            got = json.loads(line[-1][len("RESULT "):])
            report["device"] = got["device"]
            row = report["calls_us"][key] = got["calls_us"]
            report["rounds"][key] = {"kernel_rounds": got["rounds"], "status": got["status"],
                                     "scipy_evaluations": got["scipy_evaluations"]}
            print(key, json.dumps({k: round(t["median"], 1) for k, t in row.items()}), json.dumps(report["rounds"][key]),
                  flush=True)
        if ended:
            break
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    else:
        rows = report["calls_us"]
        report["sweeps_plus_one_call_below_per_set_everywhere"] = all(
            r[C]["median"] + r[A]["median"] < r[B_]["median"] for r in rows.values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k not in ("calls_us", "rounds")}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
