"""Timing of the gradient refinement under constraints in one launch (cbo_acq_refine_sets_constrained,
kernels_sets_refine_con.hip) on one MI355X, at the reference's scale -- 50 observations and 200 candidates
per model, d = 1 and d = 3 -- for 2, 6 and 25 sets under 1, 2 and 4 constraints each, in both forms (EI prod PoF / cost and
log EI + sum log PoF - log cost), beside what it replaces, on the same box and the same models:

  (a) find_next_y_points(constraints=..., refine_constrained=True): the constrained grid sweeps of every set (one call) plus
      the ONE refinement call from the winners (one device launch for all sets, all rounds);
  (b) the per-set host sequence of the same tree: CausalGradientAcquisitionOptimizer.optimize(product / cost, refine=True)
      set by set -- a grid sweep, then scipy's L-BFGS-B whose every evaluation is a predict plus a get_prediction_gradients
      device call per model of the set, each with a synchronisation.

Every figure is the host's clock around one whole Python call: --warmup unrecorded calls per variant, then the variants
ALTERNATE for --reps rounds (the round's first variant rotating), and the median, quartiles, min and max per variant are
reported in microseconds (§4q's method).  The rounds every search of (a) took are reported beside them (min / median / max
over the sets).  Every (d, sets) shape is measured by a fresh child process under its own time limit; the first child that
fails or runs out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/sets_refine_con_timing.py --out profiles/sets_refine_con_timing.json
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
N_CON = [1, 2, 4]
FORMS = ["EI", "LOGCEI"]
N, M = 50, 200
A, B_ = "(a) sweeps + one refinement call", "(b) per set (optimize(refine=True))"


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "p25": float(np.percentile(v, 25)), "p75": float(np.percentile(v, 75)), "count": int(v.size)}


def launch_rounds(models, cons, xs, box, cost, form, y_best):
    """The entry point itself from the grid winners: (rounds, status) of every set's search."""
    import ctypes
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.utils_functions.causal_optimizer import _refine_call_arrays
    from cbo_with_oop_amd.utils_functions.constrained import SENSE_CODE
    s = len(models)
    starts = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    lo, hi = np.array([b[0] for b in box], dtype=np.float64), np.array([b[1] for b in box], dtype=np.float64)
    sets, keep, (x, v, g, rounds, status) = _refine_call_arrays(list(range(s)), starts, [lo] * s, [hi] * s, [cost] * s)
    flat = [c for row in cons for c in row]
    values, jitters = np.array([float(c.max_value) for c in flat]), np.array([float(c.jitter) for c in flat])
    _lib.check(_lib.load().cbo_acq_refine_sets_constrained(
        s, (ctypes.c_void_p * s)(*[m._handle for m in models]), sets, int(form == "LOGCEI"), _lib.dptr(np.full(s, y_best)), 0,
        0.0, (ctypes.c_int * s)(*[len(row) for row in cons]), (ctypes.c_void_p * len(flat))(*[c.model._handle for c in flat]),
        _lib.dptr(values), _lib.dptr(jitters), (ctypes.c_int * len(flat))(*[SENSE_CODE[c.sense] for c in flat]), 200,
        _lib.dptr(x), _lib.dptr(v), _lib.dptr(g), rounds.ctypes.data_as(_lib.c_int_p), status.ctypes.data_as(_lib.c_int_p)))
    return rounds, status


def measure(d, s, reps, warmup):
    """One (d, sets) shape, in this process: per form and n_con {variant: stats} and the rounds of the searches."""
    import functools
    import warnings
    from cbo_with_oop_amd import CandidateGrid, _lib, graphs
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.utils_functions import (CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost,
                                                  ProbabilityOfFeasibility, find_next_y_points)
    from cbo_with_oop_amd.utils_functions.constrained import AcquisitionProduct, ConstrainedLogExpectedImprovement
    from cbo_with_oop_amd.utils_functions.pointwise_acquisitions import CausalLogExpectedImprovement
    warnings.simplefilter("ignore", RuntimeWarning)
    rng = np.random.default_rng(100 * d + s)
    shape = [M] if d == 1 else [6, 6, 6]                            # 200 candidates; 216 at d = 3: six per axis
    box = [(-5.0, 5.0)] * d
    names = [f"V{k}" for k in range(d)]
    table = {v: functools.partial(graphs.cost, 1, False) for v in names}
    pts = graphs.meshgrid_candidates(box, shape)
    models, con_models, grids = [], [], []
    for _ in range(s):
        X = rng.uniform(-5.0, 5.0, (N, d))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
        models.append(HipGaussianProcess(X, y, noise_var=1e-2))
        grids.append(CandidateGrid(pts, models[-1]))
        con_models.append([HipGaussianProcess(X, np.cos(0.6 * X + 0.3 * k).sum(1, keepdims=True)
                                              + 0.1 * rng.standard_normal((N, 1)), noise_var=1e-2) for k in range(max(N_CON))])
    y_best = float(np.median(models[0].Y))
    cost = Cost(table, names)
    evaluated = [names] * s
    out = {}
    for form in FORMS:
        for n_con in N_CON:
            cons = [[ProbabilityOfFeasibility(c, max_value=0.25 * (k + 1), sense=("<=", ">=")[k % 2])
                     for k, c in enumerate(con_models[i][:n_con])] for i in range(s)]
            if form == "EI":
                acqs = [AcquisitionProduct([CausalExpectedImprovement(y_best, "min", m)] + cons[i]) / cost
                        for i, m in enumerate(models)]
            else:
                acqs = [ConstrainedLogExpectedImprovement(CausalLogExpectedImprovement(y_best, "min", m), cons[i]) / cost
                        for i, m in enumerate(models)]
            opts = [CausalGradientAcquisitionOptimizer(box, grid_shape=shape) for _ in range(s)]
            cache, state = {}, {}

            def one_call():
                state["xs"], state["ys"] = find_next_y_points(models, y_best, evaluated, table, "min", grids, cache=cache,
                                                              acquisition=form, spaces=[box] * s, refine_constrained=True,
                                                              constraints=cons)

            def per_set():
                for o, a in zip(opts, acqs):
                    o.optimize(a, refine=True)

            variants = {A: one_call, B_: per_set}
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
            # the rounds the launch's searches take from the grid winners (the entry itself reports them)
            xs, _ = find_next_y_points(models, y_best, evaluated, table, "min", grids, acquisition=form, constraints=cons)
            rounds, status = launch_rounds(models, cons, xs, box, cost, form, y_best)
            for a in acqs:
                a.numerator.close()
            out[f"{form}, n_con = {n_con}"] = {
                "calls_us": {k: stats(t) for k, t in times.items()},
                "rounds": {"min": int(rounds.min()), "median": float(np.median(rounds)), "max": int(rounds.max())},
                "status": sorted(set(_lib.REFINE_STATUS_NAME[int(c)] for c in status))}
    name = _lib.Context.get().name()
    for o in grids + models + [c for row in con_models for c in row]:
        o.close()
    return {"device": name, "cases": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_refine_con_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--step-timeout", type=float, default=280.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", type=int, nargs=2, default=None, help="(child) measure this (d, sets) and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(a.shape[0], a.shape[1], a.reps, a.warmup)), flush=True)
        return 0
    report = {"n": N, "m": M, "warmup": a.warmup, "reps": a.reps,
              "clock": "time.perf_counter_ns around one whole call, variants alternating with a rotating start; one child "
                       "process per (d, sets) shape",
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
            for case, row in got["cases"].items():
                report["calls_us"][f"{key}, {case}"] = row["calls_us"]
                report["rounds"][f"{key}, {case}"] = {"kernel_rounds": row["rounds"], "status": row["status"]}
                print(f"{key}, {case}", json.dumps({k: round(t["median"], 1) for k, t in row["calls_us"].items()}),
                      json.dumps(report["rounds"][f"{key}, {case}"]), flush=True)
        if ended:
            break
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    rows = report["calls_us"]
    if rows:
        report["one_call_below_per_set_in_every_case_measured"] = all(r[A]["median"] < r[B_]["median"] for r in rows.values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k not in ("calls_us", "rounds")}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
