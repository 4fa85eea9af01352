"""Timing of causal exploration sets inside the one-launch refinement (cbo_acq_refine_sets_prior and the device-resident
do-calculus prior, kernels_sets_refine.hip / kernels_do_prior.hip) on one MI355X, by the method of
scripts/sets_refine_timing.py: 50 observations and 200 candidates per exploration set, d = 1 and d = 3, 2, 6 and 25 CAUSAL
sets whose priors are the do-calculus closures of a graph GP of 100 and of 1000 rows (N_obs = n_g; d + 1 input columns, the
first d intervened), beside what the parent commit runs for such sets, on the same box and the same models:

  (a) refine_sets(device_prior=True): ONE call refines every set's grid winner -- the sets' priors are created, one launch
      advances every search with the prior evaluated inside it, the priors are closed;
      (a') the creation (and closing) of the sets' priors alone, the part of (a) that is not the launch;
  (b) the per-set sequence: CausalGradientAcquisitionOptimizer.optimize(acquisition, refine=True) set by set -- a grid
      sweep, then scipy's L-BFGS-B whose every evaluation runs the Python closures (two cbo_gp_predict_do calls of N_obs
      graph-GP predictions each) beside a predict and a get_prediction_gradients call;
  (c) the grid sweeps alone (find_next_y_points), the part of a trial both share.

The bar is (c) + (a) below (b).  Every figure is the host's clock around one whole call: --warmup unrecorded calls per
variant, then the variants ALTERNATE for --reps rounds (the round's first variant rotating); median, quartiles, min and max
in microseconds.  Every (n_g, d, sets) shape is measured by a fresh child process under its own time limit; the first child
that fails or runs out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/sets_refine_causal_timing.py --out profiles/sets_refine_causal_timing.json
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
ROWS = [100, 1000]
N, M = 50, 200
A, A1, B_, C = ("(a) one call (refine_sets(device_prior=True))", "(a') creating the priors", "(b) per set (optimize(refine=True))",
                "(c) grid sweeps (find_next_y_points)")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "p25": float(np.percentile(v, 25)), "p75": float(np.percentile(v, 75)), "count": int(v.size)}


def measure(n_g, d, s, reps, warmup):
    """One shape, in this process: {variant: stats}, the statuses of the searches and the device's name."""
    import functools
    import warnings
    from cbo_with_oop_amd import CandidateGrid, _lib, graphs
    from cbo_with_oop_amd.DoCalculus import DoPrior, do_prior_functions, prior_spec
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.utils_functions import CausalExpectedImprovement, CausalGradientAcquisitionOptimizer, Cost
    from cbo_with_oop_amd.utils_functions import find_next_y_points
    from cbo_with_oop_amd.utils_functions.causal_optimizer import refine_sets
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(100000 * (n_g // 100) + 100 * d + s)
    shape = [M] if d == 1 else [6, 6, 6]                            # 200 candidates; 216 at d = 3: six per axis
    box = [(-5.0, 5.0)] * d
    names = [f"V{k}" for k in range(d)]
    table = {v: functools.partial(graphs.cost, 1, False) for v in names}
    pts = graphs.meshgrid_candidates(box, shape)
    Xg = rng.uniform(-5.0, 5.0, (n_g, d + 1))
    yg = np.sin(Xg).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n_g, 1))
    graph_gp = HipGaussianProcess(Xg, yg, variance=1.0, lengthscale=1.5, noise_var=1e-2, fix_noise=True)
    idx = list(range(d)) + [-1]
    models, grids, opts = [], [], []
    for _ in range(s):
        X = rng.uniform(-5.0, 5.0, (N, d))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
        m_fn, v_fn = do_prior_functions(graph_gp, Xg, idx)
        models.append(HipGaussianProcess(X, y, noise_var=1e-2, mean_function=m_fn, variance_adjustment=v_fn))
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
        state["res"] = refine_sets(models, state["xs"], [box] * s, y_best, "min", [cost] * s, device_prior=True,
                                   host_fallback=False)

    def create():
        for p in [DoPrior(*prior_spec(m)) for m in models]:
            p.close()

    def per_set():
        for o, a in zip(opts, acqs):
            o.optimize(a, refine=True)

    sweeps()
    variants = {A: one_call, A1: create, B_: per_set, C: sweeps}
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
    status = np.concatenate([r[2] for r in state["res"]])
    name = _lib.Context.get().name()
    for o in grids + models + [graph_gp]:
        o.close()
    return {"device": name, "calls_us": {k: stats(t) for k, t in times.items()},
            "status": sorted(set(_lib.REFINE_STATUS_NAME[int(c)] for c in status))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_refine_causal_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", type=int, nargs=3, default=None, help="(child) measure this (n_g, d, sets) and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(a.shape[0], a.shape[1], a.shape[2], a.reps, a.warmup)), flush=True)
        return 0
    report = {"n": N, "m": M, "warmup": a.warmup, "reps": a.reps,
              "clock": "time.perf_counter_ns around one whole call, variants alternating with a rotating start; one child process per shape",
              "calls_us": {}, "status": {}, "complete": False}
    ended = None
    for n_g in ROWS:
        for d in DIMS:
            for s in SETS:
                key = f"n_g = {n_g}, d = {d}, {s} sets"
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(n_g), str(d), str(s), "--reps", str(a.reps),
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
                report["status"][key] = got["status"]
                print(key, json.dumps({k: round(t["median"], 1) for k, t in row.items()}), got["status"], flush=True)
            if ended:
                break
        if ended:
            break
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    else:
        rows = report["calls_us"]
        report["sweeps_plus_one_call_over_per_set"] = {k: (r[C]["median"] + r[A]["median"]) / r[B_]["median"] for k, r in rows.items()}
        report["sweeps_plus_one_call_below_per_set_everywhere"] = all(
            r[C]["median"] + r[A]["median"] < r[B_]["median"] for r in rows.values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k not in ("calls_us", "status")}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
