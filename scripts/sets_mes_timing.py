"""Timing of max-value entropy search in the multi-set form (cbo_gp_mes_gumbel_sets, cbo_acq_sweep_sets_mes)
on one MI355X: 2, 6 and 25 exploration sets of 50 observations and 200 candidates, K = 10 Gumbel samples, Gumbel grids of
5050 points (the model's 50 on top of emukit's default 5000), each new call beside the per-set sequence it replaces and
beside its floor, on the same box and the same models:

  * cbo_gp_mes_gumbel_sets: the Gumbel fit of every set in one call -- against cbo_gp_fit + cbo_gp_mes_gumbel, set by set;
  * cbo_acq_sweep_sets_mes: every set scored in one launch -- against cbo_acq_sweep_mes per fitted set (the fit of the
    per-set Gumbel sequence is the one it sweeps on: a fresh fit every round, so no cached solution is reused);
  * cbo_acq_sweep_sets (the causal EI: the same kernel with the EI epilogue) as the floor.

Every figure is the host's clock around one whole call (each call ends with its results on the host): --warmup unrecorded
calls per variant, then the variants ALTERNATE for --reps rounds, and the median, min and max per variant are reported in
microseconds.

    python scripts/sets_mes_timing.py --out profiles/sets_mes_timing.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = [2, 6, 25]
N, M, D, K, GRID = 50, 200, 1, 10, 5000


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_mes_timing.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    ctx = _lib.Context.get()
    report = {"device": ctx.name(), "n": N, "m": M, "d": D, "num_samples": K, "gumbel_grid_points": N + GRID,
              "warmup": a.warmup, "clock": "time.perf_counter_ns around one whole call, variants alternating", "calls_us": {}}
    for s in SETS:
        rng = np.random.default_rng(s)
        models, grids, gumbel_points, gumbel_grids = [], [], [], []
        for _ in range(s):
            X = rng.uniform(-5.0, 5.0, (N, D))
            y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
            models.append(HipGaussianProcess(X, y, noise_var=1e-2, fit=False))
            grids.append(CandidateGrid(np.linspace(-5.0, 5.0, M)[:, None] * np.ones((1, D)), models[-1]))
            gumbel_points.append(_lib.as_f64(np.vstack([X, rng.uniform(-5.0, 5.0, (GRID, D))])))
            gumbel_grids.append(CandidateGrid(gumbel_points[-1], models[-1]))
        gps = (ctypes.c_void_p * s)(*[m._handle for m in models])
        cds = (ctypes.c_void_p * s)(*[g._handle for g in grids])
        gds = (ctypes.c_void_p * s)(*[g._handle for g in gumbel_grids])
        y_best, costs = np.full(s, float(np.median(models[0].Y))), np.ones(s)
        vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
        yb, cs, vp, ip = _lib.dptr(y_best), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
        bv, bi = ctypes.c_double(), ctypes.c_int64()
        q, ga, gb = np.empty((s, 3)), np.empty(s), np.empty(s)
        q1, a1, b1 = np.empty(3), ctypes.c_double(), ctypes.c_double()

        def gumbel_sets():
            _lib.check(lib.cbo_gp_mes_gumbel_sets(s, gps, gds, _lib.dptr(q), _lib.dptr(ga), _lib.dptr(gb)))

        def gumbel_per_set():
            for m, pts in zip(models, gumbel_points):
                _lib.check(lib.cbo_gp_fit(m._handle, None, None))
                _lib.check(lib.cbo_gp_mes_gumbel(m._handle, pts.shape[0], _lib.dptr(pts), None, None, _lib.dptr(q1),
                                                 ctypes.byref(a1), ctypes.byref(b1), None, None))

        # the samples every scoring variant uses: from the sets' own Gumbel fits
        gumbel_sets()
        u = rng.random((s, K))
        mins = [np.ascontiguousarray(np.log(-np.log(1 - u[i])) * gb[i] + ga[i]) for i in range(s)]
        counts = (ctypes.c_int * s)(*[K] * s)
        ptrs = (ctypes.c_void_p * s)(*[m.ctypes.data for m in mins])

        def sets_ei():
            _lib.check(lib.cbo_acq_sweep_sets(s, gps, cds, yb, 0, 0.0, cs, vp, ip))

        def mes_sets():
            _lib.check(lib.cbo_acq_sweep_sets_mes(s, gps, cds, counts, ptrs, cs, vp, ip))

        def mes_per_set():
            for m, g, mn in zip(models, grids, mins):
                _lib.check(lib.cbo_acq_sweep_mes(m._handle, g._handle, K, _lib.dptr(mn), 1.0, None, None, None,
                                                 ctypes.byref(bv), ctypes.byref(bi)))

        # (the per-set Gumbel sequence goes first in every round: it leaves the fresh fits the per-set scoring sweeps on)
        variants = {"Gumbel fits per set (cbo_gp_fit + cbo_gp_mes_gumbel)": gumbel_per_set,
                    "Gumbel fits one call (cbo_gp_mes_gumbel_sets)": gumbel_sets,
                    "MES per fitted set (cbo_acq_sweep_mes)": mes_per_set,
                    "MES one launch (cbo_acq_sweep_sets_mes)": mes_sets,
                    "EI one launch (cbo_acq_sweep_sets)": sets_ei}
        for call in variants.values():
            for _ in range(a.warmup):
                call()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, call in variants.items():
                t0 = time.perf_counter_ns()
                call()
                times[k].append((time.perf_counter_ns() - t0) * 1e-3)
        row = report["calls_us"][f"{s} sets"] = {k: stats(v) for k, v in times.items()}
        print(f"{s} sets", json.dumps({k: round(v["median"], 1) for k, v in row.items()}), flush=True)
        for o in grids + gumbel_grids + models:
            o.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
