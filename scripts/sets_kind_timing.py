"""Timing of the point-wise acquisitions in the one-launch multi-set sweep (cbo_acq_sweep_sets_kind, kernels_sets.hip) on
one MI355X, at BASELINE config 1's shape -- 2 exploration sets x 200 candidates x 50 observations -- and at 6 and 25 sets of
that shape, beside what it replaces and beside its floor, on the same box and the same models:

  * cbo_acq_sweep_sets_kind per kind (LCB, PI, VAR, MPEI): one call for all sets;
  * the per-set sequence the call replaces: cbo_gp_fit + cbo_acq_sweep_kind, set by set;
  * cbo_acq_sweep_sets (the causal EI: small_sets_kernel<kEiKind>, the same kernel with the EI epilogue) as the floor.

Every figure is the host's clock around one whole call (each call ends with its results on the host: the multi-set calls
poll their pinned result records, the per-set calls synchronise their stream): --warmup unrecorded calls per variant, then the
variants ALTERNATE for --reps rounds, and the median, min and max per variant are reported in microseconds.

    python scripts/sets_kind_timing.py --out profiles/sets_kind_timing.json
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
N, M, D = 50, 200, 1
KINDS = (("LCB", 1, 1.0), ("PI", 2, 0.0), ("VAR", 3, 0.0), ("MPEI", 4, 0.0))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_kind_timing.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    ctx = _lib.Context.get()
    report = {"device": ctx.name(), "n": N, "m": M, "d": D, "warmup": a.warmup,
              "clock": "time.perf_counter_ns around one whole call, variants alternating", "calls_us": {}}
    for s in SETS:
        rng = np.random.default_rng(s)
        models, grids = [], []
        for _ in range(s):
            X = rng.uniform(-5.0, 5.0, (N, D))
            y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
            models.append(HipGaussianProcess(X, y, noise_var=1e-2, fit=False))
            grids.append(CandidateGrid(np.linspace(-5.0, 5.0, M)[:, None] * np.ones((1, D)), models[-1]))
        gps = (ctypes.c_void_p * s)(*[m._handle for m in models])
        cds = (ctypes.c_void_p * s)(*[g._handle for g in grids])
        y_best, costs = np.full(s, float(np.median(models[0].Y))), np.ones(s)
        vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
        yb, cs, vp, ip = _lib.dptr(y_best), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
        bv, bi = ctypes.c_double(), ctypes.c_int64()

        def sets_ei():
            _lib.check(lib.cbo_acq_sweep_sets(s, gps, cds, yb, 0, 0.0, cs, vp, ip))

        def sets_kind(kind, param):
            return lambda: _lib.check(lib.cbo_acq_sweep_sets_kind(s, gps, cds, kind, yb, 0, param, cs, vp, ip))

        def per_set(kind, param):
            def run():
                for m, g in zip(models, grids):
                    _lib.check(lib.cbo_gp_fit(m._handle, None, None))
                    _lib.check(lib.cbo_acq_sweep_kind(m._handle, g._handle, kind, y_best[0], 0, param, 1.0, None, None, None,
                                                      ctypes.byref(bv), ctypes.byref(bi)))
            return run

        variants = {"EI one launch (cbo_acq_sweep_sets)": sets_ei}
        for name, kind, param in KINDS:
            variants[f"{name} one launch (cbo_acq_sweep_sets_kind)"] = sets_kind(kind, param)
        for name, kind, param in KINDS:
            variants[f"{name} per set (cbo_gp_fit + cbo_acq_sweep_kind)"] = per_set(kind, param)
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
        for o in grids + models:
            o.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
