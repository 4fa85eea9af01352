"""Timing of the hyper-parameter-marginalised EI in the one-launch multi-set sweep (cbo_acq_sweep_sets_hyper,
hyper_sets_kernel of kernels_hyper.hip) on one MI355X, at BASELINE config 1's shape -- 50 observations and 200 candidates
per set, d = 1 -- for 2, 6 and 25 sets with 1, 10 and 50 samples each, beside what it replaces and beside its floor, on the
same box and the same models:

  * cbo_acq_sweep_sets_hyper: one call for all sets and all their samples;
  * the per-set sequence the call replaces: cbo_acq_sweep_hyper, set by set (one launch, one copy of the rows into the
    pinned buffer and one poll of the result record per set);
  * cbo_acq_sweep_sets (the causal EI at the models' own hyper-parameters: small_sets_kernel, the same stages once) as the
    floor.

Every figure is the host's clock around one whole call (each call ends with its results on the host: every variant polls
its pinned result records): --warmup unrecorded calls per variant, then the variants ALTERNATE for --reps rounds, and the
median, min and max per variant are reported in microseconds.  Per number of sets the walk's price per added sample,
(t(H = 50) - t(H = 10)) / 40 of the one call's medians, is recorded too: what a sample-parallel grid would go after.

    python scripts/sets_hyper_timing.py --out profiles/sets_hyper_timing.json
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
SAMPLES = [1, 10, 50]
N, M, D = 50, 200, 1
ONE, PER_SET, FLOOR = ("one launch (cbo_acq_sweep_sets_hyper)", "per set (cbo_acq_sweep_hyper, set by set)",
                       "EI one launch (cbo_acq_sweep_sets), the floor")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_hyper_timing.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    ctx = _lib.Context.get()
    report = {"device": ctx.name(), "n": N, "m": M, "d": D, "warmup": a.warmup,
              "clock": "time.perf_counter_ns around one whole call, variants alternating", "calls_us": {},
              "us_per_added_sample": {}, "acceptance": {}}
    pts = np.linspace(-5.0, 5.0, M)[:, None] * np.ones((1, D))
    for s in SETS:
        for h in SAMPLES:
            rng = np.random.default_rng(100 * s + h)
            pairs = []
            for _ in range(s):
                X = rng.uniform(-5.0, 5.0, (N, D))
                y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
                model = HipGaussianProcess(X, y, noise_var=1e-2, fit=False)
                pairs.append((model, CandidateGrid(pts, model)))
            # (variance, lengthscale, noise) within a factor of two of the models' own (1, 1, 1e-2)
            rows = [np.ascontiguousarray(np.array([1.0, 1.0, 2e-2]) * 2.0 ** rng.uniform(-1.0, 1.0, (h, 3))) for _ in range(s)]
            gps = (ctypes.c_void_p * s)(*[m._handle for m, _ in pairs])
            cds = (ctypes.c_void_p * s)(*[g._handle for _, g in pairs])
            counts = (ctypes.c_int * s)(*([h] * s))
            ptrs = (ctypes.c_void_p * s)(*[r.ctypes.data for r in rows])
            row_ptrs = [_lib.dptr(r) for r in rows]
            y_best, costs = np.full(s, float(np.median(pairs[0][0].Y))), np.ones(s)
            vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
            yb, cs, vp, ip = _lib.dptr(y_best), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
            bv, bi = ctypes.c_double(), ctypes.c_int64()

            def one_launch():
                _lib.check(lib.cbo_acq_sweep_sets_hyper(s, gps, cds, counts, ptrs, yb, 0, 0.0, cs, vp, ip))

            def per_set():
                for i, (m, g) in enumerate(pairs):
                    _lib.check(lib.cbo_acq_sweep_hyper(m._handle, g._handle, h, row_ptrs[i], y_best[0], 0, 0.0, 1.0, None,
                                                       ctypes.byref(bv), ctypes.byref(bi)))

            def sets_ei():
                _lib.check(lib.cbo_acq_sweep_sets(s, gps, cds, yb, 0, 0.0, cs, vp, ip))

            variants = {ONE: one_launch, PER_SET: per_set, FLOOR: sets_ei}
            for call in variants.values():
                for _ in range(a.warmup):
                    call()
            times = {name: [] for name in variants}
            for _ in range(a.reps):
                for name, call in variants.items():
                    t0 = time.perf_counter_ns()
                    call()
                    times[name].append((time.perf_counter_ns() - t0) * 1e-3)
            key = f"{s} sets, {h} samples"
            row = report["calls_us"][key] = {name: stats(v) for name, v in times.items()}
            report["acceptance"][key] = bool(row[ONE]["median"] < row[PER_SET]["median"])
            print(key, json.dumps({name: round(v["median"], 1) for name, v in row.items()}), flush=True)
            for m, g in pairs:
                g.close()
                m.close()
        t10 = report["calls_us"][f"{s} sets, 10 samples"][ONE]["median"]
        t50 = report["calls_us"][f"{s} sets, 50 samples"][ONE]["median"]
        report["us_per_added_sample"][f"{s} sets"] = (t50 - t10) / 40.0
    report["accepted"] = all(report["acceptance"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
