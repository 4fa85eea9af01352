"""Timing of the hyper-marginalised EI in log space (cbo_acq_sweep_sets_hyper_log / cbo_acq_sweep_hyper_log, the log
instantiations of kernels_hyper.hip) on one MI355X, by scripts/sets_hyper_timing.py's method and at its
shapes -- 50 observations and 200 candidates per set, d = 1, for 2, 6 and 25 sets with 1, 10 and 50 samples each -- beside
the EI form and beside what the one call replaces, on the same box and the same models:

  * cbo_acq_sweep_sets_hyper_log: one call for all sets and all their samples;
  * cbo_acq_sweep_sets_hyper: the EI form's one call (the same stages, acquisition_of and a sum in the epilogue);
  * the per-set sequence the log call replaces: cbo_acq_sweep_hyper_log, set by set.

Then the single-set call at 128 observations, 16384 candidates (256 candidate blocks) and 10 samples, d = 3, log form and EI
form, under both schedules (CBO_HIP_HYPER_SCHEDULE = 1: every workgroup factors every sample; 2: two launches), each schedule
on a context of its own.

Every figure is the host's clock around one whole call (each call ends with its results on the host): --warmup unrecorded
calls per variant, then the variants ALTERNATE for --reps rounds, and the median, min and max per variant are reported in
microseconds, with the ratio of the log form's median to the EI form's.  Condition: the one call's median is below the
per-set sequence's in every row.

    python scripts/hyper_log_timing.py --out profiles/hyper_log_timing.json
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
BIG_N, BIG_M, BIG_D, BIG_H = 128, 16384, 3, 10
LOG, EI, PER_SET = ("log form, one launch (cbo_acq_sweep_sets_hyper_log)", "EI form, one launch (cbo_acq_sweep_sets_hyper)",
                    "log form per set (cbo_acq_sweep_hyper_log, set by set)")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def alternate(variants, warmup, reps):
    for call in variants.values():
        for _ in range(warmup):
            call()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, call in variants.items():
            t0 = time.perf_counter_ns()
            call()
            times[name].append((time.perf_counter_ns() - t0) * 1e-3)
    return {name: stats(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyper_log_timing.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    ctx = _lib.Context.get()
    report = {"device": ctx.name(), "n": N, "m": M, "d": D, "warmup": a.warmup,
              "clock": "time.perf_counter_ns around one whole call, variants alternating", "calls_us": {},
              "log_over_ei": {}, "acceptance": {}, "single_set": {}}
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

            def log_form():
                _lib.check(lib.cbo_acq_sweep_sets_hyper_log(s, gps, cds, counts, ptrs, yb, 0, 0.0, cs, vp, ip))

            def ei_form():
                _lib.check(lib.cbo_acq_sweep_sets_hyper(s, gps, cds, counts, ptrs, yb, 0, 0.0, cs, vp, ip))

            def per_set():
                for i, (m, g) in enumerate(pairs):
                    _lib.check(lib.cbo_acq_sweep_hyper_log(m._handle, g._handle, h, row_ptrs[i], y_best[0], 0, 0.0, 1.0, None,
                                                           ctypes.byref(bv), ctypes.byref(bi)))

            key = f"{s} sets, {h} samples"
            row = report["calls_us"][key] = alternate({LOG: log_form, EI: ei_form, PER_SET: per_set}, a.warmup, a.reps)
            report["acceptance"][key] = bool(row[LOG]["median"] < row[PER_SET]["median"])
            report["log_over_ei"][key] = row[LOG]["median"] / row[EI]["median"]
            print(key, json.dumps({name: round(v["median"], 1) for name, v in row.items()}),
                  "log / EI", round(report["log_over_ei"][key], 3), flush=True)
            for m, g in pairs:
                g.close()
                m.close()
    # the single-set call under both schedules, each on a context of its own (the schedule is read when a context is made)
    rng = np.random.default_rng(7)
    X = rng.uniform(-2.0, 2.0, (BIG_N, BIG_D))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((BIG_N, 1))
    Xs = rng.uniform(-2.0, 2.0, (BIG_M, BIG_D))
    rows = np.ascontiguousarray(np.array([1.0, 1.0, 2e-2]) * 2.0 ** rng.uniform(-1.0, 1.0, (BIG_H, 3)))
    y_best = float(np.median(y))
    for schedule in ("1", "2"):
        os.environ["CBO_HIP_HYPER_SCHEDULE"] = schedule
        own = _lib.Context(ctx.device_id)
        model = HipGaussianProcess(X, y, noise_var=1e-2, fit=False, context=own)
        grid = CandidateGrid(Xs, model)
        bv, bi = ctypes.c_double(), ctypes.c_int64()

        def single(call):
            return lambda: _lib.check(call(model._handle, grid._handle, BIG_H, _lib.dptr(rows), y_best, 0, 0.0, 1.0, None,
                                           ctypes.byref(bv), ctypes.byref(bi)))
        row = alternate({"log form (cbo_acq_sweep_hyper_log)": single(lib.cbo_acq_sweep_hyper_log),
                         "EI form (cbo_acq_sweep_hyper)": single(lib.cbo_acq_sweep_hyper)}, a.warmup, max(a.reps // 4, 1))
        ratio = row["log form (cbo_acq_sweep_hyper_log)"]["median"] / row["EI form (cbo_acq_sweep_hyper)"]["median"]
        key = f"n {BIG_N}, m {BIG_M}, d {BIG_D}, {BIG_H} samples, schedule {schedule}"
        report["single_set"][key] = dict(row, log_over_ei=ratio)
        print(key, json.dumps({name: round(v["median"], 1) for name, v in row.items()}), "log / EI", round(ratio, 3), flush=True)
        grid.close()
        model.close()
        own.close()
    del os.environ["CBO_HIP_HYPER_SCHEDULE"]
    report["accepted"] = all(report["acceptance"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({"accepted": report["accepted"], "log_over_ei": report["log_over_ei"]}, indent=1))


if __name__ == "__main__":
    main()
