"""Timing of the constrained acquisition in the one-launch multi-set sweep (cbo_acq_sweep_sets_constrained,
kernels_sets_con.hip) on one MI355X, at BASELINE config 1's shape -- 50 observations and 200 candidates per set -- for 2, 6
and 25 sets with 0, 1, 2 and 4 constraints each, beside what it replaces and beside its floor, on the same box and the same
models:

  * cbo_acq_sweep_sets_constrained: one call for all sets and all their models;
  * the per-set sequence the call replaces: cbo_gp_fit on every model of the set, then cbo_acq_sweep_constrained, set by set;
  * cbo_acq_sweep_sets (the causal EI: small_sets_kernel of kernels_sets.hip, the same stages for one model) as the floor, in the rows
    without constraints.

Every figure is the host's clock around one whole call (each call ends with its results on the host: the multi-set calls
poll their pinned result records, the per-set calls synchronise their stream): --warmup unrecorded calls per variant, then the
variants ALTERNATE for --reps rounds, and the median, min and max per variant are reported in microseconds.

    python scripts/sets_constrained_timing.py --out profiles/sets_constrained_timing.json
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
N_CON = [0, 1, 2, 4]
N, M, D = 50, 200, 1


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_constrained_timing.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    ctx = _lib.Context.get()
    report = {"device": ctx.name(), "n": N, "m": M, "d": D, "warmup": a.warmup,
              "clock": "time.perf_counter_ns around one whole call, variants alternating", "calls_us": {}}
    pts = np.linspace(-5.0, 5.0, M)[:, None] * np.ones((1, D))
    for s in SETS:
        for k in N_CON:
            rng = np.random.default_rng(100 * s + k)

            def pair(f):
                X = rng.uniform(-5.0, 5.0, (N, D))
                y = f(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
                model = HipGaussianProcess(X, y, noise_var=1e-2, fit=False)
                return model, CandidateGrid(pts, model)
            objectives = [pair(np.sin) for _ in range(s)]
            cons = [[pair(np.cos) for _ in range(k)] for _ in range(s)]
            flat = [p for row in cons for p in row]
            gps = (ctypes.c_void_p * s)(*[m._handle for m, _ in objectives])
            cds = (ctypes.c_void_p * s)(*[g._handle for _, g in objectives])
            cgp = (ctypes.c_void_p * max(1, s * k))(*[m._handle for m, _ in flat])
            ccd = (ctypes.c_void_p * max(1, s * k))(*[g._handle for _, g in flat])
            n_con = (ctypes.c_int * s)(*([k] * s))
            values, jitters = np.full(max(1, s * k), 0.3), np.zeros(max(1, s * k))
            senses = (ctypes.c_int * max(1, s * k))(*[i % 2 for i in range(s * k)])
            y_best, costs = np.full(s, float(np.median(objectives[0][0].Y))), np.ones(s)
            vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
            yb, cs, vp, ip = _lib.dptr(y_best), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
            vd, jd = _lib.dptr(values), _lib.dptr(jitters)
            bv, bi = ctypes.c_double(), ctypes.c_int64()

            def one_launch():
                _lib.check(lib.cbo_acq_sweep_sets_constrained(s, gps, cds, yb, 0, 0.0, cs, n_con, cgp, ccd, vd, jd, senses, vp,
                                                              ip))

            # the per-set call's slices, made once (the sequence is not charged for building them)
            slices = []
            for i in range(s):
                sl = slice(i * k, (i + 1) * k)
                v, j = np.ascontiguousarray(values[sl]), np.ascontiguousarray(jitters[sl])
                slices.append(((ctypes.c_void_p * max(1, k))(*cgp[sl]), (ctypes.c_void_p * max(1, k))(*ccd[sl]), v, j,
                               _lib.dptr(v) if k else None, _lib.dptr(j) if k else None,
                               (ctypes.c_int * max(1, k))(*senses[sl])))

            def per_set():
                for i, (m, g) in enumerate(objectives):
                    _lib.check(lib.cbo_gp_fit(m._handle, None, None))
                    for cm, _ in cons[i]:
                        _lib.check(lib.cbo_gp_fit(cm._handle, None, None))
                    g_arr, c_arr, _, _, v_ptr, j_ptr, s_arr = slices[i]
                    _lib.check(lib.cbo_acq_sweep_constrained(m._handle, g._handle, y_best[0], 0, 0.0, 1.0, k, g_arr, c_arr,
                                                             v_ptr, j_ptr, s_arr, None, None, None, ctypes.byref(bv),
                                                             ctypes.byref(bi)))

            def sets_ei():
                _lib.check(lib.cbo_acq_sweep_sets(s, gps, cds, yb, 0, 0.0, cs, vp, ip))

            variants = {"one launch (cbo_acq_sweep_sets_constrained)": one_launch,
                        "per set (cbo_gp_fit on every model + cbo_acq_sweep_constrained)": per_set}
            if k == 0:
                variants["EI one launch (cbo_acq_sweep_sets), the floor"] = sets_ei
            for call in variants.values():
                for _ in range(a.warmup):
                    call()
            times = {name: [] for name in variants}
            for _ in range(a.reps):
                for name, call in variants.items():
                    t0 = time.perf_counter_ns()
                    call()
                    times[name].append((time.perf_counter_ns() - t0) * 1e-3)
            row = report["calls_us"][f"{s} sets, {k} constraints"] = {name: stats(v) for name, v in times.items()}
            print(f"{s} sets, {k} constraints", json.dumps({name: round(v["median"], 1) for name, v in row.items()}), flush=True)
            for m, g in objectives + flat:
                g.close()
                m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
