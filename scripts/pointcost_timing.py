"""Timing of the per-candidate cost pass on one MI355X beside the EI's, same box, same models, same run:

  * the candidate pass alone at 2^24 candidates (stored q, mu): cbo_acq_sweep_pointcost, both forms (pointcost_acq_kernel:
    acq_pass with the cost vector as a fifth 8-byte stream) beside cbo_acq_sweep (acq_kernel), the library's own event timer
    around the pass (``ms_acq``), acquisition values stored and not stored, alternating, --pass-reps passes each; the
    fraction of an 8 TB/s HBM roofline is taken at 24 + 8 bytes per candidate (stored) and 16 + 8 (not stored) for the new
    pass, 24 and 16 for the EI's;
  * the one-launch multi-set sweep at 2, 6 and 25 sets of 50 observations x 200 candidates (BASELINE config 1's shape):
    cbo_acq_sweep_sets_pointcost, both forms, beside cbo_acq_sweep_sets and cbo_acq_sweep_sets_logei, the host's clock around
    one whole call, --warmup unrecorded calls, then alternating for --reps rounds.

    python scripts/pointcost_timing.py --out profiles/pointcost_timing.json
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
N, M = 50, 200


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def set_cost(_lib, lib, grid, d):
    fix, flags = np.ones(d), np.ones(d, dtype=np.int32)
    _lib.check(lib.cbo_cands_set_cost(grid._handle, _lib.dptr(fix), flags.ctypes.data_as(_lib.c_int_p)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcost_timing.json"))
    ap.add_argument("--log2m", type=int, default=24)
    ap.add_argument("--pass-reps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    ctx = _lib.Context.get(0)
    report = {"device": ctx.name(), "pass": {}, "sets": {}}

    # ---- the pass alone
    m = 1 << a.log2m
    Xe = np.random.default_rng(3).uniform(-5.0, 5.0, (64, 3))
    ye = np.sin(Xe).sum(1, keepdims=True)
    model = HipGaussianProcess(Xe, ye, context=ctx)
    grid = CandidateGrid(np.random.default_rng(4).uniform(-5.0, 5.0, (m, 3)), model, context=ctx)
    set_cost(_lib, lib, grid, 3)
    acq = np.empty(m)
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    y_best = float(ye.min())

    def ei_pass(out):
        _lib.check(lib.cbo_acq_sweep(model._handle, grid._handle, y_best, 0, 0.0, 3.0, _lib.dptr(acq) if out else None, None,
                                     None, ctypes.byref(bv), ctypes.byref(bi)))

    def pointcost_pass(log_form):
        def call(out):
            _lib.check(lib.cbo_acq_sweep_pointcost(model._handle, grid._handle, log_form, y_best, 0, 0.0,
                                                   _lib.dptr(acq) if out else None, None, None, ctypes.byref(bv),
                                                   ctypes.byref(bi)))
        return call

    def timed(call, out):
        ctx.set_profiling(True)
        ctx.reset_timers()
        call(out)
        ms = ctx.timers()["ms_acq"]
        ctx.set_profiling(False)
        return ms * 1e3

    passes = {"EI (cbo_acq_sweep)": (ei_pass, 0.0), "EI / c(x) (cbo_acq_sweep_pointcost, log_form 0)": (pointcost_pass(0), 8.0),
              "log EI - log c(x) (cbo_acq_sweep_pointcost, log_form 1)": (pointcost_pass(1), 8.0)}
    report["pass"] = {"candidates": m, "clock": "the library's event timer around the pass (ms_acq), variants alternating",
                      "hbm_bytes_per_candidate": {"stored": "24 (+ 8 with the cost stream)", "not stored": "16 (+ 8)"}, "us": {}}
    for out in (True, False):
        for call, _ in passes.values():
            call(out)
            call(out)
        times = {k: [] for k in passes}
        for _ in range(a.pass_reps):
            for k, (call, _) in passes.items():
                times[k].append(timed(call, out))
        row = report["pass"]["us"]["stored" if out else "not stored"] = {k: stats(v) for k, v in times.items()}
        for k, v in row.items():
            v["bytes_per_candidate"] = (24.0 if out else 16.0) + passes[k][1]
            v["fraction_of_8TBps"] = v["bytes_per_candidate"] * m / (v["median"] * 1e-6) / 8e12
        print("pass, acquisition values", "stored" if out else "not stored",
              json.dumps({k: (round(v["median"], 1), round(v["fraction_of_8TBps"], 3)) for k, v in row.items()}), flush=True)
    grid.close()
    model.close()

    # ---- the one-launch multi-set sweep
    report["sets"] = {"n": N, "m": M, "d": 1, "noise_var": 1e-10, "warmup": a.warmup,
                      "clock": "time.perf_counter_ns around one whole call, variants alternating", "calls_us": {}}
    for s in SETS:
        rng = np.random.default_rng(7 + s)
        models, grids = [], []
        for _ in range(s):
            X = rng.uniform(-5.0, 20.0, (N, 1))
            y = np.cos(X) - np.exp(-X / 20.0)
            models.append(HipGaussianProcess(X, y, noise_var=1e-10, fit=False))
            grids.append(CandidateGrid(np.linspace(-5.0, 20.0, M)[:, None], models[-1]))
            set_cost(_lib, lib, grids[-1], 1)
        gps = (ctypes.c_void_p * s)(*[g._handle for g in models])
        cds = (ctypes.c_void_p * s)(*[g._handle for g in grids])
        yb_arr, costs = np.array([float(g.Y.min()) for g in models]), np.ones(s)
        vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)
        yb, cs, vp, ip = _lib.dptr(yb_arr), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
        variants = {"EI one launch (cbo_acq_sweep_sets)": lambda: _lib.check(lib.cbo_acq_sweep_sets(s, gps, cds, yb, 0, 0.0, cs, vp, ip)),
                    "EI / c(x) one launch (cbo_acq_sweep_sets_pointcost, log_form 0)":
                        lambda: _lib.check(lib.cbo_acq_sweep_sets_pointcost(s, gps, cds, 0, yb, 0, 0.0, vp, ip)),
                    "log EI one launch (cbo_acq_sweep_sets_logei)":
                        lambda: _lib.check(lib.cbo_acq_sweep_sets_logei(s, gps, cds, yb, 0, 0.0, cs, vp, ip)),
                    "log EI - log c(x) one launch (cbo_acq_sweep_sets_pointcost, log_form 1)":
                        lambda: _lib.check(lib.cbo_acq_sweep_sets_pointcost(s, gps, cds, 1, yb, 0, 0.0, vp, ip))}
        for call in variants.values():
            for _ in range(a.warmup):
                call()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, call in variants.items():
                t0 = time.perf_counter_ns()
                call()
                times[k].append((time.perf_counter_ns() - t0) * 1e-3)
        row = report["sets"]["calls_us"][f"{s} sets"] = {k: stats(v) for k, v in times.items()}
        print(f"{s} sets", json.dumps({k: round(v["median"], 1) for k, v in row.items()}), flush=True)
        for o in grids + models:
            o.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
