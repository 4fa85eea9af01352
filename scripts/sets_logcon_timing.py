"""Timing of the constrained acquisition in log space on one MI355X, the log form beside the product form,
in one run with the two forms alternating:

  (a) the general pass at m = 2^24 candidates with 0, 1, 2 and 4 constraints (non-causal models, no per-candidate outputs):
      every (model, candidate set) pair is cached, so a call is constrained_acq_kernel -- its log or its product
      instantiation -- plus argmax_final_kernel.  Device time between cbo_region_begin and cbo_region_end around one call.
  (b) the one launch (small_sets_con_kernel) at 2, 6 and 25 sets of 50 observations x 200 candidates with the same numbers
      of constraints per set, unfitted models: the host's clock around one whole call, which ends with the results on the
      host.

    python scripts/sets_logcon_timing.py --out profiles/sets_logcon_timing.json
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

M_PASS, N_PASS, D_PASS = 1 << 24, 64, 3
SETS = [2, 6, 25]
N_CON = [0, 1, 2, 4]
N, M, D = 50, 200, 1
FORMS = {"log": "cbo_acq_sweep_constrained_log", "product": "cbo_acq_sweep_constrained"}
SETS_FORMS = {"log": "cbo_acq_sweep_sets_constrained_log", "product": "cbo_acq_sweep_sets_constrained"}


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def general_pass(report, reps):
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib, ctx = _lib.load(), _lib.Context.get()
    rng = np.random.default_rng(1)
    pts = rng.uniform(-2.0, 2.0, (M_PASS, D_PASS))

    def model(seed):
        X = rng.uniform(-2.0, 2.0, (N_PASS, D_PASS))
        y = np.sin(X + seed).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N_PASS, 1))
        return HipGaussianProcess(X, y, noise_var=1e-2)
    models = [model(k) for k in range(1 + max(N_CON))]
    grids = [CandidateGrid(pts, g) for g in models]
    y_best = float(models[0].Y.min())
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    out = report["general_pass_ms"] = {"m": M_PASS, "n_model": N_PASS, "d": D_PASS, "reps": reps,
                                       "clock": "cbo_region_begin / cbo_region_end around one call, forms alternating"}
    for k in N_CON:
        gps = (ctypes.c_void_p * max(1, k))(*[g._handle for g in models[1:1 + k]])
        cds = (ctypes.c_void_p * max(1, k))(*[g._handle for g in grids[1:1 + k]])
        values, jitters = np.array([0.1 * (c - 1) for c in range(max(1, k))]), np.zeros(max(1, k))
        senses = (ctypes.c_int * max(1, k))(*[c % 2 for c in range(max(1, k))])

        def call(name):
            _lib.check(getattr(lib, name)(models[0]._handle, grids[0]._handle, y_best, 0, 0.0, 2.0, k, gps if k else None,
                                          cds if k else None, _lib.dptr(values) if k else None,
                                          _lib.dptr(jitters) if k else None, senses if k else None, None, None, None,
                                          ctypes.byref(bv), ctypes.byref(bi)))
        times = {form: [] for form in FORMS}
        for i in range(reps + 1):                                   # (round 0: every pair's vectors are cached from here on)
            for form, name in FORMS.items():
                ctx.region_begin()
                call(name)
                ms = ctx.region_end()
                if i:
                    times[form].append(ms)
        row = out[f"{k} constraints"] = {form: stats(v) for form, v in times.items()}
        row["log_over_product"] = row["log"]["median"] / row["product"]["median"]
        print(f"general pass, {k} constraints", json.dumps({f: round(row[f]["median"], 4) for f in FORMS}), flush=True)
    for o in grids + models:
        o.close()


def one_launch(report, reps, warmup):
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    out = report["one_launch_us"] = {"n": N, "m": M, "d": D, "reps": reps, "warmup": warmup,
                                     "clock": "time.perf_counter_ns around one whole call, forms alternating"}
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
            flat = [pair(np.cos) for _ in range(s * k)]
            gps = (ctypes.c_void_p * s)(*[m._handle for m, _ in objectives])
            cds = (ctypes.c_void_p * s)(*[g._handle for _, g in objectives])
            cgp = (ctypes.c_void_p * max(1, s * k))(*[m._handle for m, _ in flat])
            ccd = (ctypes.c_void_p * max(1, s * k))(*[g._handle for _, g in flat])
            n_con = (ctypes.c_int * s)(*([k] * s))
            values, jitters = np.full(max(1, s * k), 0.3), np.zeros(max(1, s * k))
            senses = (ctypes.c_int * max(1, s * k))(*[i % 2 for i in range(s * k)])
            y_best, costs = np.full(s, float(np.median(objectives[0][0].Y))), np.full(s, 2.0)
            vals, idxs = np.empty(s), np.empty(s, dtype=np.int64)

            def call(name):
                _lib.check(getattr(lib, name)(s, gps, cds, _lib.dptr(y_best), 0, 0.0, _lib.dptr(costs), n_con, cgp, ccd,
                                              _lib.dptr(values), _lib.dptr(jitters), senses, _lib.dptr(vals),
                                              idxs.ctypes.data_as(_lib.c_int64_p)))
            for name in SETS_FORMS.values():
                for _ in range(warmup):
                    call(name)
            times = {form: [] for form in SETS_FORMS}
            for _ in range(reps):
                for form, name in SETS_FORMS.items():
                    t0 = time.perf_counter_ns()
                    call(name)
                    times[form].append((time.perf_counter_ns() - t0) * 1e-3)
            row = out[f"{s} sets, {k} constraints"] = {form: stats(v) for form, v in times.items()}
            row["log_over_product"] = row["log"]["median"] / row["product"]["median"]
            print(f"one launch, {s} sets, {k} constraints", json.dumps({f: round(row[f]["median"], 1) for f in SETS_FORMS}),
                  flush=True)
            for m, g in objectives + flat:
                g.close()
                m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_logcon_timing.json"))
    ap.add_argument("--pass-reps", type=int, default=15)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    a = ap.parse_args()
    from cbo_with_oop_amd import _lib
    report = {"device": _lib.Context.get().name()}
    general_pass(report, a.pass_reps)
    one_launch(report, a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
