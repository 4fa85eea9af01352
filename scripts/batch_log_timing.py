"""Timing of greedy batch selection in log space beside the EI form it mirrors, on one MI355X, the two forms
ALTERNATING in one run:

  general path   cbo_acq_sweep_batch / cbo_acq_sweep_batch_logei at the headline shape (4096 observations x 16384 candidates,
                 d = 3, fp64, a kept solution: no substitution is timed), B = 1 / 4 / 8; device time between cbo_region_begin
                 and cbo_region_end; (B8 - B1) / 7 is the cost of one further pick
  one launch     cbo_acq_sweep_sets_batch / cbo_acq_sweep_sets_batch_logei for 2 / 6 / 25 sets of 50 x 200 (d = 1), B = 4,
                 beside the per-set sequences they replace (cbo_gp_fit + cbo_acq_sweep_batch[_logei], set by set); the host's
                 clock around one whole call

--warmup unrecorded calls per variant, then --reps rounds in which the variants alternate with a rotating start; medians,
quartiles, min and max per variant.  Every section is measured by a fresh child process under its own time limit; the first
child that fails or runs out of time ends the run (nothing more is started on the GPU) and the report says so.
--ei-only measures the EI rows alone: the same script then runs on a build that lacks the log entry points (the parent
commit), for the comparison of the EI rows between two builds.

    python scripts/batch_log_timing.py --out profiles/batch_log_timing.json
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENERAL = dict(n=4096, m_shape=[32, 32, 16], batches=[1, 4, 8])
SETS, SET_N, SET_M, SET_B = [2, 6, 25], 50, 200, 4


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "p25": float(np.percentile(v, 25)), "p75": float(np.percentile(v, 75)), "count": int(v.size)}


def alternate(variants, reps, warmup, timed):
    """{name: [time per call]}: the variants in turn, the round's first one rotating."""
    for call in variants.values():
        for _ in range(warmup):
            call()
    times = {k: [] for k in variants}
    names = list(variants)
    for r in range(reps):
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(timed(variants[k]))
    return times


def measure_general(reps, warmup, ei_only):
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    lib = _lib.load()
    box = [(-5.0, 5.0), (-5.0, 20.0), (-5.0, 5.0)]
    lo, hi = np.array([b[0] for b in box]), np.array([b[1] for b in box])
    rng = np.random.default_rng(0)
    X = rng.uniform(lo, hi, (GENERAL["n"], 3))
    y = (np.cos(np.exp(-X[:, 0] / 3)) + 0.3 * np.sin(X[:, 1]) + 0.3 * np.sin(X[:, 2]))[:, None]
    y = y + 0.1 * rng.standard_normal((GENERAL["n"], 1))
    g = HipGaussianProcess(X, y, noise_var=1e-2)
    grid = CandidateGrid(meshgrid_candidates(box, GENERAL["m_shape"]), g, keep_solution=True)
    ctx = _lib.Context.get()
    y_best = float(y.min())
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    _lib.check(lib.cbo_acq_sweep(g._handle, grid._handle, y_best, 0, 0.0, 1.0, None, None, None, ctypes.byref(bv),
                                 ctypes.byref(bi)))                                          # V resident
    picks = {}

    def variant(name, B):
        fn = getattr(lib, name)
        vals, idxs = np.empty(B), np.empty(B, dtype=np.int64)

        def call():
            _lib.check(fn(g._handle, grid._handle, y_best, 0, 0.0, 1.0, B, 0, _lib.dptr(vals),
                          idxs.ctypes.data_as(_lib.c_int64_p), None, None, None))
            picks[f"{name} B = {B}"] = idxs.tolist()
        return call

    names = ["cbo_acq_sweep_batch"] + ([] if ei_only else ["cbo_acq_sweep_batch_logei"])
    variants = {f"{name} B = {B}": variant(name, B) for B in GENERAL["batches"] for name in names}
    ms = ctypes.c_double()

    def timed(call):
        _lib.check(lib.cbo_region_begin(ctx.handle))
        call()
        _lib.check(lib.cbo_region_end(ctx.handle, ctypes.byref(ms)))
        return ms.value * 1e3

    times = alternate(variants, reps, warmup, timed)
    out = {"device": ctx.name(), "unit": "us, device time of one call", "calls_us": {k: stats(v) for k, v in times.items()},
           "picks": picks}
    lo_b, hi_b = GENERAL["batches"][0], GENERAL["batches"][-1]
    for name in names:
        out[f"{name}: one further pick, us"] = (out["calls_us"][f"{name} B = {hi_b}"]["median"] -
                                                out["calls_us"][f"{name} B = {lo_b}"]["median"]) / (hi_b - lo_b)
    grid.close(); g.close()
    return out


def measure_sets(s, reps, warmup, ei_only):
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
    rng = np.random.default_rng(s)
    models, grids = [], []
    for _ in range(s):
        X = rng.uniform(-5.0, 5.0, (SET_N, 1))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((SET_N, 1))
        models.append(HipGaussianProcess(X, y, noise_var=1e-2, fit=False))
        grids.append(CandidateGrid(np.linspace(-5.0, 5.0, SET_M)[:, None], models[-1]))
    gps = (ctypes.c_void_p * s)(*[m._handle for m in models])
    cds = (ctypes.c_void_p * s)(*[g._handle for g in grids])
    y_best, costs = np.full(s, float(np.median(models[0].Y))), np.ones(s)
    vals, idxs = np.empty(s * SET_B), np.empty(s * SET_B, dtype=np.int64)
    yb, cs, vp, ip = _lib.dptr(y_best), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
    one_v, one_i = np.empty(SET_B), np.empty(SET_B, dtype=np.int64)
    ovp, oip = _lib.dptr(one_v), one_i.ctypes.data_as(_lib.c_int64_p)

    def one_call(name):
        fn = getattr(lib, name)
        return lambda: _lib.check(fn(s, gps, cds, yb, 0, 0.0, cs, SET_B, 0, vp, ip))

    def per_set(name):
        fn = getattr(lib, name)

        def call():
            for m, g in zip(models, grids):
                _lib.check(lib.cbo_gp_fit(m._handle, None, None))
                _lib.check(fn(m._handle, g._handle, y_best[0], 0, 0.0, 1.0, SET_B, 0, ovp, oip, None, None, None))
        return call

    variants = {"one call, EI (cbo_acq_sweep_sets_batch)": one_call("cbo_acq_sweep_sets_batch"),
                "per set, EI (cbo_gp_fit + cbo_acq_sweep_batch)": per_set("cbo_acq_sweep_batch")}
    if not ei_only:
        variants["one call, log (cbo_acq_sweep_sets_batch_logei)"] = one_call("cbo_acq_sweep_sets_batch_logei")
        variants["per set, log (cbo_gp_fit + cbo_acq_sweep_batch_logei)"] = per_set("cbo_acq_sweep_batch_logei")

    def timed(call):
        t0 = time.perf_counter_ns()
        call()
        return (time.perf_counter_ns() - t0) * 1e-3

    times = alternate(variants, reps, warmup, timed)
    name = _lib.Context.get().name()
    for o in grids + models:
        o.close()
    return {"device": name, "unit": "us, the host's clock around one whole call", "calls_us": {k: stats(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_log_timing.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--general-reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ei-only", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds one section's child process may take")
    ap.add_argument("--section", default=None, help="(child) 'general' or a number of sets: measure it and print it")
    a = ap.parse_args()
    if a.section is not None:
        got = (measure_general(a.general_reps, min(a.warmup, 5), a.ei_only) if a.section == "general"
               else measure_sets(int(a.section), a.reps, a.warmup, a.ei_only))
        print("RESULT " + json.dumps(got), flush=True)
        return 0
    report = {"general": dict(GENERAL, d=3, reps=a.general_reps), "sets": dict(n=SET_N, m=SET_M, d=1, batch=SET_B, reps=a.reps),
              "warmup": a.warmup, "ei_only": a.ei_only, "sections": {}, "complete": False}
    ended = None
    for section in ["general"] + [str(s) for s in SETS]:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", section, "--reps", str(a.reps), "--general-reps",
               str(a.general_reps), "--warmup", str(a.warmup)] + (["--ei-only"] if a.ei_only else [])
        label = "general path" if section == "general" else f"{section} sets"
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            ended = f"{label}: no result within {a.step_timeout} s"
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            ended = f"{label}: exit status {r.returncode}: {r.stderr[-400:]}"
            break
        got = report["sections"][label] = json.loads(line[-1][len("RESULT "):])
        print(label, json.dumps({k: round(v["median"], 1) for k, v in got["calls_us"].items()}), flush=True)
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
