"""Timing of greedy batch selection in the one-launch multi-set sweep (cbo_acq_sweep_sets_batch, kernels_sets_batch.hip) on
one MI355X, at BASELINE config 1's shape -- 50 observations and 200 candidates per exploration set, d = 1 -- for 2, 6 and 25
sets and batches of 1, 4 and 8, beside what it replaces and beside its floor, on the same box and the same models:

  (a) cbo_acq_sweep_sets_batch: one call for all sets;
  (b) the per-set sequence the call replaces: cbo_gp_fit + cbo_acq_sweep_batch, set by set;
  (c) cbo_acq_sweep_sets (the causal EI, one pick per set): the floor for a batch of one.

Every figure is the host's clock around one whole call (each call ends with its results on the host): --warmup unrecorded
calls per variant, then the variants ALTERNATE for --reps rounds (the round's first variant rotating, so that every variant
follows every other equally often), and the median, quartiles, min and max per variant are reported in microseconds.
Every (sets, batch) shape is measured by a fresh child process under its own time limit; the first child that fails or runs
out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/sets_batch_timing.py --out profiles/sets_batch_timing.json
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

SETS = [2, 6, 25]
BATCHES = [1, 4, 8]
N, M, D = 50, 200, 1
A, B_, C = ("(a) one call (cbo_acq_sweep_sets_batch)", "(b) per set (cbo_gp_fit + cbo_acq_sweep_batch)",
            "(c) EI one launch (cbo_acq_sweep_sets)")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "p25": float(np.percentile(v, 25)), "p75": float(np.percentile(v, 75)), "count": int(v.size)}


def measure(s, batch, reps, warmup):
    """One shape, in this process: {variant: stats} and the device's name."""
    from cbo_with_oop_amd import CandidateGrid, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    lib = _lib.load()
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
    vals, idxs = np.empty(s * batch), np.empty(s * batch, dtype=np.int64)
    yb, cs, vp, ip = _lib.dptr(y_best), _lib.dptr(costs), _lib.dptr(vals), idxs.ctypes.data_as(_lib.c_int64_p)
    one_v, one_i = np.empty(batch), np.empty(batch, dtype=np.int64)
    ovp, oip = _lib.dptr(one_v), one_i.ctypes.data_as(_lib.c_int64_p)

    def one_call():
        _lib.check(lib.cbo_acq_sweep_sets_batch(s, gps, cds, yb, 0, 0.0, cs, batch, 0, vp, ip))

    def per_set():
        for m, g in zip(models, grids):
            _lib.check(lib.cbo_gp_fit(m._handle, None, None))
            _lib.check(lib.cbo_acq_sweep_batch(m._handle, g._handle, y_best[0], 0, 0.0, 1.0, batch, 0, ovp, oip, None, None, None))

    def sets_ei():
        _lib.check(lib.cbo_acq_sweep_sets(s, gps, cds, yb, 0, 0.0, cs, vp, ip))

    variants = {A: one_call, B_: per_set, C: sets_ei}
    for call in variants.values():
        for _ in range(warmup):
            call()
    times = {k: [] for k in variants}
    names = list(variants)
    for r in range(reps):
        # (the round's first variant rotates: a call's time depends a little on what ran before it -- the call behind the
        # per-set sequence finds the caches and the stream as 2-25 fits left them)
        for k in names[r % len(names):] + names[:r % len(names)]:
            t0 = time.perf_counter_ns()
            variants[k]()
            times[k].append((time.perf_counter_ns() - t0) * 1e-3)
    name = _lib.Context.get().name()
    for o in grids + models:
        o.close()
    return {"device": name, "calls_us": {k: stats(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_batch_timing.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", type=int, nargs=2, default=None, help="(child) measure this (sets, batch) and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(a.shape[0], a.shape[1], a.reps, a.warmup)), flush=True)
        return 0
    report = {"n": N, "m": M, "d": D, "warmup": a.warmup, "reps": a.reps,
              "clock": "time.perf_counter_ns around one whole call, variants alternating with a rotating start; one child process per shape",
              "calls_us": {}, "complete": False}
    ended = None
    for s in SETS:
        for batch in BATCHES:
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(s), str(batch), "--reps", str(a.reps),
                   "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                ended = f"{s} sets, B = {batch}: no result within {a.step_timeout} s"
                break
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                ended = f"{s} sets, B = {batch}: exit status {r.returncode}: {r.stderr[-400:]}"
                break
            got = json.loads(line[-1][len("RESULT "):])
            report["device"] = got["device"]
            row = report["calls_us"][f"{s} sets, B = {batch}"] = got["calls_us"]
            print(f"{s} sets, B = {batch}", json.dumps({k: round(v["median"], 1) for k, v in row.items()}), flush=True)
        if ended:
            break
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    else:
        rows = report["calls_us"]
        report["a_below_b_everywhere"] = all(r[A]["median"] < r[B_]["median"] for r in rows.values())
        # (a) at B = 1 against (c): equal when the median of one lies inside the other's interquartile range
        report["a_equals_c_at_batch_1"] = all(r[C]["p25"] <= r[A]["median"] <= r[C]["p75"] or
                                              r[A]["p25"] <= r[C]["median"] <= r[A]["p75"]
                                              for k, r in rows.items() if k.endswith("B = 1"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k != "calls_us"}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
