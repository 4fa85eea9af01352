"""Timing of the one-launch hyper-parameter MLE for models of 129..256 observations (cbo_gp_mle_sets_rows with max_rows = 256,
kernels_mle_mid.hip) on one MI355X, beside what it replaces, on the same box and from the same starts:

  (a) optimize_together(models, optimizer="device", device_rows=256): ONE cbo_gp_mle_sets_rows call, every search inside it;
  (b) optimize_together(models): scipy's L-BFGS-B runs in lockstep, one cbo_gp_lml_gradients_batch launch per round;
  (c) [m.optimize() for m in models]: scipy's L-BFGS-B per model, a refit and the general likelihood path per evaluation.

Shapes (noise fixed at 1e-2 throughout, as for every graph-level GP): the complete graph's ten graph GPs (d = 1, 1, 2, 2, 3,
3, 4, 4, 5, 6, ARD off) at 140, 200 and 256 rows; the coral graph's fifteen (d = 1..8, four of them ARD) at 200 rows; and (a)
with 8 starts per model at ten models of 200 rows, the restarts drawn from the same seed.
Every repetition starts from the same hyper-parameters (reset outside the clock), the variants ALTERNATE, and the median,
min and max per variant are reported in milliseconds -- whole Python calls.  Per variant the report also holds what the
search did (rounds / evaluations, final lml per model) and the final lml of (b) minus (a) per model.  The call itself is
timed through mle_runs_device as well: its time over the largest 1 + rounds of its runs is the launch's time per likelihood
evaluation of its longest run; beside it, one cbo_gp_lml_gradients_batch call on one such model.
Every shape is measured by a fresh child process under its own time limit, one at a time; the first child that fails or
runs out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/mle_mid_timing.py --out profiles/mle_mid_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A, B_, C_ = "(a) one launch (optimizer='device', device_rows=256)", "(b) lockstep (optimize_together)", "(c) per model (optimize)"
COMPLETE = [(d, False) for d in (1, 1, 2, 2, 3, 3, 4, 4, 5, 6)]
CORAL = [(1, False), (5, True), (4, True), (2, True), (2, True), (6, False), (3, False), (3, False), (8, False), (6, False),
         (3, False), (6, False), (7, False), (4, False), (7, False)]
SHAPES = ([(f"10 graph GPs of {n} rows", dict(models=COMPLETE, n=n)) for n in (140, 200, 256)]
          + [("15 coral graph GPs of 200 rows", dict(models=CORAL, n=200)),
             ("10 graph GPs of 200 rows, 8 starts", dict(models=COMPLETE, n=200, restarts=8))])


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def measure(spec, reps):
    """One shape, in this process."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import (HipGaussianProcess, _optimizer_start, lml_gradients_batch,
                                                         mle_runs_device, optimize_together)
    n, restarts = spec["n"], spec.get("restarts")
    rng = np.random.default_rng(1000 + n + len(spec["models"]))
    data = []
    for d, ard in spec["models"]:
        X = rng.uniform(-2.0, 2.0, (n, d))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
        data.append((X, y, ard, np.ones(d) if ard else 1.0))

    def build():
        return [HipGaussianProcess(X, y, ard=ard, lengthscale=ls0, noise_var=1e-2, fix_noise=True, fit=False)
                for X, y, ard, ls0 in data]

    def reset(models, seed):
        for m, (_, _, _, ls0) in zip(models, data):
            m.set_hyperparameters(1.0, ls0, 1e-2, fit=False)
        np.random.seed(seed)

    if restarts is None:
        names = [A, B_, C_]
        variants = {A: lambda ms: optimize_together(ms, optimizer="device", device_rows=256, host_fallback=False),
                    B_: lambda ms: optimize_together(ms), C_: lambda ms: [m.optimize() for m in ms]}
    else:
        names = [A]
        variants = {A: lambda ms: optimize_together(ms, optimizer="device", device_rows=256, num_restarts=restarts,
                                                    host_fallback=False)}
    lists = {k: build() for k in names}
    times = {k: [] for k in names}
    did = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for k in names:                                               # (one unrecorded call each: buffers, first loads)
            reset(lists[k], 0)
            variants[k](lists[k])
        for r in range(reps):
            for k in names[r % len(names):] + names[:r % len(names)]:
                reset(lists[k], 1 + r)
                t0 = time.perf_counter_ns()
                results = variants[k](lists[k])
                times[k].append((time.perf_counter_ns() - t0) * 1e-6)
                did[k] = {"final_lml": [-float(res.fun) for res in results], "rounds": [int(res.nit) for res in results],
                          "evaluations": [int(res.nfev) for res in results],
                          "status": [str(res.message if isinstance(res.message, str) else res.message.decode()) for res in results]}
                if k == A:
                    did[k]["best_run"] = [res.best_run for res in results]
        # the call on its own: fixed starts, no Python around it but the wrapper's
        reset(lists[A], 0)
        theta0s = [_optimizer_start(m, "logexp")[0] for m in lists[A]]
        call = []
        for _ in range(1 + max(reps, 5)):
            t0 = time.perf_counter_ns()
            outs = mle_runs_device(lists[A], theta0s, 1000, device_rows=256)
            call.append((time.perf_counter_ns() - t0) * 1e-6)
        longest = max(1 + int(o["rounds"].max()) for o in outs)
        one = []
        for _ in range(120):
            t0 = time.perf_counter_ns()
            lml_gradients_batch(lists[A][-1:])
            one.append((time.perf_counter_ns() - t0) * 1e-3)
    name = _lib.Context.get().name()
    for lst in lists.values():
        for m in lst:
            m.close()
    out = {"device": name, "calls_ms": {k: stats(t) for k, t in times.items()}, "searches": did,
           "mle_sets_rows_call_ms": stats(call[1:]), "longest_run_evaluations": longest,
           "launch_us_per_evaluation_of_the_longest_run": 1e3 * float(np.median(call[1:])) / longest,
           "one_lml_gradients_batch_call_on_one_model_us": stats(one[20:])}
    if B_ in did:
        out["final_lml_lockstep_minus_device"] = [b - a for a, b in zip(did[A]["final_lml"], did[B_]["final_lml"])]
    return out


def write(report, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_mid_timing.json"))
    ap.add_argument("--reps", type=int, default=5, help="alternating rounds per shape")
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(child) measure SHAPES[i] and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(SHAPES[a.shape][1], a.reps)), flush=True)
        return 0
    report = {"clock": "time.perf_counter_ns around one whole Python call, variants alternating with a rotating start, same "
                       "start per round; one child process per shape",
              "shapes": {}, "complete": False}
    ended = None
    for i, (key, spec) in enumerate(SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(i), "--reps", str(a.reps)]
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
        report["device"] = got.pop("device")
        report["shapes"][key] = got
        write(report, a.out)                                          # (what is measured so far survives an early end)
        print(key, json.dumps({k: round(t["median"], 3) for k, t in got["calls_ms"].items()}), "call alone",
              round(got["mle_sets_rows_call_ms"]["median"], 3), "ms,", round(got["launch_us_per_evaluation_of_the_longest_run"], 1),
              "us / evaluation of the longest run (", got["longest_run_evaluations"], "); one batch likelihood call",
              round(got["one_lml_gradients_batch_call_on_one_model_us"]["median"], 1), "us", flush=True)
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    else:
        r = report["shapes"]["10 graph GPs of 200 rows"]["calls_ms"]
        report["one_launch_below_lockstep_at_10_models_of_200_rows"] = r[A]["median"] < r[B_]["median"]
    write(report, a.out)
    print(json.dumps({k: v for k, v in report.items() if k != "shapes"}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
