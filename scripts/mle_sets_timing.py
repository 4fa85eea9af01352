"""Timing of the one-launch hyper-parameter MLE (cbo_gp_mle_sets, kernels_mle.hip) on one MI355X, beside
what it replaces, on the same box and from the same starts:

  (a) optimize_together(models, optimizer="device"): ONE cbo_gp_mle_sets call, every model's whole search inside it;
  (b) optimize_together(models): scipy's L-BFGS-B runs in lockstep, one cbo_gp_lml_gradients_batch launch per round;
  (c) [m.optimize() for m in models]: scipy's L-BFGS-B per model, one cbo_gp_lml_gradients launch per evaluation.

Shapes: group 1 -- 2, 6 and 25 models of 50 observations, d = 1 and d = 3 (ARD), noise fitted; group 2 -- 10 graph-GP-shaped
models of 100 rows (d = 1..3, ARD off, noise fixed at 1e-2: the complete graph's observe step); group 3 -- (a) with 1 and
with 8 starts per model (6 models of 50 observations, d = 3), the restarts drawn from the same seed.
Every repetition starts from the same hyper-parameters (twin model lists, reset outside the clock), the variants ALTERNATE,
and the median, min and max per variant are reported in milliseconds -- whole Python calls.  Per variant the report also
holds what the search did: rounds (device) or iterations / evaluations (scipy) and the final lml per model, so the reader
sees whether the device search ends as high as scipy's.  The call itself is timed through mle_runs_device as well: its time
over the largest 1 + rounds of its runs is the launch's time per likelihood evaluation of its longest run.
Every shape is measured by a fresh child process under its own time limit, one at a time; the first child that fails or
runs out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/mle_sets_timing.py --out profiles/mle_sets_timing.json
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

A, B_, C_ = "(a) one launch (optimizer='device')", "(b) lockstep (optimize_together)", "(c) per model (optimize)"
SHAPES = ([("group 1", f"d = {d}, {s} models of 50", dict(kind="plain", d=d, s=s, n=50)) for d in (1, 3) for s in (2, 6, 25)]
          + [("group 2", "10 graph GPs of 100 rows, fixed noise", dict(kind="graph", d=0, s=10, n=100))]
          + [("group 3", f"d = 3, 6 models of 50, {r} start(s)", dict(kind="plain", d=3, s=6, n=50, restarts=r)) for r in (1, 8)])


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def measure(spec, reps):
    """One shape, in this process."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import (HipGaussianProcess, _optimizer_start, mle_runs_device,
                                                         optimize_together)
    kind, s, n, restarts = spec["kind"], spec["s"], spec["n"], spec.get("restarts")
    rng = np.random.default_rng(1000 * spec["d"] + s)
    data = []
    for j in range(s):
        d = spec["d"] if kind == "plain" else 1 + j % 3
        X = rng.uniform(-2.0, 2.0, (n, d))
        y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
        ard = kind == "plain" and d > 1
        data.append((X, y, ard, np.linspace(0.8, 1.2, d) if ard else 1.0))

    def build():
        return [HipGaussianProcess(X, y, ard=ard, lengthscale=ls0, noise_var=1e-2, fix_noise=kind == "graph", fit=False)
                for X, y, ard, ls0 in data]

    def reset(models, seed):
        for m, (_, _, _, ls0) in zip(models, data):
            m.set_hyperparameters(1.0, ls0, 1e-2, fit=False)
        np.random.seed(seed)

    if restarts is None:
        names = [A, B_, C_]
        variants = {A: lambda ms: optimize_together(ms, optimizer="device"), B_: lambda ms: optimize_together(ms),
                    C_: lambda ms: [m.optimize() for m in ms]}
    else:
        names = [A]
        variants = {A: lambda ms: optimize_together(ms, optimizer="device", num_restarts=restarts)}
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
            outs = mle_runs_device(lists[A], theta0s, 1000)
            call.append((time.perf_counter_ns() - t0) * 1e-6)
        longest = max(1 + int(o["rounds"].max()) for o in outs)
        one = []
        for _ in range(220):
            t0 = time.perf_counter_ns()
            lists[A][0].log_likelihood_gradients()
            one.append((time.perf_counter_ns() - t0) * 1e-3)
    name = _lib.Context.get().name()
    for lst in lists.values():
        for m in lst:
            m.close()
    return {"device": name, "calls_ms": {k: stats(t) for k, t in times.items()}, "searches": did,
            "mle_sets_call_ms": stats(call[1:]), "longest_run_evaluations": longest,
            "launch_us_per_evaluation_of_the_longest_run": 1e3 * float(np.median(call[1:])) / longest,
            "one_lml_gradients_call_us": stats(one[20:])}


def write(report, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_sets_timing.json"))
    ap.add_argument("--reps", type=int, default=5, help="alternating rounds per shape (3 at 25 models)")
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(child) measure SHAPES[i] and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(SHAPES[a.shape][2], a.reps)), flush=True)
        return 0
    report = {"clock": "time.perf_counter_ns around one whole Python call, variants alternating with a rotating start, same "
                       "start per round; one child process per shape",
              "shapes": {}, "complete": False}
    ended = None
    for i, (group, label, spec) in enumerate(SHAPES):
        key = f"{group}: {label}"
        reps = min(a.reps, 3) if spec["s"] >= 25 else a.reps
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(i), "--reps", str(reps)]
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
              round(got["mle_sets_call_ms"]["median"], 3), "ms,", round(got["launch_us_per_evaluation_of_the_longest_run"], 1),
              "us / evaluation of the longest run (", got["longest_run_evaluations"], "); one lml call",
              round(got["one_lml_gradients_call_us"]["median"], 1), "us", flush=True)
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    else:
        report["one_launch_below_lockstep_at_6_and_25_models"] = all(
            r["calls_ms"][A]["median"] < r["calls_ms"][B_]["median"]
            for k, r in report["shapes"].items() if k.startswith("group 1") and ", 2 models" not in k)
    write(report, a.out)
    print(json.dumps({k: v for k, v in report.items() if k != "shapes"}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
