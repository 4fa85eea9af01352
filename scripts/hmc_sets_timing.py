"""Timing of the one-launch HMC sampler (cbo_gp_hmc_sets, kernels_hmc.hip) on one MI355X, at the reference's
scale -- 2, 6 and 25 models of 50 observations, d = 1 and d = 3 (ARD) -- for two chains: emukit's defaults (100 burn-in + 10
samples at interval 10 = 200 samples of 20 leapfrog steps: 4001 likelihood evaluations per model) and a short one (10
burn-in + 5 samples at interval 2 = 20 samples of 5 steps: 101 evaluations), beside what it replaces, on the same box:

  (a) generate_hyperparameters_samples_together(models): optimize_together, the draws, ONE cbo_gp_hmc_sets call;
  (b) [m.generate_hyperparameters_samples() for m in models]: per model optimize(), the draws, and the host chain -- one
      cbo_gp_set_hyper plus one polled cbo_gp_lml_gradients launch per position.

Both start every repetition from the same hyper-parameters and the same seed (twin model lists, reset outside the clock), the
variants ALTERNATE, and the median, min and max per variant are reported in milliseconds.  The call itself is timed through
hmc_chains_device as well (fixed starts and draws, no optimiser): its time over 1 + num_samples * hmc_iters is the launch's
time per likelihood evaluation, reported beside the median of one cbo_gp_lml_gradients call on one of the models.
Every (d, models, chain) shape is measured by a fresh child process under its own time limit, one at a time; the first
child that fails or runs out of time ends the run (nothing more is started on the GPU) and the report says so.

    python scripts/hmc_sets_timing.py --out profiles/hmc_sets_timing.json
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

MODELS = [2, 6, 25]
DIMS = [1, 3]
N = 50
CHAINS = {"default": dict(n_samples=10, n_burnin=100, subsample_interval=10, step_size=1e-1, leapfrog_steps=20),
          "short": dict(n_samples=5, n_burnin=10, subsample_interval=2, step_size=1e-1, leapfrog_steps=5)}
A, B_ = "(a) one call (generate_hyperparameters_samples_together)", "(b) per model (generate_hyperparameters_samples)"


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def measure(d, s, chain, reps):
    """One shape, in this process."""
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import (HipGaussianProcess, generate_hyperparameters_samples_together,
                                                         hmc_chains_device)
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
    kw = CHAINS[chain]
    num = kw["n_burnin"] + kw["n_samples"] * kw["subsample_interval"]
    rng = np.random.default_rng(100 * d + s)
    ard = d > 1
    ls0 = np.linspace(0.8, 1.2, d) if ard else 1.0

    def build():
        out = []
        for _ in range(s):
            X = rng.uniform(-2.0, 2.0, (N, d))
            y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
            out.append((X, y))
        return out
    data = build()
    lists = {k: [HipGaussianProcess(X, y, ard=ard, lengthscale=ls0, noise_var=1e-2, fit=False) for X, y in data] for k in (A, B_)}

    def reset(models, seed):
        for m in models:
            m.set_hyperparameters(1.0, ls0, 1e-2, fit=False)
        np.random.seed(seed)

    variants = {A: lambda: generate_hyperparameters_samples_together(lists[A], **kw),
                B_: lambda: [m.generate_hyperparameters_samples(**kw) for m in lists[B_]]}
    times = {k: [] for k in variants}
    order = list(variants)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        reset(lists[A], 0)
        variants[A]()                                                 # (one unrecorded call: buffers, the kernel's first load)
        for r in range(reps):
            for k in order[r % 2:] + order[:r % 2]:
                reset(lists[k], 1 + r)
                t0 = time.perf_counter_ns()
                variants[k]()
                times[k].append((time.perf_counter_ns() - t0) * 1e-6)
        # the call on its own: fixed starts and draws
        P = 2 + (d if ard else 1)
        theta0s = [np.concatenate([[1.0], np.atleast_1d(ls0) * np.ones(P - 2), [1e-2]]) for _ in range(s)]
        np.random.seed(5)
        draws = [hmc_draws(P, num) for _ in range(s)]
        call = []
        for _ in range(1 + max(reps, 5)):
            t0 = time.perf_counter_ns()
            outs = hmc_chains_device(lists[A], theta0s, draws, kw["leapfrog_steps"], kw["step_size"])
            call.append((time.perf_counter_ns() - t0) * 1e-6)
        assert all(o["status"] == _lib.HMC_OK for o in outs)
        accepted = float(np.mean([o["accept"].mean() for o in outs]))
        one = []
        m = lists[B_][0]
        for _ in range(220):
            t0 = time.perf_counter_ns()
            m.log_likelihood_gradients()
            one.append((time.perf_counter_ns() - t0) * 1e-3)
    evals = 1 + num * kw["leapfrog_steps"]
    name = _lib.Context.get().name()
    for lst in lists.values():
        for m in lst:
            m.close()
    return {"device": name, "calls_ms": {k: stats(t) for k, t in times.items()}, "hmc_sets_call_ms": stats(call[1:]),
            "evaluations_per_model": evals, "launch_us_per_evaluation": 1e3 * float(np.median(call[1:])) / evals,
            "one_lml_gradients_call_us": stats(one[20:]), "accept_rate": accepted}


def write(report, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_sets_timing.json"))
    ap.add_argument("--reps", type=int, default=5, help="alternating rounds per shape (3 at 25 models)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds one shape's child process may take")
    ap.add_argument("--shape", nargs=3, default=None, help="(child) measure this (d, models, chain) and print it")
    a = ap.parse_args()
    if a.shape is not None:
        print("RESULT " + json.dumps(measure(int(a.shape[0]), int(a.shape[1]), a.shape[2], a.reps)), flush=True)
        return 0
    report = {"n": N, "chains": CHAINS,
              "clock": "time.perf_counter_ns around one whole call, variants alternating with a rotating start, same seed and "
                       "start per round; one child process per shape",
              "shapes": {}, "complete": False}
    ended = None
    for chain in CHAINS:
        for d in DIMS:
            for s in MODELS:
                key = f"{chain} chain, d = {d}, {s} models"
                reps = min(a.reps, 3) if s >= 25 else a.reps
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(d), str(s), chain, "--reps", str(reps)]
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
                write(report, a.out)                                  # (what is measured so far survives an early end)
                print(key, json.dumps({k: round(t["median"], 2) for k, t in got["calls_ms"].items()}),
                      "call alone", round(got["hmc_sets_call_ms"]["median"], 2), "ms,",
                      round(got["launch_us_per_evaluation"], 2), "us / evaluation; one lml call",
                      round(got["one_lml_gradients_call_us"]["median"], 1), "us", flush=True)
            if ended:
                break
        if ended:
            break
    report["complete"] = ended is None
    if ended:
        report["ended"] = ended
        print("ended:", ended, flush=True)
    else:
        report["one_call_below_per_model_at_6_and_25_models"] = all(
            r["calls_ms"][A]["median"] < r["calls_ms"][B_]["median"]
            for k, r in report["shapes"].items() if not k.endswith(", 2 models"))
    write(report, a.out)
    print(json.dumps({k: v for k, v in report.items() if k != "shapes"}, indent=1))
    return 0 if ended is None else 1


if __name__ == "__main__":
    sys.exit(main())
