"""Timing of the hyper-parameter priors' stage (csrc/hyper_prior.h) on one MI355X: whole cbo_gp_hmc_sets and
cbo_gp_mle_sets calls (through hmc_chains_device / mle_runs_device, fixed starts and draws) at the reference's scale -- 2, 6
and 25 models of 50 observations, d = 1 and d = 3 (ARD) -- without priors and with a Gamma prior on every parameter.  The
chain is 20 samples of 5 leapfrog steps (101 likelihood evaluations per model), the search at most 40 rounds.

Within a process the two variants ALTERNATE (twin model lists, one with priors), medians of whole Python calls in
milliseconds (time.perf_counter_ns).  ``--parent-lib PATH`` names a libcbo_hip.so built from the parent commit: the no-prior
calls are then also measured against that library -- a child process per (library, round) that runs the no-prior variant
ALONE, this tree's library and the parent's alike (the same sequence of calls in both, so the comparison is of the libraries
and of nothing else), the two alternating round by round on the same box in the same session -- and the report states whether
the no-prior calls of this tree stay within 5 % of the parent's (the box-to-box spread README.md reports; more would hide a
regression in the untouched path).  The parent library knows nothing of priors: a no-prior child unbinds the three new
symbols before loading.  The first child that fails or runs out of time ends the run: nothing more is started on the GPU.

    python scripts/hyper_prior_timing.py --out profiles/hyper_prior_timing.json [--parent-lib /path/to/parent/libcbo_hip.so]
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
NUM, ITERS, STEP, ROUNDS = 20, 5, 0.05, 40
NEW_SYMBOLS = ("cbo_gp_set_priors", "cbo_gp_get_priors", "cbo_gp_log_prior_batch")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def measure(reps, with_priors):
    """Every shape in this process: {shape: {call: {variant: [ms, ...]}}}."""
    from cbo_with_oop_amd import _lib
    if not with_priors:                                  # a library from before the priors: bind what it has
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess, hmc_chains_device, mle_runs_device
    from cbo_with_oop_amd.utils_functions.integrated_hyper import hmc_draws
    from cbo_with_oop_amd.utils_functions.priors import Gamma
    out = {}
    for d in DIMS:
        for s in MODELS:
            rng = np.random.default_rng(100 * d + s)
            ard = d > 1
            ls0 = np.linspace(0.8, 1.2, d) if ard else np.array([1.0])
            data = []
            for _ in range(s):
                X = rng.uniform(-2.0, 2.0, (N, d))
                data.append((X, np.sin(X[:, :1]) + 0.2 * X[:, -1:] + 0.05 * rng.standard_normal((N, 1))))

            def build(priors):
                models = []
                for X, y in data:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", RuntimeWarning)
                        m = HipGaussianProcess(X, y, ard=ard, variance=1.0, lengthscale=ls0 if ard else 1.0, noise_var=0.05, fit=False)
                    if priors:
                        for name in ("variance", "lengthscale", "noise_var"):
                            m.set_prior(name, Gamma.from_EV(1.0, 10.0))
                    models.append(m)
                return models
            variants = {"no priors": build(False)}
            if with_priors:
                variants["priors"] = build(True)
            theta0 = np.concatenate([[1.0], ls0, [0.05]])
            np.random.seed(7)
            draws = [hmc_draws(theta0.size, NUM) for _ in range(s)]
            calls = {
                "cbo_gp_hmc_sets": lambda models: hmc_chains_device(models, [theta0] * s, draws, ITERS, STEP),
                "cbo_gp_mle_sets": lambda models: mle_runs_device(models, [theta0] * s, ROUNDS),
            }
            shape = {}
            for call, fn in calls.items():
                times = {v: [] for v in variants}
                for r in range(3 + reps):
                    for v, models in variants.items():
                        t0 = time.perf_counter_ns()
                        ans = fn(models)
                        t1 = time.perf_counter_ns()
                        if r >= 3:
                            times[v].append((t1 - t0) * 1e-6)
                        if call == "cbo_gp_hmc_sets":
                            assert all(a["status"] == _lib.HMC_OK for a in ans)
                        else:
                            assert not any(a["declined"] for a in ans) and all(np.isfinite(a["lml"][0]) for a in ans)
                shape[call] = times
            out[f"d = {d}, {s} models of {N}"] = shape
            for models in variants.values():
                for m in models:
                    m.close()
    name = _lib.Context.get().name()
    return {"device": name, "shapes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyper_prior_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per library")
    ap.add_argument("--child", choices=["head", "plain", "parent"], default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per child process")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps, with_priors=args.child == "head")))
        return 0
    libs = [("head", None)] + ([("plain", None), ("parent", args.parent_lib)] if args.parent_lib else [])
    merged, device, complete = {}, None, True
    for rnd in range(args.rounds):
        for label, lib in (libs if rnd % 2 == 0 else libs[::-1]):           # the libraries alternate, the start rotates
            env = dict(os.environ)
            if lib:
                env["CBO_HIP_LIB"] = os.path.abspath(lib)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label, "--reps", str(args.reps)],
                                   env=env, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                r = None
            if r is None or r.returncode != 0:
                print(f"child {label} round {rnd}: " + ("time limit" if r is None else f"exit {r.returncode}\n{r.stderr[-2000:]}"),
                      file=sys.stderr)
                complete = False
                break
            got = json.loads(r.stdout.strip().splitlines()[-1])
            device = got["device"]
            for shape, calls in got["shapes"].items():
                for call, times in calls.items():
                    for variant, ms in times.items():
                        key = {"head": variant, "plain": "no priors, alone", "parent": "no priors, alone, parent library"}[label]
                        merged.setdefault(shape, {}).setdefault(call, {}).setdefault(key, []).extend(ms)
        if not complete:
            break
    report = {"clock": "time.perf_counter_ns around one whole Python call (hmc_chains_device: 20 samples x 5 leapfrog steps; "
                       "mle_runs_device: at most 40 rounds); variants alternating inside a process, libraries alternating "
                       "process by process; medians over every process's calls, milliseconds",
              "device": device, "complete": complete, "shapes": {}}
    worst = 0.0
    for shape, calls in merged.items():
        report["shapes"][shape] = {}
        for call, times in calls.items():
            entry = {k: stats(v) for k, v in times.items()}
            if "priors" in entry:
                entry["priors_over_no_priors"] = entry["priors"]["median"] / entry["no priors"]["median"]
            if "no priors, alone, parent library" in entry:
                entry["no_priors_over_parent"] = (entry["no priors, alone"]["median"]
                                                  / entry["no priors, alone, parent library"]["median"])
                worst = max(worst, entry["no_priors_over_parent"])
            report["shapes"][shape][call] = entry
    if args.parent_lib:
        report["worst_no_priors_over_parent"] = worst
        report["no_prior_calls_within_5_percent_of_the_parent"] = bool(complete and worst <= 1.05)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k != "shapes"}))
    for shape, calls in report["shapes"].items():
        for call, e in calls.items():
            print(shape, call, {k: (round(v["median"], 4) if isinstance(v, dict) else round(v, 4)) for k, v in e.items()})
    return 0 if complete else 1


if __name__ == "__main__":
    sys.exit(main())
