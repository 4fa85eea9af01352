"""Cost of leave-one-out cross-validation on the device (cbo_gp_loo, cbo_gp_loo_batch): device times between
cbo_region_begin and cbo_region_end and wall-clock times of the same calls, medians of 15 runs after 3 warm-ups.

General path, n = 4096 (d = 3, noise 1e-2), one child process per configuration (the knobs are read when the context is
created):
  auto            the route cbo_gp_loo picks: the whole identity fits the workspace, right-looking schedule
  one launch      CBO_HIP_LOO_ROUTE=1, default workspace: the identity in ONE left-looking launch (64 strips, full height)
  trailing x4     CBO_HIP_LOO_ROUTE=1, CBO_HIP_WORKSPACE_MB=33: four chunks of 1024 columns, trailing systems
  full height x4  CBO_HIP_LOO_ROUTE=2, CBO_HIP_WORKSPACE_MB=33: the same four chunks at full height
  host            cbo_gp_get_posterior (L over the link) + LAPACK dtrtri + column norms
Small path: 12 and 50 models of 50 rows (d = 1; complete graph with both priors, coral): one cbo_gp_loo_batch call against
cbo_gp_fit + cbo_gp_loo model by model.

Usage: python scripts/loo_timing.py [--out profiles/loo_timing.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RUNS, WARM = 15, 3
GENERAL = [("auto", {}), ("one launch", {"CBO_HIP_LOO_ROUTE": "1"}),
           ("trailing x4", {"CBO_HIP_LOO_ROUTE": "1", "CBO_HIP_WORKSPACE_MB": "33"}),
           ("full height x4", {"CBO_HIP_LOO_ROUTE": "2", "CBO_HIP_WORKSPACE_MB": "33"})]


def timed(ctx, call):
    dev, wall = [], []
    for r in range(WARM + RUNS):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.region_begin()
        call()
        ms = ctx.region_end()
        t1 = time.perf_counter()
        if r >= WARM:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    return dict(device_ms=statistics.median(dev), wall_ms=statistics.median(wall))


def general_problem(n=4096, d=3):
    rng = np.random.default_rng(0)
    X = rng.uniform(-5, 5, (n, d))
    y = np.cos(X[:, :1]) + 0.3 * np.sin(X[:, 1:2]) + 0.1 * rng.standard_normal((n, 1))
    return X, y


def child_general(host):
    from scipy.linalg import lapack
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X, y = general_problem()
    m = HipGaussianProcess(X, y, noise_var=1e-2)
    out = {}
    if host:
        def route():
            L, alpha = m.posterior_state()
            Li, info = lapack.dtrtri(L, lower=1)
            c = np.sum(Li * Li, axis=0)
            return y[:, 0] - alpha[:, 0] / c, 1.0 / c
        out = timed(m._ctx, route)
    else:
        out = timed(m._ctx, lambda: m._loo(True, True, True))
        out["sum_lpd"] = m.loo_score()
    print("RESULT " + json.dumps(out))


def child_small(n_models):
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    from cbo_with_oop_amd.utils_functions.model_check import loo_scores
    rng = np.random.default_rng(1)
    models = []
    for s in range(n_models):
        X = np.sort(rng.uniform(-5, 20, (50, 1)), axis=0)
        y = np.sin(X) + 0.1 * rng.standard_normal(X.shape)
        kw = dict(noise_var=1e-2, fit=False)
        if s % 2:
            kw.update(mean_function=lambda a: 0.5 * np.sin(a[:, :1]), variance_adjustment=lambda a: 0.2 + 0.0 * a[:, :1])
        models.append(HipGaussianProcess(X, y, **kw))
    ctx = models[0]._ctx

    def one_by_one():
        return [(m._fit(), m.loo_score())[1] for m in models]

    out = dict(batch=timed(ctx, lambda: loo_scores(models)), one_by_one=timed(ctx, one_by_one))
    a, b = loo_scores(models), one_by_one()
    out["max_abs_difference_of_sums"] = float(np.max(np.abs(np.array(a) - np.array(b))))
    print("RESULT " + json.dumps(out))


def run_child(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} {env_extra} ended with {p.returncode}: stopping")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_timing.json"))
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "general":
            child_general(host=a.child[1] == "host")
        else:
            child_small(int(a.child[1]))
        return
    res = {"runs": RUNS, "warmups": WARM, "general_n4096": {}, "small_50_rows": {}}
    for name, env in GENERAL:
        res["general_n4096"][name] = dict(run_child(["--child", "general", "device"], env, 240), env=env)
        print(name, res["general_n4096"][name], flush=True)
    res["general_n4096"]["host"] = run_child(["--child", "general", "host"], {}, 400)
    print("host", res["general_n4096"]["host"], flush=True)
    for k in (12, 50):
        res["small_50_rows"][f"{k} models"] = run_child(["--child", "small", str(k)], {}, 240)
        print(k, res["small_50_rows"][f"{k} models"], flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
