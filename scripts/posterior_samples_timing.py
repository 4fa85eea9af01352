"""Timing of the joint posterior samples (cbo_gp_posterior_samples: solve, cov_tile_kernel, factorisation,
samples_tile_kernel of kernels_joint.hip) on one MI355X, at (n, m, s) = (50, 200, 100) (reference scale),
(1024, 4096, 1024), (4096, 4096, 4096) and (4096, 8192, 1024).

Two runs make one report:

    python scripts/posterior_samples_timing.py --calls-only                 # under rocprofv3 --kernel-trace --stats
    python scripts/posterior_samples_timing.py --trace <dir of that run> --out profiles/posterior_samples_timing.json

The first form only makes the calls (two warm-ups, then --reps timed ones per size) for
`rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python ...`.  The second times the whole calls
with the profiler off (host clock around calls that end in a stream synchronise; the normals are drawn beforehand) and
takes from the trace, per timed call, the time of each kernel group: the normals' transpose, the solve (K*, L^-1 K*,
the mean), the padding of the factor buffer, cov_tile_kernel, the factorisation (the sum of its kernels' durations: its
look-ahead stream overlaps some of them) and samples_tile_kernel.  Share of peak: m^2 s flop (the triangle-aware
product) over the product kernel's time and the 78.6 TFLOP/s fp64 MFMA peak.  A host baseline,
np.random.multivariate_normal on the device's Sigma, is timed at (1024, 4096, 1024).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(50, 200, 100), (1024, 4096, 1024), (4096, 4096, 4096), (4096, 8192, 1024)]
HOST_BASELINE = (1024, 4096, 1024)
PEAK_F64 = 78.6e12
GROUPS = ("transpose", "solve", "padding", "cov", "factor", "product")


def problem(n, m, s, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return X, y, rng.uniform(-2.0, 2.0, (m, d)), rng.standard_normal((s, m))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def run_calls(reps):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    out, jitter = {}, {}
    for n, m, s in SIZES:
        X, y, Xs, Z = problem(n, m, s)
        g = HipGaussianProcess(X, y, noise_var=1e-2)
        g.posterior_samples_f(Xs, s, normals=Z)      # warm-up: code objects, workspaces, buffers
        g.posterior_samples_f(Xs, s, normals=Z)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.posterior_samples_f(Xs, s, normals=Z)
            t.append((time.perf_counter() - t0) * 1e3)
        out[(n, m, s)] = t
        jitter[(n, m, s)] = g.last_sample_jitter
        g.close()
    return out, jitter


def host_baseline(reps=3):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    n, m, s = HOST_BASELINE
    X, y, Xs, _ = problem(n, m, s)
    g = HipGaussianProcess(X, y, noise_var=1e-2)
    mean, cov = g.predict(Xs, include_likelihood=False, full_cov=True)
    g.close()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        np.random.multivariate_normal(mean[:, 0], cov, s)
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def read_trace(trace_dir, reps):
    """Per size the kernel-group times (ms) of the timed calls.  A call's kernels run in order: transpose, solve,
    then per ladder attempt padding, cov and the factorisation, and samples_tile_kernel closes the call."""
    kfile = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not kfile:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(kfile[0]) as f:
        kern = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    calls, cur, phase = [], defaultdict(float), "solve"
    for t0, t1, name in kern:
        dt = (t1 - t0) * 1e-6
        if "normals_transpose_kernel" in name:
            cur["transpose"] += dt
        elif "factor_padding_kernel" in name:
            phase = "factor"
            cur["padding"] += dt
        elif "cov_tile_kernel" in name:
            cur["cov"] += dt
        elif "samples_tile_kernel" in name:
            cur["product"] += dt
            calls.append(cur)
            cur, phase = defaultdict(float), "solve"
        else:
            cur[phase] += dt
    per_size = 2 + reps
    if len(calls) != per_size * len(SIZES):
        raise SystemExit(f"expected {per_size * len(SIZES)} samples_tile_kernel launches in the trace, found {len(calls)}")
    return {size: calls[i * per_size + 2:(i + 1) * per_size] for i, size in enumerate(SIZES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls-only", action="store_true", help="only make the calls (run under rocprofv3)")
    ap.add_argument("--trace", help="directory of the rocprofv3 run of --calls-only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_samples_timing.json"))
    a = ap.parse_args()
    if a.calls_only:
        run_calls(a.reps)
        return
    if not a.trace:
        raise SystemExit("--trace <dir> (the rocprofv3 run of --calls-only) is needed for the kernel times")
    from cbo_with_oop_amd import _lib
    wall, jitter = run_calls(a.reps)
    device = _lib.Context.get().name()
    traced = read_trace(a.trace, a.reps)
    rows = []
    for n, m, s in SIZES:
        calls = traced[(n, m, s)]
        flop = float(m) * m * s
        kernels = {k: stats([c.get(k, 0.0) for c in calls]) for k in GROUPS}
        prod = np.asarray([c["product"] for c in calls])
        row = {
            "n": n, "m": m, "s": s,
            "whole_call_ms": stats(wall[(n, m, s)]),
            "kernel_ms": kernels,
            "jitter_tries": jitter[(n, m, s)][0], "jitter": jitter[(n, m, s)][1],
            "product_flop": flop,
            "product_fraction_of_fp64_peak": stats(flop / (prod * 1e-3) / PEAK_F64),
        }
        rows.append(row)
        print(json.dumps({"n": n, "m": m, "s": s}),
              f"product {kernels['product']['median']:.3f} ms = {row['product_fraction_of_fp64_peak']['median']:.3f} of peak,"
              f" call {row['whole_call_ms']['median']:.3f} ms", flush=True)
    host = host_baseline()
    print(f"host np.random.multivariate_normal at {HOST_BASELINE}: {np.median(host):.1f} ms", flush=True)
    report = {
        "what": "joint posterior samples: kernel groups per call (rocprofv3 kernel trace), whole call (host clock, profiler "
                "off, normals drawn beforehand); medians with min / max over the timed calls",
        "device": device,
        "peak_fp64_mfma_flops": PEAK_F64,
        "flop_convention": "m^2 s for the triangle-aware product",
        "kernel_groups": {"transpose": "normals_transpose_kernel", "solve": "K*, L^-1 K* and the mean",
                          "padding": "factor_padding_kernel", "cov": "cov_tile_kernel (SYM, into the factor buffer)",
                          "factor": "launch_cholesky's kernels, durations summed", "product": "samples_tile_kernel"},
        "reps": a.reps,
        "rows": rows,
        "host_baseline": {"n": HOST_BASELINE[0], "m": HOST_BASELINE[1], "s": HOST_BASELINE[2],
                          "what": "np.random.multivariate_normal(mean, Sigma, s) on the device's Sigma (SVD on the host)",
                          "ms": stats(host)},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
