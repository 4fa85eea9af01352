"""Timing of the joint posterior (cbo_gp_predict_cov / cbo_gp_cov_between, cov_tile_kernel of kernels_joint.hip) on one
MI355X, at (n, m) = (50, 200) (reference scale), (1024, 4096), (4096, 8192) and (4096, 16384).

Two runs make one report:

    python scripts/covariance_timing.py --calls-only                       # under rocprofv3 (kernel + copy trace)
    python scripts/covariance_timing.py --trace <dir of that run> --out profiles/covariance_timing.json

The first form only makes the calls (warm-up, then --reps timed ones per size and product) for
`rocprofv3 --kernel-trace --memory-copy-trace -d <dir> -o run --output-format csv -- python ...`.  The second times the
whole calls with the profiler off (host clock around calls that end in a stream synchronise) and takes from the trace
the time of cov_tile_kernel alone and of the device-to-host copy of the result (into the caller's pageable array), per
call; the whole call without the copy is the whole call less the median copy.  Every figure is a median
with its min and max.  Share of peak: flop / kernel time over the 78.6 TFLOP/s fp64 MFMA peak, counting n_pad m^2 flop
for the symmetric product (the upper half) and 2 n_pad m1 m2 for the cross product.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(50, 200), (1024, 4096), (4096, 8192), (4096, 16384)]
PEAK_F64 = 78.6e12


def problem(n, m, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return X, y, rng.uniform(-2.0, 2.0, (m, d)), rng.uniform(-2.0, 2.0, (m, d))


def n_pad(n):
    return -(-n // 128) * 128


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def run_calls(reps):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    out = {}
    for n, m in SIZES:
        X, y, Xs, Xt = problem(n, m)
        g = HipGaussianProcess(X, y, noise_var=1e-2)
        for kind in ("sym", "cross"):
            call = (lambda: g.predict(Xs, full_cov=True)) if kind == "sym" else \
                   (lambda: g.posterior_covariance_between_points(Xs, Xt))
            call()                                   # warm-up: code objects, workspaces, output buffer
            call()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()                                # returns after the stream is synchronised
                t.append((time.perf_counter() - t0) * 1e3)
            out[(n, m, kind)] = t
        g.close()
    return out


def read_trace(trace_dir, reps):
    """Per (size, product) the durations (ms) of the timed calls' cov_tile_kernel and of the copy of their result.  A
    pageable m1 x m2 result comes back in staged pieces (32 MiB each): the copy is the span from the first to the last
    device-to-host piece between the call's kernel and the next call's, so the last timed call of each group has
    none."""
    kfile = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    cfile = glob.glob(os.path.join(trace_dir, "**", "*memory_copy_trace.csv"), recursive=True)
    if not kfile:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(kfile[0]) as f:
        kern = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)
                      if "cov_tile_kernel" in r["Kernel_Name"])
    d2h = []
    if cfile:
        with open(cfile[0]) as f:
            d2h = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)
                         if "DEVICE_TO_HOST" in r["Direction"])
    per_call = 2 + reps
    expected = per_call * 2 * len(SIZES)
    if len(kern) != expected:
        raise SystemExit(f"expected {expected} cov_tile_kernel launches in the trace, found {len(kern)}")
    out, ki = {}, 0
    for n, m in SIZES:
        for kind in ("sym", "cross"):
            ks, cs = [], []
            for i in range(ki + 2, ki + per_call):
                ks.append((kern[i][1] - kern[i][0]) * 1e-6)
                if i + 1 < ki + per_call:
                    w = [(a, b) for a, b in d2h if kern[i][1] <= a < kern[i + 1][0]]
                    if w:
                        cs.append((w[-1][1] - w[0][0]) * 1e-6)
            out[(n, m, kind)] = {"kernel": ks, "copy": cs if len(cs) == len(ks) - 1 else []}
            ki += per_call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls-only", action="store_true", help="only make the calls (run under rocprofv3)")
    ap.add_argument("--trace", help="directory of the rocprofv3 run of --calls-only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_timing.json"))
    ap.add_argument("--wall-out", help="also write the raw whole-call times here")
    ap.add_argument("--wall-in", help="take the whole-call times from such a file instead of measuring them")
    a = ap.parse_args()
    if a.calls_only:
        run_calls(a.reps)
        return
    if not a.trace:
        raise SystemExit("--trace <dir> (the rocprofv3 run of --calls-only) is needed for the kernel and copy times")
    from cbo_with_oop_amd import _lib
    if a.wall_in:
        with open(a.wall_in) as f:
            raw = json.load(f)
        device = raw["device"]
        wall = {(int(k.split(":")[0]), int(k.split(":")[1]), k.split(":")[2]): v for k, v in raw["wall"].items()}
    else:
        wall = run_calls(a.reps)
        device = _lib.Context.get().name()
        if a.wall_out:
            with open(a.wall_out, "w") as f:
                json.dump({"device": device, "wall": {f"{n}:{m}:{k}": v for (n, m, k), v in wall.items()}}, f)
    traced = read_trace(a.trace, a.reps)
    rows = []
    for n, m in SIZES:
        for kind in ("sym", "cross"):
            k = traced[(n, m, kind)]
            flop = n_pad(n) * m * m * (1 if kind == "sym" else 2)
            kern_ms = np.asarray(k["kernel"])
            whole = np.asarray(wall[(n, m, kind)])
            copy = np.asarray(k["copy"]) if k["copy"] else None
            row = {
                "n": n, "m1": m, "m2": m, "n_pad": n_pad(n),
                "product": "predict_cov (symmetric, upper tiles)" if kind == "sym" else "cov_between (cross)",
                "flop": flop,
                "kernel_ms": stats(kern_ms),
                "whole_call_ms": stats(whole),
                "host_copy_ms": stats(copy) if copy is not None else "not measured (no copy in the trace)",
                "whole_call_without_copy_ms": stats(whole - np.median(copy)) if copy is not None else "not measured",
                "kernel_fraction_of_fp64_peak": stats(flop / (kern_ms * 1e-3) / PEAK_F64),
            }
            rows.append(row)
            print(json.dumps({key: row[key] for key in ("n", "m1", "product")}),
                  f"kernel {row['kernel_ms']['median']:.3f} ms = {row['kernel_fraction_of_fp64_peak']['median']:.3f} of peak,"
                  f" call {row['whole_call_ms']['median']:.3f} ms", flush=True)
    report = {
        "what": "joint posterior covariance: cov_tile_kernel alone (rocprofv3 kernel trace), whole call (host clock, "
                "profiler off), the result's device-to-host copy (rocprofv3 memory-copy trace); medians with min / max "
                "over the timed calls",
        "device": device,
        "peak_fp64_mfma_flops": PEAK_F64,
        "flop_convention": "n_pad m^2 for the symmetric product, 2 n_pad m1 m2 for the cross product",
        "reps": a.reps,
        "rows": rows,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
