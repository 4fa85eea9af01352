"""Timing of the integrated variance reduction (cbo_gp_integrated_variance_reduction: ivr_tile_kernel of
kernels_joint.hip and its closing launch) on one MI355X, at (n, m, p) = (4096, 8192, 16384) and (1024, 4096, 100000)
(emukit's default number of integration points), against emukit's per-candidate loop and a numpy / BLAS restatement.

Two runs make one report:

    python scripts/ivr_timing.py --calls-only                        # under rocprofv3 --kernel-trace --stats
    python scripts/ivr_timing.py --trace <dir of that run> --out profiles/ivr_timing.json

The first form only makes the device calls (two warm-up calls, then --reps timed ones per shape) for
`rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python ...`.  The second times, with the
profiler off:
  - whole IntegratedVarianceReduction.evaluate calls (host clock around calls that end in a stream synchronise);
  - emukit's loop, np.mean(model.calculate_variance_reduction(x[[i]], X_mc)) per candidate on the device's covariance
    entry points, over the first --loop-candidates candidates only; the whole loop is extrapolated linearly in m;
  - the numpy / BLAS restatement (scipy Cholesky, L^-1 K solves, one GEMM per block of integration points, the squares
    summed on the host), once per shape, with the host's own thread count;
and takes from the trace the time of ivr_tile_kernel (summed over the chunks of a call) and of the rest of the call's
kernels.  Flop are counted from shapes: 2 n_pad m p for the tile product.  Every figure is a median with its min and
max; the share of peak is the tile product's flop over the kernel time over the 78.6 TFLOP/s fp64 MFMA peak.
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

SHAPES = [(4096, 8192, 16384), (1024, 4096, 100000)]
PEAK_F64 = 78.6e12


def problem(n, m, p, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, d))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return X, y, rng.uniform(-2.0, 2.0, (m, d)), rng.uniform(-2.0, 2.0, (p, d))


def n_pad(n):
    return -(-n // 128) * 128


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def make(n, m, p):
    from cbo_with_oop_amd import IntegratedVarianceReduction
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    X, y, Xc, Xint = problem(n, m, p)
    g = HipGaussianProcess(X, y, noise_var=1e-2)
    return g, IntegratedVarianceReduction(g, [(-2.0, 2.0)] * 3, x_monte_carlo=Xint), X, y, Xc, Xint


def run_calls(reps):
    out = {}
    for n, m, p in SHAPES:
        g, ivr, _, _, Xc, _ = make(n, m, p)
        ivr.evaluate(Xc)                             # warm-up: code objects, workspace, partials buffer
        ivr.evaluate(Xc)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ivr.evaluate(Xc)
            t.append((time.perf_counter() - t0) * 1e3)
        out[(n, m, p)] = t
        g.close()
    return out


def emukit_loop(n, m, p, count):
    """ms per candidate of emukit's evaluate loop on the device's calculate_variance_reduction (first `count`)."""
    g, ivr, _, _, Xc, Xint = make(n, m, p)
    np.mean(g.calculate_variance_reduction(Xc[[0]], Xint))      # warm-up
    t0 = time.perf_counter()
    vals = [np.mean(g.calculate_variance_reduction(Xc[[i]], Xint)) for i in range(count)]
    per = (time.perf_counter() - t0) * 1e3 / count
    dev = ivr.evaluate(Xc[:count])[:, 0]
    g.close()
    return per, float(np.max(np.abs(dev - np.array(vals))) / np.max(np.abs(vals)))


def host_restatement(n, m, p, block=8192):
    """numpy / scipy: the whole IVR on the host, integration points in blocks (no m x p matrix at once).  Returns ms."""
    import scipy.linalg
    from oracle import gp_oracle as O
    X, y, Xc, Xint = problem(n, m, p)
    t0 = time.perf_counter()
    post = O.fit(X, y, noise_var=1e-2)
    V1 = scipy.linalg.solve_triangular(post.L, O.rbf_K(X, Xc), lower=True)
    var = O.predict(post, Xc)[1][:, 0]
    acc = np.zeros(m)
    for j0 in range(0, p, block):
        B = Xint[j0:j0 + block]
        V2 = scipy.linalg.solve_triangular(post.L, O.rbf_K(X, B), lower=True)
        C = O.rbf_K(Xc, B) - V1.T @ V2
        acc += np.einsum("ij,ij->i", C, C)
    host = acc / var / p
    return (time.perf_counter() - t0) * 1e3, host


def read_trace(trace_dir, reps):
    """Per shape and timed call: ivr_tile_kernel's time summed over the call's chunks, and the call's other kernels."""
    kfile = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not kfile:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(kfile[0]) as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)),
                      key=lambda r: r[0])
    # a call ends with argmax_final_kernel right behind ivr_finish_kernel: split the trace there
    calls, cur, seen_finish = [], [], False
    for r in rows:
        cur.append(r)
        if "ivr_finish_kernel" in r[2]:
            seen_finish = True
        elif seen_finish and "argmax_final_kernel" in r[2]:
            calls.append(cur)
            cur, seen_finish = [], False
    expected = (2 + reps) * len(SHAPES)
    if len(calls) != expected:
        raise SystemExit(f"expected {expected} calls in the trace, found {len(calls)}")
    out = {}
    for s, shape in enumerate(SHAPES):
        group = calls[s * (2 + reps) + 2:(s + 1) * (2 + reps)]
        tile = [sum((b - a) for a, b, k in c if "ivr_tile_kernel" in k) * 1e-6 for c in group]
        other = [sum((b - a) for a, b, k in c if "ivr_tile_kernel" not in k) * 1e-6 for c in group]
        chunks = [sum(1 for _, _, k in c if "ivr_tile_kernel" in k) for c in group]
        out[shape] = {"tile": tile, "other": other, "chunks": chunks}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls-only", action="store_true", help="only make the calls (run under rocprofv3)")
    ap.add_argument("--trace", help="directory of the rocprofv3 run of --calls-only")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-candidates", type=int, default=32, help="candidates of emukit's loop that are timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivr_timing.json"))
    a = ap.parse_args()
    if a.calls_only:
        run_calls(a.reps)
        return
    if not a.trace:
        raise SystemExit("--trace <dir> (the rocprofv3 run of --calls-only) is needed for the kernel times")
    from cbo_with_oop_amd import _lib
    traced = read_trace(a.trace, a.reps)
    wall = run_calls(a.reps)
    report_rows = []
    for n, m, p in SHAPES:
        k = traced[(n, m, p)]
        flop = 2 * n_pad(n) * m * p
        tile = np.asarray(k["tile"])
        whole = np.asarray(wall[(n, m, p)])
        per_cand, loop_err = emukit_loop(n, m, p, a.loop_candidates)
        host_ms, host = host_restatement(n, m, p)
        g, ivr, _, _, Xc, _ = make(n, m, p)
        dev = ivr.evaluate(Xc)[:, 0]
        g.close()
        loop_ms = per_cand * m
        row = {
            "n": n, "m": m, "p": p, "n_pad": n_pad(n),
            "flop_tile_product": flop,
            "chunks_per_call": int(np.median(k["chunks"])),
            "ivr_tile_kernel_ms": stats(tile),
            "other_kernels_ms": stats(k["other"]),
            "tile_kernel_fraction_of_fp64_peak": stats(flop / (tile * 1e-3) / PEAK_F64),
            "whole_call_ms": stats(whole),
            "emukit_loop": {
                "what": "np.mean(model.calculate_variance_reduction(x[[i]], X_mc)) per candidate on the device's "
                        "covariance entry points; timed over the first candidates only and extrapolated linearly to m",
                "timed_candidates": a.loop_candidates,
                "ms_per_candidate": per_cand,
                "extrapolated_ms": loop_ms,
                "max_rel_diff_to_ivr": loop_err,
            },
            "host_restatement": {
                "what": "numpy / scipy on the host (one run, the host's BLAS threads), integration points in blocks of 8192",
                "ms": host_ms,
                "max_rel_diff_to_ivr": float(np.max(np.abs(host - dev)) / np.max(np.abs(host))),
            },
            "speedup_over_emukit_loop": loop_ms / float(np.median(whole)),
            "speedup_over_host": host_ms / float(np.median(whole)),
        }
        report_rows.append(row)
        print(json.dumps({key: row[key] for key in ("n", "m", "p")}),
              f"tile {row['ivr_tile_kernel_ms']['median']:.3f} ms = "
              f"{row['tile_kernel_fraction_of_fp64_peak']['median']:.3f} of peak, call {np.median(whole):.3f} ms, "
              f"emukit loop ~{loop_ms:.0f} ms, host {host_ms:.0f} ms", flush=True)
    report = {
        "what": "integrated variance reduction: ivr_tile_kernel (summed over the chunks of a call) and the call's other "
                "kernels from a rocprofv3 kernel trace; whole calls with the profiler off (host clock); emukit's "
                "per-candidate loop (extrapolated from a subset) and a numpy / BLAS restatement as baselines; medians "
                "with min / max over the timed calls",
        "device": _lib.Context.get().name(),
        "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
        "peak_fp64_mfma_flops": PEAK_F64,
        "flop_convention": "2 n_pad m p for the tile product",
        "reps": a.reps,
        "rows": report_rows,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
