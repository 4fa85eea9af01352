"""Timing of max-value entropy search (kernels_mes.hip) on one MI355X: the scoring sweep (cbo_acq_sweep_mes:
mes_acq_kernel) at m = 2^24 candidates, K = 10 and 64 samples, beside the EI sweep's acq_kernel on the same grid, and the
Gumbel fit (cbo_gp_mes_gumbel: gumbel_quantiles_kernel) with the whole update_parameters at (n, grid_size) = (1024, 5000)
and (4096, 5000); against a numpy / scipy restatement of both steps on the host.

Two runs make one report:

    python scripts/mes_timing.py --calls-only                        # under rocprofv3 --kernel-trace --stats
    python scripts/mes_timing.py --trace <dir of that run> --out profiles/mes_timing.json

The first form only makes the device calls (a warm-up, then --reps of each) for
`rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python ...`.  The second times, with the profiler
off, whole calls (host clock around calls that end in a stream synchronise; median, min, max of --reps) and the host
restatement (numpy / scipy with the host's own thread count, fewer repetitions), and takes the kernels' times from the
trace.  VALU instructions of mes_acq_kernel are counted in its ISA (static counts: --isa <.s of kernels_mes.hip>).
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M_SWEEP = 1 << 24
N_SWEEP = 64
KS = [10, 64]
FITS = [(1024, 5000), (4096, 5000)]
D = 3


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def model(n, seed=0):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, D))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    return HipGaussianProcess(X, y, noise_var=1e-2)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def device_calls(reps, record):
    """Every timed device call; record(name, ms list) receives the whole-call times."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement, MaxValueEntropySearch
    g = model(N_SWEEP)
    pts = np.random.default_rng(1).uniform(-2.0, 2.0, (M_SWEEP, D))
    cands = CandidateGrid(pts, g)
    ei = CausalExpectedImprovement(0.0, "min", g)
    ei.sweep(cands)                                        # q, mu cached with the candidates: the sweeps below re-score
    record("ei_sweep_cached_m2^24", timed(lambda: ei.sweep(cands), reps + 1)[1:])
    for k in KS:
        mes = MaxValueEntropySearch(g, [(-2.0, 2.0)] * D, num_samples=k)
        mes.update_parameters()
        record(f"mes_sweep_cached_m2^24_K{k}", timed(lambda: mes.sweep(cands), reps + 1)[1:])
    cands.close()
    for n, size in FITS:
        gf = model(n)
        mes = MaxValueEntropySearch(gf, [(-2.0, 2.0)] * D)
        record(f"update_parameters_n{n}_grid{size}", timed(mes.update_parameters, reps + 1)[1:])


def host_restatement(reps):
    """numpy / scipy: update_parameters (the predict excluded: the device's mean and variance are given) and evaluate at
    the sweep's shape, extrapolated from a slice of candidates."""
    from scipy.optimize import bisect
    from scipy.special import log_ndtr
    from scipy.stats import norm
    out = {}
    rng = np.random.default_rng(2)
    for n, size in FITS:
        fmean = rng.standard_normal((n + size, 1))
        fsd = np.sqrt(rng.uniform(0.01, 1.0, (n + size, 1)))

        def fit():
            def probf(x):
                return 1 - np.exp(np.sum(log_ndtr(-(x - fmean) / fsd), axis=0))
            left, right = np.min(fmean - 5 * fsd), np.max(fmean + 5 * fsd)
            return [bisect(lambda x: probf(x) - v, left, right, maxiter=10000) for v in (0.25, 0.5, 0.75)]
        out[f"host_fit_gumbel_n{n}_grid{size}"] = stats(timed(fit, reps))
    rows = 1 << 20
    mean = rng.standard_normal((rows, 1))
    fsd = np.sqrt(rng.uniform(0.01, 1.0, (rows, 1)))
    for k in KS:
        mins = rng.standard_normal(k) - 2.0

        def evaluate():
            gamma = (mins - mean) / np.maximum(fsd, 1e-10)
            mc = np.clip(1 - norm.cdf(gamma), 1e-10, 1)
            return np.mean(-gamma * norm.pdf(gamma) / (2 * mc) - np.log(mc), axis=1)[:, None]
        t = stats(timed(evaluate, max(2, reps // 3)))
        scale = M_SWEEP / rows
        out[f"host_evaluate_m2^24_K{k}"] = {k2: (v * scale if k2 != "count" else v) for k2, v in t.items()}
        out[f"host_evaluate_m2^24_K{k}"]["note"] = f"measured on {rows} rows, scaled linearly to 2^24"
    return out


def kernel_stats(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {}
    out = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            for key in ("mes_acq_kernel", "acq_kernel", "gumbel_quantiles_kernel"):
                if re.search(r"\b" + key + r"\b", name) or (key == "acq_kernel" and "cbo::acq_kernel" in name):
                    if key == "acq_kernel" and "mes_acq_kernel" in name:
                        continue
                    out.setdefault(name, {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                          "average_us": float(row["AverageNs"]) / 1e3,
                                          "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3})
    return out


def kernel_launches(trace_dir):
    """Per-launch durations (us) from the kernel trace, labelled by the order device_calls makes them: per timed sweep
    one mes_acq_kernel (K = 10, then K = 64) or acq_kernel; per update_parameters one gumbel_quantiles_kernel (the two
    sweeps' fits at n = N_SWEEP, then FITS in order)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {}
    seq = {"mes_acq_kernel": [], "acq_kernel": [], "gumbel_quantiles_kernel": []}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            if "mes_acq_kernel" in name:
                seq["mes_acq_kernel"].append(us)
            elif "cbo::acq_kernel<false, false>" in name:
                seq["acq_kernel"].append(us)
            elif "gumbel_quantiles_kernel" in name:
                seq["gumbel_quantiles_kernel"].append(us)
    out = {"acq_kernel_m2^24 (EI, cached q, mu)": stats(seq["acq_kernel"]) if seq["acq_kernel"] else None}
    half = len(seq["mes_acq_kernel"]) // 2
    if half:
        out["mes_acq_kernel_m2^24_K10"] = stats(seq["mes_acq_kernel"][:half])
        out["mes_acq_kernel_m2^24_K64"] = stats(seq["mes_acq_kernel"][half:])
    g = seq["gumbel_quantiles_kernel"]
    if len(g) >= 2 + 2 * len(FITS):
        out[f"gumbel_quantiles_kernel_n{N_SWEEP}_grid5000"] = stats(g[:2])
        per = (len(g) - 2) // len(FITS)
        for i, (n, size) in enumerate(FITS):
            out[f"gumbel_quantiles_kernel_n{n}_grid{size}"] = stats(g[2 + i * per:2 + (i + 1) * per])
    return out


def isa_counts(path):
    """Static VALU instruction counts of each mes_acq_kernel instance in a device .s file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN3cbo14mes_acq_kernel\w*):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M):
        body = m.group(2)
        out[m.group(1)] = {"valu": len(re.findall(r"^\s+v_", body, re.M)),
                           "valu_f64": len(re.findall(r"^\s+v_\w*f64", body, re.M))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--isa")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mes_timing.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.calls_only:
        device_calls(3, lambda name, v: None)
        return
    calls = {}
    device_calls(a.reps, lambda name, v: calls.__setitem__(name, stats(v)))
    report = {"device": "MI355X", "whole_calls_ms": calls, "host_restatement_ms": host_restatement(a.reps),
              "host_threads": os.environ.get("OMP_NUM_THREADS", "default"),
              "kernels_from_trace": kernel_stats(a.trace) if a.trace else "not measured (no --trace)",
              "kernel_launches_us": kernel_launches(a.trace) if a.trace else "not measured (no --trace)",
              "isa_static_counts": isa_counts(a.isa) if a.isa else "not counted (no --isa)"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
