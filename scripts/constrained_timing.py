"""Timing of the constrained acquisition (cbo_acq_sweep_constrained: constrained_acq_kernel of kernels_con.hip) on one
MI355X at m = 2^24 candidates, n_con = 1, 2, 4, non-causal models, no per-candidate outputs:

  (a) the constrained epilogue alone: every (model, candidate set) pair is cached, so the call is constrained_acq_kernel
      plus argmax_final_kernel;
  (b) the existing EI epilogue: a cbo_acq_sweep re-sweep from cache on the same grid, in the same process.

The bar is (a) <= (n_con + 1) x (b) x 1.10.  Device times are taken between cbo_region_begin and
cbo_region_end around one call (median of --reps), the same way for both.  Also recorded: the fraction of the 8 TB/s HBM
roofline (a) reaches on its 2 (n_con + 1) doubles per candidate, and, for information, the end-to-end time of the host route
at m = 2^20 -- n_con + 1 device sweeps / predictions with their outputs copied back and scipy's product on the host.

    python scripts/constrained_timing.py --out profiles/constrained_timing.json
    python scripts/constrained_timing.py --ei-only --root <another tree> --out <json>    # (b) alone on that tree's build

The second form needs nothing of the constrained code: it measures (b) with another checkout's library (the parent
commit's own figure); --merge <that json> puts its result into the report.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

M_SWEEP = 1 << 24
M_HOST = 1 << 20
N_MODEL = 64
D = 3
N_CONS = [1, 2, 4]
HBM_BYTES_PER_S = 8e12


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def model(seed):
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N_MODEL, D))
    y = np.sin(X + seed).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N_MODEL, 1))
    return HipGaussianProcess(X, y, noise_var=1e-2)


def region_ms(ctx, fn, reps):
    """Device time of one call of fn between cbo_region_begin / cbo_region_end, reps times after one warm-up."""
    out = []
    for i in range(reps + 1):
        ctx.region_begin()
        fn()
        ms = ctx.region_end()
        if i:
            out.append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--ei-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement, _lib
    ctx = _lib.Context.get()
    pts = np.random.default_rng(1).uniform(-2.0, 2.0, (M_SWEEP, D))
    g = model(0)
    grid = CandidateGrid(pts, g)
    ei = CausalExpectedImprovement(float(g.Y.min()), "min", g)
    ei.sweep(grid)                                              # q, mu cached with the candidates
    report = {"device": ctx.name(), "m": M_SWEEP, "n_model": N_MODEL, "d": D, "reps": a.reps,
              "ei_epilogue_ms": stats(region_ms(ctx, lambda: ei.sweep(grid), a.reps))}
    b = report["ei_epilogue_ms"]["median"]
    report["ei_epilogue_roofline_fraction"] = 2 * 8 * M_SWEEP / (b * 1e-3) / HBM_BYTES_PER_S
    if not a.ei_only:
        from scipy.stats import norm
        from cbo_with_oop_amd.utils_functions import ProbabilityOfFeasibility
        cons_models = [model(10 + k) for k in range(max(N_CONS))]
        cons_grids = [CandidateGrid(pts, c) for c in cons_models]
        pofs = [ProbabilityOfFeasibility(c, 0.0, 0.1 * (k - 1), sense="<=" if k % 2 == 0 else ">=")
                for k, c in enumerate(cons_models)]
        report["constrained"] = {}
        for n_con in N_CONS:
            prod = ei
            for p in pofs[:n_con]:
                prod = prod * p
            grids = [grid] + cons_grids[:n_con]
            prod.sweep(grids)                                   # every pair cached from here on
            t = stats(region_ms(ctx, lambda: prod.sweep(grids), a.reps))
            bar = (n_con + 1) * b * 1.10
            report["constrained"][f"n_con={n_con}"] = {
                "epilogue_ms": t, "bar_ms": bar, "ratio_to_ei_epilogue": t["median"] / b,
                "ratio_to_bar": t["median"] / bar, "meets_bar": bool(t["median"] <= bar),
                "bytes_per_candidate": 16 * (n_con + 1),
                "roofline_fraction": 16 * (n_con + 1) * M_SWEEP / (t["median"] * 1e-3) / HBM_BYTES_PER_S}
        # the same bar with the EI epilogue measured again AFTER the constrained runs (drift within the process)
        report["ei_epilogue_ms_after"] = stats(region_ms(ctx, lambda: ei.sweep(grid), a.reps))
        # the host route at m = 2^20, end to end (wall clock): what a user of the parent commit has to do
        hp = np.ascontiguousarray(pts[:M_HOST])
        report["host_route_m2^20_ms"] = {}
        for n_con in N_CONS:
            def host_route():
                val = ei.sweep(hp, want_acq=True)["acq"][:, 0]
                for p in pofs[:n_con]:
                    mean, var = p.model.predict(hp)
                    u = (p.max_value - (mean[:, 0] + p.jitter)) / np.sqrt(var[:, 0])
                    val = val * norm.cdf(u if p.sense == "<=" else -u)
                return int(np.argmax(val))
            wall = []
            for _ in range(3):
                t0 = time.perf_counter()
                host_route()
                wall.append((time.perf_counter() - t0) * 1e3)
            hg = [CandidateGrid(hp, m_) for m_ in [g] + cons_models[:n_con]]
            prod = ei
            for p in pofs[:n_con]:
                prod = prod * p
            dev = []
            for _ in range(3):
                for x in hg:
                    x.close()
                hg = [CandidateGrid(hp, m_) for m_ in [g] + cons_models[:n_con]]
                t0 = time.perf_counter()
                prod.sweep(hg)                                  # substitution of every pair included
                dev.append((time.perf_counter() - t0) * 1e3)
            for x in hg:
                x.close()
            report["host_route_m2^20_ms"][f"n_con={n_con}"] = {"host_route": stats(wall), "one_device_call_fresh": stats(dev)}
        report["host_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
    if a.merge and os.path.exists(a.merge):
        parent = json.load(open(a.merge))
        report["parent_commit_ei_epilogue_ms"] = parent["ei_epilogue_ms"]
        pb = parent["ei_epilogue_ms"]["median"]
        for n_con in N_CONS:
            e = report["constrained"][f"n_con={n_con}"]
            e["ratio_to_parent_bar"] = e["epilogue_ms"]["median"] / ((n_con + 1) * pb * 1.10)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
