"""Timing of the point-wise acquisition passes (kernels_pointwise.hip) on one MI355X beside the EI pass (acq_kernel through
cbo_acq_sweep, whose code this feature does not touch) on the same box, the same model and the same candidate sets, at
2^20 and 2^24 candidates with q, mu cached: every timed call is the epilogue alone (the pass and the closing arg-max launch;
no per-candidate output).

The figures are the library's own region timer of the epilogue (cbo_set_profiling: device events around the pass and
argmax_final_kernel, `ms_acq`), one call per reading: --warmup unrecorded calls, then the median, min and max of --reps.
MPEI's reading also holds the plug-in incumbent's prediction epilogue over the model's n points.

    python scripts/pointwise_timing.py --out profiles/pointwise_timing.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [1 << 20, 1 << 24]
N, D = 40, 2
KINDS = (("LCB", 1, 1.0), ("PI", 2, 0.0), ("VAR", 3, 0.0), ("MPEI", 4, 0.0))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def models():
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    rng = np.random.default_rng(0)
    X = rng.uniform(-2.0, 2.0, (N, D))
    y = np.sin(2 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
    plain = HipGaussianProcess(X, y, variance=1.0, lengthscale=0.7, noise_var=1e-2)
    causal = HipGaussianProcess(X, y, variance=1.0, lengthscale=0.7, noise_var=1e-2,
                                mean_function=lambda a: 0.3 * np.sin(a).sum(1, keepdims=True),
                                variance_adjustment=lambda a: 0.05 + 0.02 * np.cos(a).sum(1, keepdims=True) ** 2)
    return {"plain": plain, "causal": causal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise_timing.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from cbo_with_oop_amd import CandidateGrid, _lib
    lib = _lib.load()
    ctx = _lib.Context.get()
    bv, bi = ctypes.c_double(), ctypes.c_int64()

    def epilogue_ms(call):
        out = []
        for i in range(a.warmup + a.reps):
            ctx.reset_timers()
            _lib.check(call())
            if i >= a.warmup:
                out.append(ctx.timers()["ms_acq"])
        return stats(out)

    report = {"device": ctx.name(), "n": N, "d": D, "timer": "cbo_get_timers ms_acq per call (pass + argmax_final_kernel)",
              "warmup": a.warmup, "passes_ms": {}}
    for label, g in models().items():
        y_best = float(np.median(g.Y))
        for m in SIZES:
            pts = np.random.default_rng(1).uniform(-2.5, 2.5, (m, D))
            grid = CandidateGrid(pts, g)
            ei = lambda: lib.cbo_acq_sweep(g._handle, grid._handle, y_best, 0, 0.0, 1.0, None, None, None,      # noqa: E731
                                           ctypes.byref(bv), ctypes.byref(bi))
            _lib.check(ei())                              # the substitution: q, mu are cached with the set from here on
            ctx.set_profiling(True)
            key = f"{label}_m2^{m.bit_length() - 1}"
            row = report["passes_ms"][key] = {"EI (cbo_acq_sweep, acq_kernel)": epilogue_ms(ei)}
            for name, kind, param in KINDS:
                row[name] = epilogue_ms(lambda: lib.cbo_acq_sweep_kind(g._handle, grid._handle, kind, y_best, 0, param, 1.0,
                                                                       None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
            row["EI again (drift check)"] = epilogue_ms(ei)
            ctx.set_profiling(False)
            grid.close()
            print(key, json.dumps({k: round(v["median"], 4) for k, v in row.items()}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
