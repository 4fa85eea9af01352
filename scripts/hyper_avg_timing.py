"""Timing of the hyper-parameter-marginalised causal EI (cbo_acq_sweep_hyper, kernels_hyper.hip) on one MI355X:
ONE call against the loop it replaces -- H x (set_hyperparameters + fit + sweep(want_acq=True)) with the average taken on the
host -- in the same process, at (n, m, H) = (50, 200, 10), (128, 16384, 10), (128, 16384, 50), d = 3, ARD, causal prior.

Both schedules of hyper_avg_kernel are timed (CBO_HIP_HYPER_SCHEDULE, read when a context is created: 1 = every workgroup
factors every sample itself, 2 = a first launch factors the samples and the sweep reads the factors back), each on a context
of its own, beside the automatic choice.  Per measurement: --warmup calls, then --reps timed ones; the host clock around the
whole call (wall) and the device time between cbo_region_begin / cbo_region_end around the same calls (a separate series:
the region's event synchronisation would otherwise sit inside the wall time); medians with min and max.

    python scripts/hyper_avg_timing.py --out profiles/hyper_avg_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(50, 200, 10), (128, 16384, 10), (128, 16384, 50)]
D = 3


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "count": int(v.size)}


def prior_mean(x):
    return 0.3 * np.sum(x, axis=1, keepdims=True)


def prior_var(x):
    return 0.2 + 0.1 * np.square(x[:, :1])


def problem(n, m, H, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, D))
    y = np.sin(X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-2.0, 2.0, (m, D))
    base = np.array([1.3, 0.8, 0.95, 1.1, 2e-2])
    rows = base * 2.0 ** rng.uniform(-1.0, 1.0, (H, D + 2))
    rows[:, -1] = np.maximum(rows[:, -1], 1e-2)
    return X, y, Xs, np.ascontiguousarray(rows)


def measure(ctx, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    wall, device = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    for _ in range(reps):
        ctx.region_begin()
        fn()
        device.append(ctx.region_end())
    return {"wall_ms": stats(wall), "device_region_ms": stats(device)}


def run(schedule, warmup, reps, with_loop):
    """One context under CBO_HIP_HYPER_SCHEDULE=schedule ("auto": unset): every shape's single call, and the loop if asked."""
    from cbo_with_oop_amd import CandidateGrid, CausalExpectedImprovement, IntegratedHyperParameterAcquisition, _lib
    from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
    if schedule == "auto":
        os.environ.pop("CBO_HIP_HYPER_SCHEDULE", None)
    else:
        os.environ["CBO_HIP_HYPER_SCHEDULE"] = str(schedule)
    ctx = _lib.Context(0)
    out = {}
    for n, m, H in SHAPES:
        X, y, Xs, rows = problem(n, m, H)
        model = HipGaussianProcess(X, y, variance=1.3, lengthscale=rows[0, 1:-1].copy(), ard=True, noise_var=2e-2,
                                   mean_function=prior_mean, variance_adjustment=prior_var, context=ctx)
        grid = CandidateGrid(Xs, model)
        y_best = float(y.min())
        acq = IntegratedHyperParameterAcquisition(model, lambda g: CausalExpectedImprovement(y_best, "min", g), samples=rows)
        key = f"n{n}_m{m}_H{H}"
        out[key] = {"single_call": measure(ctx, lambda: acq.sweep(grid, cost=3.0, want_acq=True), warmup, reps)}
        single = acq.sweep(grid, cost=3.0, want_acq=True)
        if with_loop:
            ei = CausalExpectedImprovement(y_best, "min", model)

            def loop():
                total = np.zeros(m)
                for row in rows:
                    model.set_hyperparameters(row[0], row[1:-1], row[-1], fit=True)
                    total = total + ei.sweep(grid, cost=3.0, want_acq=True)["acq"][:, 0]
                return total / H

            out[key]["loop"] = measure(ctx, loop, warmup, reps)
            out[key]["loop_equals_single_call_bits"] = bool(np.array_equal(loop(), single["acq"][:, 0]))
            model.set_hyperparameters(1.3, rows[0, 1:-1].copy(), 2e-2)
        grid.close()
        model.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyper_avg_timing.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from cbo_with_oop_amd import _lib
    auto = run("auto", a.warmup, a.reps, True)
    one = run(1, a.warmup, a.reps, False)
    two = run(2, a.warmup, a.reps, False)
    report = {"device": _lib.Context.get().name(), "d": D, "ard": True, "causal": True, "warmup": a.warmup, "reps": a.reps,
              "shapes": {}}
    for key in auto:
        s, l = auto[key]["single_call"], auto[key]["loop"]
        report["shapes"][key] = {
            "single_call_auto": s, "loop_H_x_set_hyper_fit_sweep_host_mean": l,
            "loop_equals_single_call_bits": auto[key]["loop_equals_single_call_bits"],
            "single_call_schedule_1_every_workgroup_factors": one[key]["single_call"],
            "single_call_schedule_2_factor_launch_then_sweep": two[key]["single_call"],
            "loop_over_single_wall_ratio": l["wall_ms"]["median"] / s["wall_ms"]["median"],
            "loop_over_single_device_ratio": l["device_region_ms"]["median"] / s["device_region_ms"]["median"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
