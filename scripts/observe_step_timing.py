"""Observe-step timing: the graph-level GP fits of ``fit_all_gaussian_processes`` in lockstep (one device call per
L-BFGS round for all GPs) against one after another (``fit_gaussian_process`` per GP, the reference's order), for the
complete graph's ten fit dependencies and the coral graphs' fifteen, at n = 100, 200 and 300 observational rows; then
``CBO.run()`` per trial on the complete graph.  Prints one JSON line per configuration; ``--out`` also writes them.

    python scripts/observe_step_timing.py --repeats 3 --out profiles/observe_step_timing.json
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def complete_rows(n, seed):
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import sample_from_model
    sem = CompleteGraph.define_sem()
    rng = np.random.default_rng(seed)
    rows = [sample_from_model(sem, rng.standard_normal(len(sem))) for _ in range(n)]
    return {v: np.array([r[v] for r in rows]) for v in rows[0] if not v.startswith("U")}


def coral_rows(n, seed):
    """Columns on the coral graphs' variables (their SEM is fitted to data not shipped here): smooth functions of a
    few latent draws.  Only the shapes matter for timing."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 4))
    c = {"N": z[:, 0], "L": np.abs(z[:, 1]) + 0.5, "TE": 0.3 * z[:, 1] + 0.1 * z[:, 2], "S": 0.5 * z[:, 2]}
    c["C"] = 0.5 + 0.1 * np.tanh(c["N"] + c["L"])
    c["T"] = 2.0 * c["S"] + 0.3 * z[:, 3]
    c["D"] = -1.0 * c["S"] + 0.2 * z[:, 3]
    c["O"] = 3.0 + 0.3 * np.sin(c["T"]) + 0.1 * c["D"]
    c["Y"] = np.cos(c["N"]) + 0.5 * c["O"] - 0.2 * c["C"] + 0.05 * z[:, 0] * z[:, 3]
    return c


def time_fit_all(graph, repeats):
    out = {}
    for mode, lockstep in (("lockstep", True), ("sequential", False)):
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            gps = graph.fit_all_gaussian_processes(lockstep=lockstep)
            ts.append(time.perf_counter() - t0)
            nfev = sum(m.optimization_result.nfev for m in gps.values())
            for m in gps.values():
                m.close()
        out[mode + "_ms"] = 1e3 * float(np.median(ts))
        out[mode + "_ms_all"] = [round(1e3 * t, 3) for t in ts]
    out["evaluations"] = int(nfev)
    out["speedup"] = out["sequential_ms"] / out["lockstep_ms"]
    return out


def time_run(trials, lockstep):
    from cbo_with_oop_amd.CBO import CBO
    from cbo_with_oop_amd.graphs import CompleteGraph
    from cbo_with_oop_amd.utils_functions.graph_functions import compute_interventions
    obs = complete_rows(200, seed=11)
    sem = CompleteGraph.define_sem()
    rng = np.random.default_rng(2)
    data = []
    for s in CompleteGraph.get_exploration_set("MIS"):
        lo, hi = np.array(CompleteGraph.bounds(s)).T
        x = rng.uniform(lo, hi, (5, len(s)))
        data.append((x, compute_interventions(sem, {v: "" for v in s}, x, target_variable="Y")))
    np.random.seed(9)
    agent = CBO(CompleteGraph, {k: v[:100] for k, v in obs.items()}, obs, data, num_trials=trials,
                initial_num_obs_samples=100, lockstep=lockstep)
    t0 = time.perf_counter()
    mon = agent.run()
    total = time.perf_counter() - t0
    return {"trials": trials, "observes": mon.type_trial.count(0), "interventions": mon.type_trial.count(1),
            "ms_per_trial": 1e3 * total / trials, "ms_total": 1e3 * total, "lockstep": lockstep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="100,200,300")
    ap.add_argument("--trials", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cbo_with_oop_amd import _lib
    from cbo_with_oop_amd.graphs import CompleteGraph, CoralGraph
    ctx = _lib.Context.get(0)
    warnings.simplefilter("ignore", RuntimeWarning)
    lines = []
    # warm-up: every kernel instantiation loaded once
    CompleteGraph(complete_rows(50, 0)).fit_all_gaussian_processes()
    for n in [int(v) for v in args.sizes.split(",")]:
        for name, graph in (("complete_graph", CompleteGraph(complete_rows(n, seed=n))),
                            ("coral_shapes", CoralGraph(coral_rows(n, seed=n)))):
            rec = {"what": "fit_all_gaussian_processes", "graph": name, "n": n, "gps": len(graph.fit_dependencies),
                   "device": ctx.name().strip()}
            rec.update(time_fit_all(graph, args.repeats))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    for lockstep in (True, False):
        rec = {"what": "CBO.run", "graph": "complete_graph"}
        rec.update(time_run(args.trials, lockstep))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
