"""Cost of taking k observations into a fitted model and sweeping again (cbo_gp_append_block) against the
two existing routes, device times between cbo_region_begin and cbo_region_end, medians of 15 runs after 3 warm-ups:

  (a) one cbo_gp_append_block + one cbo_acq_sweep                                   this build
  (b) k x (cbo_gp_append + cbo_acq_sweep)                                           --parent-lib (a build of the parent commit)
  (c) cbo_gp_set_data with the grown data + cbo_acq_sweep                           --parent-lib

fp64, non-causal, candidates with a kept solution.  Shapes: n0 = 4032, m = 16384, d = 3 with k = 8 and k = 64 (the bar:
(a) <= 0.5 min(b, c)), and n0 = 50, m = 200, d = 1 with k = 4 (launch latency; reported, no bar).  Before every timed run
the model is put back on its n0 points (cbo_gp_set_data) and swept, so that the candidates' solution is the parent's.  Every
measurement runs in a child process of its own on raw ctypes under its own time limit (the parent commit's library lacks
the new symbol and cannot be loaded through the package); the first failure ends the run.

Usage: python scripts/append_block_timing.py --parent-lib PATH [--out profiles/append_block_timing.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RUNS, WARM = 15, 3
HBM_PEAK, MFMA_PEAK = 8.0e12, 78.6e12
SHAPES = [dict(name="headline k=8", n0=4032, k=8, m_shape=[32, 32, 16], bar=0.5),
          dict(name="headline k=64", n0=4032, k=64, m_shape=[32, 32, 16], bar=0.5),
          dict(name="reference scale k=4", n0=50, k=4, m_shape=[200], bar=None)]


def problem(n, m_shape, seed=0):
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    box = [(-5.0, 5.0), (-5.0, 20.0), (-5.0, 5.0)][:len(m_shape)]
    lo, hi = np.array([b[0] for b in box]), np.array([b[1] for b in box])
    rng = np.random.default_rng(seed)
    f = lambda X: (np.cos(np.exp(-X[:, 0] / 3)) + sum(0.3 * np.sin(X[:, k]) for k in range(1, X.shape[1])))[:, None]
    X = rng.uniform(lo, hi, (n, len(box)))
    y = f(X) + 0.1 * rng.standard_normal((n, 1))
    return X, np.ascontiguousarray(y[:, 0]), meshgrid_candidates(box, m_shape)


def child(lib_path, route, n0, k, m_shape):
    """One measurement in this process: prints a JSON line {"ms": [...], "best_idx": ...}."""
    from cbo_with_oop_amd import _lib as B
    lib = ctypes.CDLL(lib_path)
    names = ["cbo_init", "cbo_gp_create", "cbo_gp_fit", "cbo_gp_set_data", "cbo_cands_create", "cbo_cands_keep_solution",
             "cbo_gp_append", "cbo_acq_sweep", "cbo_region_begin", "cbo_region_end", "cbo_last_error"]
    if route == "a":
        names.append("cbo_gp_append_block")
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = B.SIGNATURES[name]
    P = lambda a: a.ctypes.data_as(B.c_double_p)

    def ok(rc):
        assert rc == 0, (rc, lib.cbo_last_error())

    X, y, Xs = problem(n0 + k, m_shape)
    d, m = X.shape[1], Xs.shape[0]
    X0, y0 = np.ascontiguousarray(X[:n0]), np.ascontiguousarray(y[:n0])
    Xb, yb = np.ascontiguousarray(X[n0:]), np.ascontiguousarray(y[n0:])
    ctx, gp, cands = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    ok(lib.cbo_init(0, ctypes.byref(ctx)))
    ls = np.array([1.0])
    ok(lib.cbo_gp_create(ctx, 0, n0, d, P(X0), P(y0), None, None, 1.0, P(ls), 0, 1e-2, 1, ctypes.byref(gp)))
    tries, jit = ctypes.c_int(0), ctypes.c_double(0.0)
    ok(lib.cbo_gp_fit(gp, ctypes.byref(tries), ctypes.byref(jit)))
    assert tries.value == 0
    ok(lib.cbo_cands_create(ctx, m, d, P(Xs), None, None, 0, ctypes.byref(cands)))
    ok(lib.cbo_cands_keep_solution(cands, 1))
    y_best = float(y.min())
    bv, bi, ms, done = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_int(0)
    sweep = lambda: ok(lib.cbo_acq_sweep(gp, cands, y_best, 0, 0.0, 1.0, None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
    times = []
    for r in range(WARM + RUNS):
        ok(lib.cbo_gp_set_data(gp, n0, P(X0), P(y0), None, None))           # back on the n0 points, V the parent's
        sweep()
        ok(lib.cbo_region_begin(ctx))
        if route == "a":
            ok(lib.cbo_gp_append_block(gp, k, P(Xb), P(yb), None, None, ctypes.byref(done)))
            assert done.value == 1, "cbo_gp_append_block did not take the shortcut"
            sweep()
        elif route == "b":
            for i in range(k):
                ok(lib.cbo_gp_append(gp, P(np.ascontiguousarray(Xb[i])), float(yb[i]), 0.0, 0.0, ctypes.byref(done)))
                assert done.value == 1, "cbo_gp_append did not take the shortcut"
                sweep()
        else:
            ok(lib.cbo_gp_set_data(gp, n0 + k, P(X), P(y), None, None))
            sweep()
        ok(lib.cbo_region_end(ctx, ctypes.byref(ms)))
        if r >= WARM:
            times.append(ms.value)
    print(json.dumps({"ms": times, "best_idx": int(bi.value), "best_val": float(bv.value)}))


def measure(lib_path, route, shape):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path, route, str(shape["n0"]), str(shape["k"]),
           ",".join(str(s) for s in shape["m_shape"])]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{cmd}: exit {r.returncode}\n{r.stdout}{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_block_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]), int(a.child[3]), [int(s) for s in a.child[4].split(",")])
    if not a.parent_lib:
        ap.error("--parent-lib is required: routes (b) and (c) are measured on a build of the parent commit")
    from cbo_with_oop_amd import _lib
    result = {"runs": RUNS, "warm_up": WARM, "routes_b_c_library": "parent commit", "shapes": []}
    for shape in SHAPES:
        ma, mb, mc = (measure(lib, route, shape) for lib, route in ((_lib.LIB_PATH, "a"), (a.parent_lib, "b"),
                                                                      (a.parent_lib, "c")))
        ta, tb, tc = (float(np.median(x["ms"])) for x in (ma, mb, mc))
        n0, k, m = shape["n0"], shape["k"], int(np.prod(shape["m_shape"]))
        m_pad, kp = (m + 63) // 64 * 64, (k + 15) // 16 * 16
        # the pass over V for the new rows: V[0:n0] and B read once, kp x m_pad partial sums written per slice
        pass_bytes = 8.0 * n0 * (m_pad + 16) + 8.0 * n0 * 64
        pass_flops = 2.0 * kp * n0 * m_pad
        ratio = ta / min(tb, tc)
        entry = dict(shape, m=m, a_ms=ta, b_ms=tb, c_ms=tc, ratio_to_best_existing=ratio,
                     bar_met=None if shape["bar"] is None else bool(ratio <= shape["bar"]),
                     same_winner=bool(ma["best_idx"] == mb["best_idx"] == mc["best_idx"]),
                     v_rows_pass_bytes=pass_bytes, v_rows_pass_flops=pass_flops,
                     a_runs=ma["ms"], b_runs=mb["ms"], c_runs=mc["ms"])
        result["shapes"].append(entry)
        verdict = "no bar" if shape["bar"] is None else ("met" if entry["bar_met"] else "MISSED")
        print(f"{shape['name']}: n0={n0} m={m}  (a) block+sweep {ta:.4f} ms  (b) {k} x (append+sweep) {tb:.4f} ms  "
              f"(c) refit+sweep {tc:.4f} ms  a / min(b, c) = {ratio:.3f} (bar 0.5: {verdict})  winners equal: "
              f"{entry['same_winner']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
