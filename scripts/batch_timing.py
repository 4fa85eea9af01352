"""Cost of one further pick of greedy batch selection (cbo_acq_sweep_batch) against the existing route to
the same pick, device times between cbo_region_begin and cbo_region_end, medians of 15 runs after a warm-up:

  (a) cbo_acq_sweep_batch with B = 1                       kept solution: no substitution is timed
  (b) the same with B = 9; (b - a) / 8 is one further pick
  (c) one cbo_gp_append + cbo_acq_sweep with a kept solution -- the existing route to the same pick -- on the library given
      with --parent-lib (a build of the parent commit), else on this build (the route's code is the same in both)

at the headline shape (n = 4096, m = 16384, d = 3, fp64, non-causal) and at the reference's scale (n = 50, m = 200).
cbo_gp_append needs a free padded row, so (c) starts 20 observations below n (the padded size, and with it the rows of V
that are read, is the same).  Every measurement runs in a child process of its own on raw ctypes (the parent commit's
library lacks the new symbol and cannot be loaded through the package).  The bar: (b - a) / 8 <= 0.5 (c).

Usage: python scripts/batch_timing.py [--parent-lib PATH] [--out profiles/batch_timing.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RUNS, WARM, B_LONG = 15, 3, 9
HBM_PEAK = 8.0e12
SHAPES = [dict(name="headline", n=4096, m_shape=[32, 32, 16]), dict(name="reference scale", n=50, m_shape=[200])]


def problem(n, m_shape, seed=0):
    from cbo_with_oop_amd.graphs import meshgrid_candidates
    box = [(-5.0, 5.0), (-5.0, 20.0), (-5.0, 5.0)][:len(m_shape)]
    lo, hi = np.array([b[0] for b in box]), np.array([b[1] for b in box])
    rng = np.random.default_rng(seed)
    f = lambda X: (np.cos(np.exp(-X[:, 0] / 3)) + sum(0.3 * np.sin(X[:, k]) for k in range(1, X.shape[1])))[:, None]
    X = rng.uniform(lo, hi, (n, len(box)))
    y = f(X) + 0.1 * rng.standard_normal((n, 1))
    extra = rng.uniform(lo, hi, (WARM + RUNS, len(box)))
    return X, y, meshgrid_candidates(box, m_shape), extra, f(extra)[:, 0]


def child(lib_path, mode, n, m_shape):
    """One measurement in this process: prints a JSON line {"ms": [...]}."""
    from cbo_with_oop_amd import _lib as B
    lib = ctypes.CDLL(lib_path)
    for name in ("cbo_init", "cbo_gp_create", "cbo_gp_fit", "cbo_cands_create", "cbo_cands_keep_solution", "cbo_gp_append",
                 "cbo_acq_sweep", "cbo_region_begin", "cbo_region_end", "cbo_last_error", "cbo_acq_sweep_batch"):
        if name == "cbo_acq_sweep_batch" and mode == "append":
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = B.SIGNATURES[name]
    P = lambda a: a.ctypes.data_as(B.c_double_p)

    def ok(rc):
        assert rc == 0, (rc, lib.cbo_last_error())

    X, y, Xs, extra, y_extra = problem(n - (20 if mode == "append" else 0), m_shape)
    d, m = X.shape[1], Xs.shape[0]
    ctx, gp, cands = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    ok(lib.cbo_init(0, ctypes.byref(ctx)))
    ls = np.array([1.0])
    yf = np.ascontiguousarray(y[:, 0])
    ok(lib.cbo_gp_create(ctx, 0, X.shape[0], d, P(X), P(yf), None, None, 1.0, P(ls), 0, 1e-2, 1, ctypes.byref(gp)))
    tries, jit = ctypes.c_int(0), ctypes.c_double(0.0)
    ok(lib.cbo_gp_fit(gp, ctypes.byref(tries), ctypes.byref(jit)))
    assert tries.value == 0
    ok(lib.cbo_cands_create(ctx, m, d, P(Xs), None, None, 0, ctypes.byref(cands)))
    ok(lib.cbo_cands_keep_solution(cands, 1))
    y_best = float(yf.min())
    bv, bi, ms = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    ok(lib.cbo_acq_sweep(gp, cands, y_best, 0, 0.0, 1.0, None, None, None, ctypes.byref(bv), ctypes.byref(bi)))   # V resident
    times, picks = [], None
    for r in range(WARM + RUNS):
        if mode == "append":
            x_new = np.ascontiguousarray(extra[r])
            done = ctypes.c_int(0)
            ok(lib.cbo_region_begin(ctx))
            ok(lib.cbo_gp_append(gp, P(x_new), float(y_extra[r]), 0.0, 0.0, ctypes.byref(done)))
            ok(lib.cbo_acq_sweep(gp, cands, y_best, 0, 0.0, 1.0, None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
            ok(lib.cbo_region_end(ctx, ctypes.byref(ms)))
            assert done.value == 1, "cbo_gp_append did not take the shortcut"
        else:
            nb = int(mode)
            vals, idxs = np.empty(nb), np.empty(nb, dtype=np.int64)
            ok(lib.cbo_region_begin(ctx))
            ok(lib.cbo_acq_sweep_batch(gp, cands, y_best, 0, 0.0, 1.0, nb, 0, P(vals), idxs.ctypes.data_as(B.c_int64_p),
                                       None, None, None))
            ok(lib.cbo_region_end(ctx, ctypes.byref(ms)))
            picks = idxs.tolist()
        if r >= WARM:
            times.append(ms.value)
    print(json.dumps({"ms": times, "picks": picks}))


def measure(lib_path, mode, shape):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path, str(mode), str(shape["n"]),
           ",".join(str(s) for s in shape["m_shape"])]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{cmd}: {r.stdout}{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]), [int(s) for s in a.child[3].split(",")])
    from cbo_with_oop_amd import _lib
    this_lib = _lib.LIB_PATH
    route_lib = a.parent_lib or this_lib
    result = {"runs": RUNS, "warm_up": WARM, "route_c_library": "parent commit" if a.parent_lib else "this build",
              "shapes": []}
    for shape in SHAPES:
        ma = measure(this_lib, 1, shape)
        mb = measure(this_lib, B_LONG, shape)
        mc = measure(route_lib, "append", shape)
        ta, tb, tc = (float(np.median(x["ms"])) for x in (ma, mb, mc))
        per_pick = (tb - ta) / (B_LONG - 1)
        n, m = shape["n"], int(np.prod(shape["m_shape"]))
        n_pad, m_pad = (n + 127) // 128 * 128, (m + 63) // 64 * 64
        ldv = m_pad + 16
        # what a further pick reads: the n rows of V, and the earlier fantasy rows (4 on average over picks 1..8)
        bytes_pick = 8.0 * n * ldv + 8.0 * m_pad * (B_LONG - 1) / 2
        entry = dict(shape, m=m, n_pad=n_pad, ldv=ldv, a_ms=ta, b_ms=tb, c_ms=tc, further_pick_ms=per_pick,
                     ratio_to_c=per_pick / tc, bar=0.5, bar_met=bool(per_pick <= 0.5 * tc),
                     bytes_per_pick=bytes_pick, fraction_of_8TBs=bytes_pick / (per_pick * 1e-3) / HBM_PEAK,
                     a_runs=ma["ms"], b_runs=mb["ms"], c_runs=mc["ms"], picks=mb["picks"])
        result["shapes"].append(entry)
        print(f"{shape['name']}: n={n} m={m}  (a) B=1 {ta:.4f} ms  (b) B={B_LONG} {tb:.4f} ms  further pick {per_pick:.4f} ms  "
              f"(c) append+sweep {tc:.4f} ms  ratio {per_pick / tc:.3f} (bar 0.5: {'met' if entry['bar_met'] else 'MISSED'})  "
              f"{bytes_pick / 1e6:.1f} MB per pick = {entry['fraction_of_8TBs']:.3f} of 8 TB/s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
