"""sha256 of what the candidate-pass kernels return (acq_kernel, pointwise_acq_kernel, mes_acq_kernel and
constrained_acq_kernel: csrc/acq_pass.h) for a plain and a causal model at sizes around a workgroup's span and past the
grid-stride wrap with an odd tail: one line per call over its outputs and its winner.  Two builds that claim the same bits
print the same lines.  usage: acq_pass_digest.py [--root <another tree>] [m ...]"""
import argparse, ctypes, hashlib, os, sys
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("m", nargs="*", type=int, default=[1, 7, 511, 513, 1000, 2 * 2048 * 256 + 3])
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
from cbo_with_oop_amd import CandidateGrid, _lib
from cbo_with_oop_amd.GaussianProcessFactory import HipGaussianProcess
L = _lib.load()


def model(seed, causal):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (40, 2))
    y = np.cos(X + seed).sum(1, keepdims=True) + 0.05 * rng.standard_normal((40, 1))
    kw = {}
    if causal:
        kw = dict(mean_function=lambda v: 0.3 * np.sin(v).sum(1, keepdims=True),
                  variance_adjustment=lambda v: 0.05 + 0.02 * np.cos(v).sum(1, keepdims=True) ** 2)
    return HipGaussianProcess(X, y, variance=1.3, lengthscale=0.9, noise_var=1e-3, **kw)


def line(tag, rc, outs, bv, bi):
    h = hashlib.sha256()
    for o in outs:
        if o is not None:
            h.update(np.ascontiguousarray(o).tobytes())
    h.update(np.array([bv.value]).tobytes() + np.array([bi.value]).tobytes())
    print(f"{tag}: rc {rc} winner {bi.value} digest {h.hexdigest()[:24]}", flush=True)


models = {"plain": model(0, False), "causal": model(1, True)}
others = {"plain": model(2, False), "causal": model(3, True)}            # the constraints' models
for m in a.m:
    pts = np.random.default_rng(m).uniform(-2.5, 2.5, (m, 2))
    grids = {k: CandidateGrid(pts, g, index_offset=5 if k == "causal" else 0) for k, g in models.items()}
    ogrids = {k: CandidateGrid(pts, g) for k, g in others.items()}
    for name, g in models.items():
        c = grids[name]
        y_best = float(g.Y.min())
        new = lambda: (np.empty(m), np.empty(m), np.empty(m))
        for task in (0, 1):
            for cost in (1.0, 3.0):
                for outs in (True, False):
                    acq, mean, var = new() if outs else (None, None, None)
                    bv, bi = ctypes.c_double(), ctypes.c_int64()
                    rc = L.cbo_acq_sweep(g._handle, c._handle, y_best, task, 0.01, cost, _lib.dptr(acq), _lib.dptr(mean),
                                         _lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi))
                    line(f"m={m} {name} sweep task={task} cost={cost} outputs={int(outs)}", rc, (acq, mean, var), bv, bi)
        pm = pv = None
        if g.causal:
            pm = np.ascontiguousarray(g.mean_function(pts)[:, 0])
            pv = np.ascontiguousarray(g.variance_adjustment(pts)[:, 0])
        for noise in (0, 1):
            mean, var = np.empty(m), np.empty(m)
            rc = L.cbo_gp_predict(g._handle, m, _lib.dptr(np.ascontiguousarray(pts)), _lib.dptr(pm), _lib.dptr(pv), noise,
                                  _lib.dptr(mean), _lib.dptr(var))
            line(f"m={m} {name} predict noise={noise}", rc, (mean, var), ctypes.c_double(0.0), ctypes.c_int64(0))
        for kind, param in ((1, 2.0), (2, 0.01), (3, 0.0), (4, 0.01)):     # CBO_ACQ_LCB, _PI, _VAR, _MPEI
            for task in (0, 1):
                for outs in (True, False):
                    acq, mean, var = new() if outs else (None, None, None)
                    bv, bi = ctypes.c_double(), ctypes.c_int64()
                    rc = L.cbo_acq_sweep_kind(g._handle, c._handle, kind, y_best, task, param, 3.0, _lib.dptr(acq),
                                              _lib.dptr(mean), _lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi))
                    line(f"m={m} {name} kind={kind} task={task} outputs={int(outs)}", rc, (acq, mean, var), bv, bi)
        for k in (1, 10):
            mins = np.ascontiguousarray(y_best + np.linspace(-3.0, 0.5, k))
            for outs in (True, False):
                acq, mean, var = new() if outs else (None, None, None)
                bv, bi = ctypes.c_double(), ctypes.c_int64()
                rc = L.cbo_acq_sweep_mes(g._handle, c._handle, k, _lib.dptr(mins), 3.0, _lib.dptr(acq), _lib.dptr(mean),
                                         _lib.dptr(var), ctypes.byref(bv), ctypes.byref(bi))
                line(f"m={m} {name} mes K={k} outputs={int(outs)}", rc, (acq, mean, var), bv, bi)
        # the constraints: one causal and one plain model, whatever the objective's is
        cons = [("causal", 0.2, 0.0, 0), ("plain", -0.1, 0.01, 1)]
        for n_con in (0, 1, 2):
            for outs in (True, False):
                acq, ei = (np.empty(m), np.empty(m)) if outs else (None, None)
                pof = np.empty((n_con, m)) if outs and n_con else None
                bv, bi = ctypes.c_double(), ctypes.c_int64()
                gps = (ctypes.c_void_p * 2)(*[others[k]._handle for k, _, _, _ in cons])
                cds = (ctypes.c_void_p * 2)(*[ogrids[k]._handle for k, _, _, _ in cons])
                val = np.array([v for _, v, _, _ in cons])
                jit = np.array([j for _, _, j, _ in cons])
                sen = (ctypes.c_int * 2)(*[s for _, _, _, s in cons])
                rc = L.cbo_acq_sweep_constrained(g._handle, c._handle, y_best, 0, 0.01, 3.0, n_con, gps, cds, _lib.dptr(val),
                                                 _lib.dptr(jit), sen, _lib.dptr(acq), _lib.dptr(ei), _lib.dptr(pof),
                                                 ctypes.byref(bv), ctypes.byref(bi))
                line(f"m={m} {name} constrained n_con={n_con} outputs={int(outs)}", rc, (acq, ei, pof), bv, bi)
    for x in list(grids.values()) + list(ogrids.values()):
        x.close()
