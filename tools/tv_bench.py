"""Cost of total-variation regularisation (mvn_set_regularization, csrc/mvn_tv.hpp) on the MI355X.
  pass    mvn_tv_time at 512^3 and 256^3: the pass against a plain streaming copy of the same volume (one read and one
          write), interleaved repeats, as a ratio and in TB/s of the 2 x volume bytes both have to move
  sweep   bench.py's headline problem (512^3, 6 views, 31^3 PSFs, one resident engine): ms per sweep with the
          regulariser off (lambda 0), Tikhonov and TV at the same lambda, each as the difference of a long and a short
          call, alternating in one process
  update  the engine's per-kind profile of a few sweeps with TV off and on: what the fused update pass pays for its
          third operand, and the pass itself inside the loop
    python tools/tv_bench.py [edge=512] [views=6] [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from libmultiviewnative_amd import native

args = sys.argv[1:]
edge = int(args[0]) if len(args) > 0 else 512
V = int(args[1]) if len(args) > 1 else 6
out_path = args[2] if len(args) > 2 else None
lib = native.lib()
res = {"pass": {}, "sweep": {}, "update": {}}

for e in sorted({edge, edge // 2}, reverse=True):
    shape = (e, e, e)
    runs = [lib.tv_time(shape, 20) for _ in range(5)]  # each call: 20 passes, then 20 copies
    tv, cp = min(r[0] for r in runs), min(r[1] for r in runs)
    gb = 2 * 4 * e ** 3 / 1e9
    res["pass"]["%d^3" % e] = {"tv_ms": tv, "copy_ms": cp, "ratio": tv / cp, "tv_TBps": gb / tv, "copy_TBps": gb / cp,
                               "all_ms": runs}
print(json.dumps(res["pass"]), flush=True)

shape = (edge, edge, edge)
eng = lib.engine(shape, V)
w = np.full(shape, 1.0 / V, np.float32)
for v in range(V):
    view, k1, k2 = bench.make_view(shape, v, 31)
    eng.set_view(v, view, w, k1, k2)
    del view
psi0 = np.full(shape, bench.start_value(), np.float32)
LAM, MINV, EPS = 0.005, 1e-4, 0.01 * bench.start_value()
SHORT, LONG, REPEATS = 2, 10, 3
KINDS = {"off": (0, 0.0), "tikhonov": (0, LAM), "tv": (1, LAM)}


def timed(kind, its, warm=True):
    k, lam = KINDS[kind]
    eng.set_regularization(k, EPS)
    if warm and k == 1:  # kind 0 frees the factor volume: its allocation belongs to neither timed call
        eng.iterate(1, lam, MINV, sync=True)
    eng.set_psi(psi0)
    eng.sync()
    t = time.perf_counter()
    eng.iterate(its, lam, MINV, sync=True)
    return time.perf_counter() - t


for kind in KINDS:  # (first use: plans, PSF forms, the factor volume)
    timed(kind, SHORT)
ms = {k: [] for k in KINDS}
for _ in range(REPEATS):
    for kind in KINDS:  # alternating: drifts of the clock hit all alike
        short = timed(kind, SHORT)
        long_ = timed(kind, LONG)
        ms[kind].append((long_ - short) / (LONG - SHORT) * 1e3)
best = {k: min(v) for k, v in ms.items()}
res["sweep"] = {"shape": shape, "views": V, "psf": [31, 31, 31], "lambda": LAM, "epsilon": EPS,
                "ms_per_sweep": best, "tv_over_off": best["tv"] / best["off"],
                "tv_over_tikhonov": best["tv"] / best["tikhonov"], "all_ms": ms}
print(json.dumps(res["sweep"]), flush=True)

for kind in ("off", "tv"):
    k, lam = KINDS[kind]
    eng.set_regularization(k, EPS)
    eng.set_psi(psi0)
    eng.profile(1)
    eng.iterate(4, lam, MINV, sync=True)
    prof = eng.profile_read()
    eng.profile(0)
    res["update"][kind] = {name: {"ms_per_launch": t / n, "launches": n} for name, (t, n) in prof.items() if n}
print(json.dumps(res["update"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
