"""Cost of the vector extrapolation between sweeps (mvn_set_acceleration) on bench.py's headline problem: 512^3, 6
views, 31^3 PSFs, one resident engine.  ms per plain sweep (mvn_engine_iterate: the launches of the loop without the
switch) against ms per accelerated sweep (mvn_engine_iterate_accelerated), each as the difference of a long and a short
call so that the state volumes' allocation drops out; the two alternate in one process, the best of the repeats is
reported with the spread.
    python tools/accel_bench.py [edge=512] [views=6] [out.json]
    python tools/accel_bench.py trace [edge] [views]    (a few sweeps of each kind, for a separate
                                                          rocprofv3 --kernel-trace --stats run: the time of k_accel_a
                                                          and k_accel_b beside the loop's own passes)"""
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
trace = bool(args) and args[0] == "trace"
if trace:
    args = args[1:]
edge = int(args[0]) if len(args) > 0 else 512
V = int(args[1]) if len(args) > 1 else 6
out_path = args[2] if len(args) > 2 else None
lib = native.lib()
shape = (edge, edge, edge)
eng = lib.engine(shape, V)
w = np.full(shape, 1.0 / V, np.float32)
for v in range(V):
    view, k1, k2 = bench.make_view(shape, v, 31)
    eng.set_view(v, view, w, k1, k2)
    del view
psi0 = np.full(shape, bench.start_value(), np.float32)
LAM, MINV = 0.006, 1e-4
SHORT, LONG, REPEATS = 2, 10, 3


def timed(kind, its):
    eng.set_psi(psi0)
    eng.sync()
    t = time.perf_counter()
    if kind == "plain":
        eng.iterate(its, LAM, MINV, sync=True)
    else:
        lib.check(lib.l.mvn_engine_iterate_accelerated(eng.h, its, LAM, MINV, -1.0, None, None, None))
        eng.sync()
    return time.perf_counter() - t


if trace:
    for kind in ("plain", "accelerated"):
        timed(kind, 4)
    eng.close()
    sys.exit(0)

for kind in ("plain", "accelerated"):  # (first use: plans, PSF forms)
    timed(kind, SHORT)
ms = {"plain": [], "accelerated": []}
for _ in range(REPEATS):
    for kind in ("plain", "accelerated"):  # alternating: drifts of the clock hit both alike
        short = timed(kind, SHORT)
        long_ = timed(kind, LONG)
        ms[kind].append((long_ - short) / (LONG - SHORT) * 1e3)
best = {k: min(v) for k, v in ms.items()}
res = {"shape": shape, "views": V, "psf": [31, 31, 31], "iterations": [SHORT, LONG], "repeats": REPEATS,
       "ms_per_plain_sweep": best["plain"], "ms_per_accelerated_sweep": best["accelerated"],
       "ratio": best["accelerated"] / best["plain"], "all_ms": ms,
       "spread_ms": {k: max(v) - min(v) for k, v in ms.items()}}
_, _, alphas = eng.iterate_accelerated(LONG, LAM, MINV)
res["alphas_after_the_timed_calls"] = alphas.tolist()
print(json.dumps(res), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
