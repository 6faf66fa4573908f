"""Cost of the noise model (mvn_set_background / mvn_set_likelihood, the divide epilogues MVN_EPI_DIVIDE_NM of
csrc/mvn_pass_bodies.hpp) on the MI355X, on bench.py's headline problem: 512^3, 6 views, 31^3 PSFs, one resident engine.
  sweep   ms per sweep with both switches off, with a background only, and with background and likelihood, each as the
          difference of a long and a short call, alternating in one process
  divide  the engine's per-kind profile of a few sweeps in each mode: ms per launch of the divide pass (rows_fused_div:
          the DIVIDE form with the switches off, the NM form otherwise) and of every other kind beside it
A library given with --lib is timed instead of this tree's; one whose tree holds its own libmultiviewnative_amd package
(the parent commit built in a scratch copy) is driven through that package and, having no noise model, is timed with
the switches off only: the yardstick for "the default path did not move", to be read against the spread of its own
repeats.
    python tools/noise_model_bench.py [--lib X.so] [--edge 512] [--views 6] [--repeats 3] [--out x.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--edge", type=int, default=512)
ap.add_argument("--views", type=int, default=6)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out")
a = ap.parse_args()
tree = ROOT
if a.lib:
    t = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(a.lib))))
    if os.path.exists(os.path.join(t, "libmultiviewnative_amd", "native.py")):
        tree = t
sys.path.insert(0, ROOT)  # (bench.py: make_view)
sys.path.insert(0, tree)  # the library's own package first
import numpy as np
from libmultiviewnative_amd import native  # (before bench.py, which puts its own tree first)
import bench

lib = native.Binding(a.lib) if a.lib else native.lib()
assert lib.backend_name() == "hip-gfx950", lib.backend_name()
V, shape = a.views, (a.edge,) * 3
eng = lib.engine(shape, V)
has_model = hasattr(eng, "set_noise_model")
w = np.full(shape, 1.0 / V, np.float32)
B = 100.0
for v in range(V):
    view, k1, k2 = bench.make_view(shape, v, 31)
    eng.set_view(v, view + np.float32(B), w, k1, k2)  # (a camera frame: the light plus the offset)
    del view
psi0 = np.full(shape, bench.start_value(), np.float32)
LAM, MINV = 0.006, 1e-4
SHORT, LONG = 2, 10
MODES = {"off": (None, 0)}
if has_model:
    MODES.update({"background": ([B] * V, 0), "background+likelihood": ([B] * V, 1)})


def select(mode):
    if has_model:
        eng.set_noise_model(*MODES[mode])


def timed(mode, its):
    select(mode)
    eng.set_psi(psi0)
    eng.sync()
    t = time.perf_counter()
    eng.iterate(its, LAM, MINV, sync=True)
    return time.perf_counter() - t


for mode in MODES:  # (first use: plans, PSF forms)
    timed(mode, SHORT)
ms = {m: [] for m in MODES}
for _ in range(a.repeats):
    for mode in MODES:  # alternating: drifts of the clock hit all alike
        short = timed(mode, SHORT)
        long_ = timed(mode, LONG)
        ms[mode].append((long_ - short) / (LONG - SHORT) * 1e3)
res = {"library": a.lib or native.PRODUCT_SO, "shape": shape, "views": V, "psf": [31, 31, 31], "background": B,
       "sweep": {"ms_per_sweep": {m: min(v) for m, v in ms.items()}, "all_ms": ms}, "divide": {}}
print(json.dumps(res["sweep"]), flush=True)

for mode in MODES:
    select(mode)
    eng.set_psi(psi0)
    eng.profile(1)
    eng.iterate(4, LAM, MINV, sync=True)
    prof = eng.profile_read()
    eng.profile(0)
    res["divide"][mode] = {name: {"ms_per_launch": t / n, "launches": n} for name, (t, n) in prof.items() if n}
    if has_model and mode != "off":
        rows = eng.last_likelihood()
        res["divide"][mode]["D_per_sweep"] = rows[:, :, 0].sum(axis=1).tolist()
print(json.dumps(res["divide"]), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
