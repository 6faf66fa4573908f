"""Cost of resampled views (mvn_deconvolve_resampled, csrc/mvn_resample.hpp) on the MI355X.
  pass    mvn_resample_time: an edge^3 block from an (edge / 4) x edge x edge uint16 raw stack, for the identity with a
          raw z-step of 4 block voxels and for that scale under a 90 degree rotation about axis 1 (a row of the block then
          walks across the raw planes), each against streaming traffic of the output's size (one volume read, two written)
  call    the warm ABI call, views x 10 iterations under "zero": mvn_deconvolve_resampled with computed weights from raw
          stacks in device memory and from raw stacks in host memory, and inplace_gpu_deconvolve on dense float32 host
          stacks of the block's extents, interleaved in one process after a first call of each
    python tools/resample_bench.py [edge=512] [views=6] [out.json]"""
import json
import os
import sys
import time

import torch  # before the library is loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder, view_geometry

args = sys.argv[1:]
edge = int(args[0]) if len(args) > 0 else 512
V = int(args[1]) if len(args) > 1 else 6
out_path = args[2] if len(args) > 2 else None
PSF, ITERS, REPEATS = 31, 10, 3
lib = native.lib()
res = {"pass": {}, "call": {}}

dims = (edge,) * 3
raw_shape = (edge // 4, edge, edge)
step = (raw_shape[0] - 1) / (edge - 1)
last = float(edge - 1)
MATRICES = {
    "identity with scale": [[step, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]],
    "rotation by 90 degrees with scale": [[0, 0, step, 0], [0, 1, 0, 0], [-1, 0, 0, last]],
}
BLEND = ((0, 0, 0), (8, 32, 32))
voxels = float(np.prod(dims))
for name, M in MATRICES.items():
    g = view_geometry(raw_shape, M, *BLEND)
    runs = [lib.resample_time(g, dims, u16=True, reps=10) for _ in range(3)]  # each: 10 passes, then 10 copies
    ms, cp = min(r[0] for r in runs), min(r[1] for r in runs)
    moved = 3 * voxels * 4 / 1e9
    res["pass"][name] = {"dims": dims, "raw": raw_shape, "pass_ms": ms, "copy_ms": cp, "ratio": ms / cp,
                         "pass_written_TBps": 2 * voxels * 4 / 1e9 / ms, "copy_TBps": moved / cp, "all_ms": runs}
print(json.dumps(res["pass"]), flush=True)

rng = np.random.default_rng(0)
raws = [rng.integers(100, 4000, raw_shape, dtype=np.uint16) for _ in range(V)]
geoms = [view_geometry(raw_shape, MATRICES["identity with scale" if v % 2 == 0 else "rotation by 90 degrees with scale"],
                       *BLEND) for v in range(V)]
views, k1, k2 = [], [], []
for v in range(V):
    view, a, b = bench.make_view(dims, v, PSF)
    views.append(view), k1.append(a), k2.append(b)
w = [np.full(dims, 1.0 / V, np.float32)] * V
h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, ITERS)
psi0 = np.full(dims, bench.start_value(), np.float32)
dev_raws = [torch.from_numpy(r.view(np.int16)).cuda() for r in raws]
torch.cuda.synchronize()


def timed(kind):
    psi = psi0.copy()
    lib.set_pad_mode("zero")
    try:
        if kind == "plain":
            t = lib.gpu_deconvolve_inplace(psi, h)
        else:
            call = lib.resample_call(psi, dev_raws if kind == "device" else raws, geoms, k1, k2, 0.006, 1e-4, ITERS,
                                     int16_is_uint16=True)
            t0 = time.perf_counter()
            call.run()
            t = time.perf_counter() - t0
    finally:
        lib.set_pad_mode(None)
    assert np.isfinite(psi).all() and not np.array_equal(psi, psi0), lib.l.mvn_last_error().decode()
    return t


KINDS = ("plain", "device", "host")
for kind in KINDS:  # (first use: the engine, its plans, the PSF forms)
    timed(kind)
secs = {k: [] for k in KINDS}
for _ in range(REPEATS):
    for kind in KINDS:  # interleaved: drifts of the clock hit all alike
        secs[kind].append(timed(kind))
best = {k: min(v) for k, v in secs.items()}
res["call"] = {"dims": dims, "raw": raw_shape, "views": V, "psf": [PSF] * 3, "iterations": ITERS, "seconds": best,
               "all_seconds": secs, "device_over_plain": best["device"] / best["plain"],
               "host_over_plain": best["host"] / best["plain"],
               "bytes_staged": {"plain": (2 * V + 1) * voxels * 4, "host": V * float(np.prod(raw_shape)) * 2 + voxels * 4,
                                "device": voxels * 4}}
print(json.dumps(res["call"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
lib.check(lib.l.mvn_release_cached_engines())
