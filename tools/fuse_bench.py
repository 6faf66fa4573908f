"""Cost of fusion (mvn_fuse_resampled, csrc/mvn_fuse.hpp) on the MI355X, and what starting psi from it buys.
  pass    mvn_fuse_time: an edge^3 float32 block from `views` resident uint16 raw stacks of (edge / 4) x edge x edge, all
          under the identity with a raw z-step of 4 block voxels, and all under that scale with a 90 degree rotation
          about axis 1 (the geometries of tools/resample_bench.py): ms[0] the fusion, ms[1] one resample pass per view on
          the same stacks (each writing an image and a weights volume: the route without this pass, less its combining),
          ms[2] a plain copy of one volume - the three interleaved inside every call, the call repeated RUNS times
  call    the warm mvn_deconvolve_resampled call with computed weights from raw stacks in device memory, from a constant
          psi (psi start 0) and from the fusion (psi start 1): r_k = S_k / P_k of every sweep with the statistics on and
          no tolerance over SWEEPS sweeps, then the timed call under mvn_set_convergence(r) with the sweeps it ran, r the r_k
          that the constant start has reached after TARGET_SWEEP sweeps
    python tools/fuse_bench.py [edge=512] [views=6] [out.json]"""
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
from libmultiviewnative_amd.abi import view_geometry

args = sys.argv[1:]
edge = int(args[0]) if len(args) > 0 else 512
V = int(args[1]) if len(args) > 1 else 6
out_path = args[2] if len(args) > 2 else None
PSF, SWEEPS, RUNS, REPS, TARGET_SWEEP = 31, 12, 5, 5, 8
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
for name, M in MATRICES.items():
    geoms = [view_geometry(raw_shape, M, *BLEND)] * V
    runs = [lib.fuse_time(geoms, dims, u16=True, reps=REPS) for _ in range(RUNS)]
    cols = list(zip(*runs))
    stat = lambda x: {"min": min(x), "median": float(np.median(x)), "max": max(x)}
    res["pass"][name] = {"dims": dims, "raw": raw_shape, "views": V, "reps": REPS,
                         "fuse_ms": stat(cols[0]), "resample_passes_ms": stat(cols[1]), "copy_ms": stat(cols[2]),
                         "fuse_over_resample_passes": float(np.median(cols[0]) / np.median(cols[1])),
                         "fuse_over_copy": float(np.median(cols[0]) / np.median(cols[2])), "all_ms": runs}
print(json.dumps(res["pass"]), flush=True)

# a specimen of blobs in the block's frame, seen by every camera through its own geometry with its own noise, as uint16:
# raw voxel (a, b, c) of an identity view lies at block (a / step, b, c), of a rotated view at (last - c, b, a / step)
rng = np.random.default_rng(0)
fine, coarse = np.linspace(-1, 1, edge, dtype=np.float32), np.linspace(-1, 1, raw_shape[0], dtype=np.float32)
blobs = [(rng.uniform(-0.7, 0.7, 3), rng.uniform(0.05, 0.3), rng.uniform(500, 3000)) for _ in range(12)]


def specimen(z, y, x):
    out = np.full(raw_shape, 100.0, np.float32)
    for c, s, h in blobs:
        out += np.float32(h) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / np.float32(2 * s * s))
    return out


SEEN = {"identity with scale": specimen(coarse[:, None, None], fine[None, :, None], fine[None, None, :]),
        "rotation by 90 degrees with scale": specimen(-fine[None, None, :], fine[None, :, None], coarse[:, None, None])}
kinds = ["identity with scale" if v % 2 == 0 else "rotation by 90 degrees with scale" for v in range(V)]
raws = [np.clip(SEEN[k] + rng.normal(0, 1, raw_shape).astype(np.float32) * np.sqrt(SEEN[k]), 0, 65535).astype(np.uint16)
        for k in kinds]
geoms = [view_geometry(raw_shape, MATRICES[k], *BLEND) for k in kinds]
k1, k2 = [], []
for v in range(V):
    a, b = bench.make_view((PSF,) * 3, v, PSF)[1:]
    k1.append(a), k2.append(b)
start = float(np.mean([r.mean() for r in raws]))
dev_raws = [torch.from_numpy(r.view(np.int16)).cuda() for r in raws]
psi = torch.empty(dims, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()


def call(psi_start, sweeps, tolerance):
    psi.fill_(start)
    torch.cuda.synchronize()
    lib.set_pad_mode("zero")
    lib.set_convergence(tolerance)
    lib.set_psi_start(psi_start, start)
    try:
        c = lib.resample_call(psi, dev_raws, geoms, k1, k2, 0.006, 1e-4, sweeps, int16_is_uint16=True)
        t0 = time.perf_counter()
        c.run()
        t = time.perf_counter() - t0
        ran, rows = lib.last_convergence()
    finally:
        lib.set_psi_start(0, 0.0)
        lib.set_convergence(-1)
        lib.set_pad_mode(None)
    assert bool(torch.isfinite(psi).all()), lib.l.mvn_last_error().decode()
    return t, ran, [float(r[0] / r[2]) for r in rows]


for mode in (0, 1):  # (first use: the engine, its plans, the PSF forms)
    call(mode, 1, -1.0)
curves = {mode: call(mode, SWEEPS, 0.0)[2] for mode in (0, 1)}
TOLERANCE = curves[0][TARGET_SWEEP - 1] * (1 + 1e-9)  # the fixed r_k: what the constant start has reached after TARGET_SWEEP sweeps
timed = {0: [], 1: []}
for _ in range(3):
    for mode in (0, 1):  # interleaved: drifts of the clock hit both alike
        t, ran, _ = call(mode, 2 * SWEEPS, TOLERANCE)
        timed[mode].append({"seconds": t, "sweeps": ran})
res["call"] = {"dims": dims, "raw": raw_shape, "views": V, "psf": [PSF] * 3, "constant_start": start,
               "r_k": {"psi start 0": curves[0], "psi start 1": curves[1]}, "tolerance": TOLERANCE,
               "max_sweeps": 2 * SWEEPS, "psi start 0": timed[0], "psi start 1": timed[1]}
print(json.dumps(res["call"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
lib.check(lib.l.mvn_release_cached_engines())
