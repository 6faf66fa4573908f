"""Cost of derived kernels (mvn_derive_kernels, csrc/mvn_psf.hpp) on the MI355X.
  derive  mvn_derive_time for V views of extents K, all four types: milliseconds per derivation (every launch) and of
          its correlation launches alone, and the double multiply-adds per second the correlation kernel reaches on
          the cropped correlations' count V (V - 1) prod(K)^2 (plus, for the efficient Bayesian type, the terms of the V
          autocorrelations whose d - t lands inside the kernel: prod(K)^2 per view)
  call    the warm ABI call, views x 10 iterations under "zero" from raw uint16 stacks in host memory with computed
          weights: kernels handed in (mvn_derive_kernels' own arrays), derivation on with raw PSF bytes the cache has
          not seen (scaled by a power of two: the derived kernels, and so the PSF spectra, keep their bits), and
          derivation on with the cache hit - interleaved in one process after a first call of each
    python tools/psf_bench.py [edge=512] [views=6] [out.json]      (edge 0: the derive part only)"""
import json
import os
import sys
import time

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
ITERS, REPEATS = 10, 3
lib = native.lib()
res = {"derive": {}, "call": {}}


def save():
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


for K in ((33, 31, 31), (33, 9, 9)):
    n = float(np.prod(K))
    for type_, name in enumerate(("independent", "efficient_bayesian", "optimization_1", "optimization_2")):
        runs = [lib.derive_time(V, K, type_, reps=3) for _ in range(3)]
        ms, corr = min(r[0] for r in runs), min(r[1] for r in runs)
        macs = V * (V - 1) * n * n if type_ in (1, 2) else 0.0
        if type_ == 1:
            macs += V * n * n
        res["derive"]["%s %s" % (K, name)] = {"views": V, "K": K, "derive_ms": ms, "correlate_ms": corr,
                                              "multiply_adds": macs, "gmacs_per_s": macs / corr / 1e6 if corr else None,
                                              "all_ms": runs}
        print(json.dumps({name: res["derive"]["%s %s" % (K, name)]}), flush=True)
save()
if edge <= 0:
    sys.exit(0)

dims = (edge,) * 3
raw_shape = (edge // 4, edge, edge)
step = (raw_shape[0] - 1) / (edge - 1)
last = float(edge - 1)
MATRICES = ([[step, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[0, 0, step, 0], [0, 1, 0, 0], [-1, 0, 0, last]])
BLEND = ((0, 0, 0), (8, 32, 32))
RAW_PSF = (7, 31, 31)  # through these matrices: K = (31, 31, 31) at edge 512
TYPE = 1
rng = np.random.default_rng(0)
raws = [rng.integers(100, 4000, raw_shape, dtype=np.uint16) for _ in range(V)]
geoms = [view_geometry(raw_shape, MATRICES[v % 2], *BLEND) for v in range(V)]
z, y, x = np.meshgrid(*[np.arange(-(m // 2), m // 2 + 1, dtype=np.float64) for m in RAW_PSF], indexing="ij")
psfs = [np.exp(-(z * z / (2 + 0.1 * v) + y * y / 18.0 + x * x / (18.0 + v))).astype(np.float32) for v in range(V)]
K = lib.psf_extents([RAW_PSF] * V, geoms)
k1, k2 = lib.derive_kernels(psfs, geoms, TYPE)
psi0 = np.full(dims, bench.start_value(), np.float32)
scale = [0]


def timed(kind):
    psi = psi0.copy()
    lib.set_pad_mode("zero")
    before = lib.derive_counters()
    try:
        if kind == "handed in":
            call = lib.resample_call(psi, raws, geoms, k1, k2, 0.006, 1e-4, ITERS)
        else:
            if kind == "derived, cold":
                scale[0] += 1
            call = lib.resample_call(psi, raws, geoms, [p * np.float32(2.0 ** scale[0]) for p in psfs], None, 0.006, 1e-4,
                                     ITERS)
            lib.set_kernel_derivation(1, TYPE)
        t0 = time.perf_counter()
        call.run()
        t = time.perf_counter() - t0
    finally:
        lib.set_kernel_derivation(0, 0)
        lib.set_pad_mode(None)
    moved = tuple(a - b for a, b in zip(lib.derive_counters(), before))
    assert moved[1:] == {"handed in": (0, 0), "derived, cold": (1, 0), "derived, hit": (0, 1)}[kind], (kind, moved)
    assert np.isfinite(psi).all() and not np.array_equal(psi, psi0), lib.l.mvn_last_error().decode()
    return t, psi


KINDS = ("handed in", "derived, cold", "derived, hit")
first = {kind: timed(kind)[1] for kind in KINDS}  # (first use: the engine, its plans, the PSF forms)
assert all(np.array_equal(first[k], first["handed in"]) for k in KINDS)
del first
secs = {k: [] for k in KINDS}
for _ in range(REPEATS):
    for kind in KINDS:  # interleaved: drifts of the clock hit all alike
        secs[kind].append(timed(kind)[0])
best = {k: min(v) for k, v in secs.items()}
res["call"] = {"dims": dims, "raw": raw_shape, "views": V, "raw_psf": RAW_PSF, "K": K, "type": TYPE, "iterations": ITERS,
               "seconds": best, "all_seconds": secs, "cold_over_handed_in": best["derived, cold"] / best["handed in"],
               "hit_over_handed_in": best["derived, hit"] / best["handed in"]}
print(json.dumps(res["call"]), flush=True)
save()
lib.check(lib.l.mvn_release_cached_engines())
