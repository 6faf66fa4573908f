"""Cost of the padding policy "reflect" (mvn_set_pad_mode, csrc/mvn_reflect.hpp) on the MI355X.
  fill    mvn_reflect_time for a 512^3 stack in its 542 x 576 x 576 volume (31^3 PSFs, window at 15), float32 and
          uint16: the fill (its three launches) against a plain streaming copy of the whole volume, repeated, with the
          bytes the fill has to write (the margins) and what the copy moves
  call    one ABI call (inplace_gpu_deconvolve) of 10 iterations on that block under "zero" and under "reflect",
          alternating in one process after a first call of each that creates the engine and its plans
    python tools/reflect_bench.py [edge=512] [views=2] [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder

args = sys.argv[1:]
edge = int(args[0]) if len(args) > 0 else 512
V = int(args[1]) if len(args) > 1 else 2
out_path = args[2] if len(args) > 2 else None
PSF, ITERS, REPEATS = 31, 10, 3
lib = native.lib()
res = {"fill": {}, "call": {}}

dims = (edge,) * 3
# the extents the default policy picks for this block: dim0 exact under the direct leg, the others FFT-friendly
ext = (edge + PSF - 1,) + tuple({512: 576, 256: 288, 128: 160, 64: 96}.get(edge, edge + PSF - 1) for _ in range(2))
off = ((PSF - 1) // 2,) * 3
voxels, inside = float(np.prod(ext)), float(np.prod(dims))
for name, u16, esz in (("float32", False, 4), ("uint16", True, 2)):
    runs = [lib.reflect_time(dims, ext, off, u16=u16, reps=20) for _ in range(5)]  # each: 20 fills, then 20 copies
    fill, cp = min(r[0] for r in runs), min(r[1] for r in runs)
    margin_gb, copy_gb = (voxels - inside) * esz / 1e9, 2 * voxels * esz / 1e9
    res["fill"][name] = {"dims": dims, "ext": ext, "off": off, "fill_ms": fill, "copy_ms": cp, "ratio": fill / cp,
                         "margin_share": 1 - inside / voxels, "margin_GB_written": margin_gb,
                         "fill_write_TBps": margin_gb / fill, "copy_GB_moved": copy_gb, "copy_TBps": copy_gb / cp,
                         "all_ms": runs}
print(json.dumps(res["fill"]), flush=True)

views, k1, k2 = [], [], []
for v in range(V):
    view, a, b = bench.make_view(dims, v, PSF)
    views.append(view), k1.append(a), k2.append(b)
w = [np.full(dims, 1.0 / V, np.float32)] * V
h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, ITERS)
psi0 = np.full(dims, bench.start_value(), np.float32)


def timed(mode):
    psi = psi0.copy()
    lib.set_pad_mode(mode)
    try:
        t = lib.gpu_deconvolve_inplace(psi, h)
    finally:
        lib.set_pad_mode(None)
    assert np.isfinite(psi).all() and not np.array_equal(psi, psi0), lib.l.mvn_last_error().decode()
    return t


for mode in ("zero", "reflect"):  # (first use: the engine, its plans, the PSF forms)
    timed(mode)
secs = {"zero": [], "reflect": []}
c0 = lib.reflect_counters()
for _ in range(REPEATS):
    for mode in secs:  # alternating: drifts of the clock hit both alike
        secs[mode].append(timed(mode))
c1 = lib.reflect_counters()
best = {m: min(v) for m, v in secs.items()}
res["call"] = {"dims": dims, "views": V, "psf": [PSF] * 3, "iterations": ITERS, "seconds": best,
               "reflect_over_zero": best["reflect"] / best["zero"], "all_seconds": secs,
               "fills_per_reflect_call": (c1[1] - c0[1]) / REPEATS, "launches_per_reflect_call": (c1[0] - c0[0]) / REPEATS}
print(json.dumps(res["call"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
lib.check(lib.l.mvn_release_cached_engines())
