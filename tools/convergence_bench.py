"""Cost of the convergence statistics (mvn_set_convergence) through the ABI call: 512^3, 6 views, 31^3 PSFs, resident,
the cyclic policy ("none") and the default one ("zero").  Per policy: ms per iteration with the statistics off, with
t = 0 (statistics only) and with t = 1e-30 (every sweep waits for its statistics on the host and never stops), as the
difference of a long and a short call so that staging and download drop out.  The three modes alternate in one
process; the best of the repeats is reported with the spread.  Then one realistic block (tests/ref_fixtures.py) at
t = 1e-3: sweeps run against the full count, and the time saved.
    python tools/convergence_bench.py [edge=512] [views=6] [out.json]
    python tools/convergence_bench.py trace [edge] [views]   (a few calls of each mode, for a separate
                                                                rocprofv3 --kernel-trace --stats run)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder

args = sys.argv[1:]
trace = bool(args) and args[0] == "trace"
if trace:
    args = args[1:]
edge = int(args[0]) if len(args) > 0 else 512
V = int(args[1]) if len(args) > 1 else 6
out_path = args[2] if len(args) > 2 else None
lib = native.lib()
shape = (edge, edge, edge)
rng = np.random.default_rng(0)
views = [rng.random(shape, dtype=np.float32) * 50 + 10 for _ in range(V)]
w = [np.full(shape, 1.0 / V, np.float32) for _ in range(V)]
ax = np.arange(31) - 15.0
g = np.exp(-0.5 * (ax[:, None, None] / 3) ** 2 - 0.5 * (ax[None, :, None] / 2) ** 2 - 0.5 * (ax[None, None, :] / 2) ** 2)
psf = (g / g.sum()).astype(np.float32)
kernels = ([psf] * V, [np.ascontiguousarray(psf[::-1, ::-1, ::-1])] * V)
psi0 = np.full(shape, 35.0, np.float32)
SHORT, LONG, REPEATS = 2, 12, 3
MODES = [("off", -1.0), ("t=0", 0.0), ("t=1e-30", 1e-30)]


def holder(its):
    return WorkspaceHolder(views, kernels[0], kernels[1], w, 0.006, 1e-4, its)


def timed_call(its, tol):
    lib.set_convergence(tol)
    try:
        psi = psi0.copy()
        s = lib.gpu_deconvolve_inplace(psi, holder(its))
        if np.array_equal(psi, psi0):
            raise RuntimeError(lib.l.mvn_last_error().decode())
        run, _ = lib.last_convergence()
        if tol >= 0 and run != its:
            raise RuntimeError("the call stopped early")
        return s
    finally:
        lib.set_convergence(-1)


if trace:
    lib.set_pad_mode("zero")
    for name, tol in MODES:
        timed_call(SHORT, tol)
    lib.set_pad_mode(None)
    sys.exit(0)

rows = []
for pad in ("none", "zero"):
    lib.set_pad_mode(pad)
    lib.check(lib.l.mvn_release_cached_engines())
    timed_call(SHORT, -1.0)  # (the first call of a plan allocates and prepares the PSFs: not timed)
    ms = {name: [] for name, _ in MODES}
    for _ in range(REPEATS):
        for name, tol in MODES:  # alternating, so that drifts of the clock or the host hit all three alike
            short = timed_call(SHORT, tol)
            long_ = timed_call(LONG, tol)
            ms[name].append((long_ - short) / (LONG - SHORT) * 1e3)
    best = {k: min(v) for k, v in ms.items()}
    for name, _ in MODES:
        rows.append({"pad": pad, "mode": name, "ms_per_it": best[name],
                     "spread_ms": max(ms[name]) - min(ms[name]), "all_ms": ms[name],
                     "vs_off": best[name] / best["off"]})
        print(json.dumps(rows[-1]), flush=True)
    lib.check(lib.l.mvn_release_cached_engines())
lib.set_pad_mode(None)

# one realistic block: how many of the sweeps a tolerance of 1e-3 leaves
from ref_fixtures import realistic_views  # noqa: E402

_, rv, rk1, rk2, rw, rpsi = realistic_views((128, 128, 128), V, (15, 15, 15), seed=7)
FULL = 40
real = {}
for name, tol in (("off", -1.0), ("t=1e-3", 1e-3)):
    lib.set_convergence(tol)
    try:
        h = WorkspaceHolder(rv, rk1, rk2, rw, 0.006, 1e-4, FULL)
        lib.gpu_deconvolve(rpsi, h, pad_mode="zero")  # (warm)
        t = time.perf_counter()
        lib.gpu_deconvolve(rpsi, h, pad_mode="zero")
        real[name] = (time.perf_counter() - t) * 1e3
        run, st = lib.last_convergence()
    finally:
        lib.set_convergence(-1)
    if name != "off":
        real["iterations_run"] = run
        real["r_k"] = (st[:, 0] / st[:, 2]).tolist()
real["time_saved_ms"] = real["off"] - real["t=1e-3"]
real["full_count"] = FULL
print(json.dumps(real), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump({"shape": shape, "views": V, "psf": [31, 31, 31], "iterations": [SHORT, LONG], "repeats": REPEATS,
                   "rows": rows, "realistic_block_128_15psf": real}, f, indent=1)
