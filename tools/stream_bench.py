"""Out-of-core views measured through the ABI call: 512^3, 6 views, 31^3 PSFs, the cyclic policy ("none") and the
default one ("zero"); s = 0, 1, 2, 3, 6 views streamed (memory mode stream:s, s = 0 also as auto under a budget of
exactly the resident need from mvn_deconvolve_memory).  Per case: ms per iteration (difference of the best of two
long and two short calls, so that staging and download drop out), bytes streamed per iteration and the H2D rate they
achieved, against a plain pageable host -> device copy timed in the same process, and the bound
1.15 x max(resident ms per iteration, streamed bytes / that rate).
    python tools/stream_bench.py [edge=512] [views=6] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder

lib = native.lib()
edge = int(sys.argv[1]) if len(sys.argv) > 1 else 512
V = int(sys.argv[2]) if len(sys.argv) > 2 else 6
out_path = sys.argv[3] if len(sys.argv) > 3 else None
shape = (edge, edge, edge)
rng = np.random.default_rng(0)
views = [rng.random(shape, dtype=np.float32) * 50 + 10 for _ in range(V)]
w = [np.full(shape, 1.0 / V, np.float32) for _ in range(V)]
ax = np.arange(31) - 15.0
g = np.exp(-0.5 * (ax[:, None, None] / 3) ** 2 - 0.5 * (ax[None, :, None] / 2) ** 2 - 0.5 * (ax[None, None, :] / 2) ** 2)
psf = (g / g.sum()).astype(np.float32)
kernels = ([psf] * V, [np.ascontiguousarray(psf[::-1, ::-1, ::-1])] * V)
psi0 = np.full(shape, 35.0, np.float32)
SHORT, LONG, REPEATS = 2, 12, 2


def holder(its):
    return WorkspaceHolder(views, kernels[0], kernels[1], w, 0.006, 1e-4, its)


def pageable_h2d_gbs():
    """a plain hipMemcpy from pageable host memory (torch's copy of a CPU tensor), one view's stack"""
    host = torch.from_numpy(views[0])
    dev = torch.empty_like(host, device="cuda")
    dev.copy_(host)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(5):
        dev.copy_(host)
    torch.cuda.synchronize()
    rate = 5 * host.numel() * 4 / (time.perf_counter() - t) / 1e9
    del dev
    torch.cuda.empty_cache()
    return rate


def per_iteration_ms(mode, budget=None):
    lib.set_memory_mode(mode)
    lib.set_memory_budget(budget)
    try:
        times, counts = {SHORT: [], LONG: []}, None
        # (the first call of a plan allocates and prepares the PSFs: not timed)
        for its in [SHORT] + [SHORT, LONG] * REPEATS:
            psi = psi0.copy()
            c0 = lib.stream_counters()
            times[its].append(lib.gpu_deconvolve_inplace(psi, holder(its)))
            if np.array_equal(psi, psi0):
                raise RuntimeError(lib.l.mvn_last_error().decode())
            counts = [b - a for a, b in zip(c0, lib.stream_counters())]
        times = {k: min(v) for k, v in times.items()}
        ms = (times[LONG] - times[SHORT]) / (LONG - SHORT) * 1e3
        return ms, counts[2] / LONG  # bytes per iteration of the long call
    finally:
        lib.set_memory_budget(None)
        lib.set_memory_mode(None)


rows = []
for pad in ("none", "zero"):
    lib.set_pad_mode(pad)
    lib.check(lib.l.mvn_release_cached_engines())
    rate = pageable_h2d_gbs()
    res_ms, _ = per_iteration_ms("resident")
    need0 = lib.deconvolve_memory(holder(SHORT), 0)
    auto_ms, auto_b = per_iteration_ms("auto", budget=need0)
    rows.append({"pad": pad, "s": 0, "mode": "resident", "ms_per_it": res_ms, "pageable_h2d_gbs": rate})
    rows.append({"pad": pad, "s": 0, "mode": "auto (budget = resident need)", "ms_per_it": auto_ms,
                 "bytes_per_it": auto_b, "vs_resident": auto_ms / res_ms})
    print(json.dumps(rows[-2]), flush=True)
    print(json.dumps(rows[-1]), flush=True)
    for s in (1, 2, 3, V):
        lib.check(lib.l.mvn_release_cached_engines())
        ms, b = per_iteration_ms("stream:%d" % s)
        bound = 1.15 * max(res_ms, b / (rate * 1e9) * 1e3)
        rows.append({"pad": pad, "s": s, "mode": "stream:%d" % s, "ms_per_it": ms, "bytes_per_it": b,
                     "achieved_h2d_gbs": b / (ms * 1e-3) / 1e9, "pageable_h2d_gbs": rate, "bound_ms": bound,
                     "within_bound": ms <= bound, "memory_bytes": lib.deconvolve_memory(holder(SHORT), s)})
        print(json.dumps(rows[-1]), flush=True)
    lib.check(lib.l.mvn_release_cached_engines())
lib.set_pad_mode(None)
if out_path:
    with open(out_path, "w") as f:
        json.dump({"shape": shape, "views": V, "iterations": [SHORT, LONG], "rows": rows}, f, indent=1)
