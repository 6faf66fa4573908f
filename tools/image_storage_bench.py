"""What image storage mode 1 (mvn_set_image_storage, include/mvn_engine_api.h: uint16 images kept as uint16 on the
device) costs or gains on bench.py's headline problem with uint16 images: 512^3, 6 views, 31^3 PSFs, padding "none",
one resident engine.  Per library and image storage mode:
  * ms per iteration (mvn_engine_iterate), as the difference of a long and a short call;
  * the fused divide pass (rows_fused_div of mvn_engine_profile): ms per launch and bytes/s against its byte model,
    2B + vol with a float32 image, 2B + vol / 2 with a uint16 image (B: the half-spectrum array, vol: the real volume);
  * one blocking described call (mvn_deconvolve_described) of uint16 stacks in host memory, seconds.
Libraries are given with --lib, any number of times: each is timed in child processes of its own, one at a time, the
libraries alternating, --repeats rounds.  A library whose tree holds its own libmultiviewnative_amd package (the parent
commit built in a scratch copy) is driven through that package, so that the binding matches the symbols; a library
without the switch is timed in mode 0 only.  Giving the SAME parent build twice measures the spread between two runs of
one library, which is what a difference between two libraries has to be read against.
    python tools/image_storage_bench.py --lib A.so [--lib B.so ...] [--edge 512] [--views 6] [--repeats 3] [--out x.json]
  * the ingest pass (needs PyTorch for the device tensors; skipped without it): seconds of a blocking
    mvn_engine_set_view_described whose image (uint16, then float32) and weights (float32) are dense tensors in device
    memory and whose PSFs the slot already holds - two launches of the pass over the whole volume and a wait, nothing
    else.  The uint16 image is written as float32 in mode 0 (k_ingest3d<uint16>) and as uint16 in mode 1
    (k_ingest3d_u16); the weights' launch is the same in both, so the difference of the two modes is the difference of
    the two forms.  k_copy3d, which embeds float32 host stacks under the padded policies, has no entry point of its own
    either: a rocprofv3 --kernel-trace --stats run of `--child` lists it beside the ingest kernels."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAM, MINV = 0.006, 1e-4
SHORT, LONG = 2, 8


def tree_of(lib_path):
    """the repository tree a library belongs to (<tree>/libmultiviewnative_amd/lib/<name>.so), else this one"""
    t = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(lib_path))))
    return t if os.path.exists(os.path.join(t, "libmultiviewnative_amd", "native.py")) else ROOT


def child(lib_path, edge, V):
    tree = tree_of(lib_path)
    sys.path.insert(0, ROOT)  # (bench.py: make_view)
    sys.path.insert(0, tree)  # the library's own package first
    try:
        import torch  # before the library is loaded
        if not (torch.cuda.is_available() and hasattr(torch, "uint16")):
            torch = None
    except ImportError:
        torch = None
    import numpy as np
    import bench
    from libmultiviewnative_amd import native
    lib = native.Binding(lib_path)
    assert lib.backend_name() == "hip-gfx950", lib.backend_name()
    has_switch = hasattr(lib, "set_image_storage")
    shape = (edge, edge, edge)
    w = np.full(shape, 1.0 / V, np.float32)
    views, k1, k2 = [], [], []
    for v in range(V):
        view, a, b = bench.make_view(shape, v, 31)
        views.append(np.rint(view * 100).astype(np.uint16))  # [1000, 6000): what a camera's 16 bits might hold
        k1.append(a)
        k2.append(b)
        del view
    psi0 = np.full(shape, bench.start_value() * 100, np.float32)
    vol = 4.0 * edge * edge * edge
    B = 8.0 * edge * edge * (edge // 2)
    res = {"lib": lib_path, "tree": tree, "shape": shape, "views": V, "modes": {}}
    for mode in ((0, 1) if has_switch else (0,)):
        if has_switch:
            lib.set_image_storage(mode)
        eng = lib.engine(shape, V)
        for v in range(V):
            eng.set_view(v, views[v], w, k1[v], k2[v])

        def timed(its):
            eng.set_psi(psi0)
            eng.sync()
            t = time.perf_counter()
            eng.iterate(its, LAM, MINV, sync=True)
            return time.perf_counter() - t

        timed(SHORT)  # (first use: plans, PSF forms)
        per = []
        for _ in range(3):
            s, l = timed(SHORT), timed(LONG)
            per.append((l - s) / (LONG - SHORT) * 1e3)
        eng.profile(1)
        timed(SHORT)
        prof = eng.profile_read()
        eng.profile(False)
        ms_div, n_div = prof.get("rows_fused_div", (0.0, 0))
        model = 2 * B + (vol / 2 if mode == 1 else vol)
        entry = {"ms_per_iteration": min(per), "ms_per_iteration_all": per,
                 "fused_divide_ms": ms_div / n_div if n_div else None, "fused_divide_launches": n_div,
                 "fused_divide_model_bytes": model,
                 "fused_divide_TBps": model / (ms_div / n_div * 1e-3) / 1e12 if n_div and ms_div > 0 else None}
        if torch is not None:  # the ingest pass on stacks in device memory (see the module docstring)
            d_u16 = torch.from_numpy(views[0]).to("cuda:0")
            d_f32 = d_u16.to(torch.float32)
            d_w = torch.from_numpy(w).to("cuda:0")
            torch.cuda.synchronize()
            for name, img in (("u16", d_u16), ("f32", d_f32)):
                ts = []
                for _ in range(5):
                    t = time.perf_counter()
                    eng.set_view(0, img, d_w, k1[0], k2[0])
                    ts.append(time.perf_counter() - t)
                entry["set_view_device_%s_ms" % name] = min(ts[1:]) * 1e3  # (the first call may re-allocate the slot)
            del d_u16, d_f32, d_w
        eng.close()
        # one blocking described call of host uint16 stacks
        lib.set_pad_mode("none")
        lib.check(lib.l.mvn_release_cached_engines())
        psi = psi0.copy()
        t = time.perf_counter()
        lib.deconvolve_described(psi, views, [w] * V, k1, k2, LAM, MINV, 2)
        entry["described_call_s"] = time.perf_counter() - t
        lib.check(lib.l.mvn_release_cached_engines())
        lib.set_pad_mode(None)
        res["modes"][str(mode)] = entry
    if has_switch:
        lib.set_image_storage(0)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="internal: time one library in this process")
    args = ap.parse_args()
    if args.child:
        child(args.lib[0], args.edge, args.views)
        return
    runs = []
    for r in range(args.repeats):
        for i, path in enumerate(args.lib):  # alternating: drifts of the clock hit every library alike
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", path, "--edge", str(args.edge),
                                "--views", str(args.views)], capture_output=True, text=True, timeout=600)
            line = [x for x in p.stdout.split("\n") if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:  # (nothing more is started on the GPU after a child that failed)
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                raise SystemExit("child for %s failed with %d" % (path, p.returncode))
            one = json.loads(line[0][7:])
            one["round"], one["slot"] = r, i
            runs.append(one)
            print("round %d, %s: %s" % (r, path, {m: round(e["ms_per_iteration"], 3) for m, e in one["modes"].items()}),
                  flush=True)
    summary = {}
    for i, path in enumerate(args.lib):
        for m in ("0", "1"):
            xs = [x["modes"][m]["ms_per_iteration"] for x in runs if x["slot"] == i and m in x["modes"]]
            if xs:
                summary["%d:%s mode %s" % (i, path, m)] = {"best_ms": min(xs), "spread_ms": max(xs) - min(xs), "all_ms": xs}
    out = {"runs": runs, "summary": summary}
    print(json.dumps(summary, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
