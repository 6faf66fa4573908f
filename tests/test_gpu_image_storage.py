"""Image storage mode 1 (mvn_set_image_storage, include/mvn_engine_api.h) on the MI355X: uint16 image stacks of described
calls stay uint16 on the device and the divide epilogue MVN_EPI_DIVIDE_U16 reads them (csrc/mvn_pass_bodies.hpp,
mvn_fixed.hpp, mvn_wave_rows.hpp; the uint16 -> uint16 ingest pass: csrc/mvn_ingest.hpp).

The reference everywhere is the SAME call in mode 0, bit for bit (np.array_equal): uint16 -> float32 is exact, so the
quotient sees the same float, and mode 0 is anchored to the CPU oracle by tests/test_gpu_described_stacks.py.  One case
here is held to the oracle as well (padding "none", 1e-4 of the maximum, the bound of that file).  Every case restores
mode 0 and releases the cached engines in a `finally`.  The shapes are the smallest of each form of the last-axis
kernels; tests/test_emu_image_storage.py runs the same cases on the host emulation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import realistic_views

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, MINV = 0.006, 1e-4
SHAPE, V, ITERS = (64, 64, 128), 4, 3

# case -> (shape, PSF extents, fx_rows of the plan): 2 views, 2 iterations.  The fixed-length and wave-row kernels take
# whole tiles only (rows_fixed, csrc/mvn_engine.cpp: d0 * d1 a multiple of the tile's rows): the (4, 16, d2) shapes are
# the smallest that run each of those forms, and the plan is asked that it does.  The shapes with 35, 15 and 60 rows
# fall to the run-time-radix kernels at the same last extents.
FORMS = {
    "run-time radix, odd d2": ((13, 17, 19), (5, 5, 5), 0),       # scalar epilogue, RP = d2 + 1
    "run-time radix, even d2": ((12, 16, 24), (5, 5, 5), 0),
    "fixed tiled, H = 32": ((4, 16, 64), (3, 5, 5), 1),
    "fixed tiled, H = 128": ((4, 16, 256), (3, 5, 5), 1),
    "fixed walking, 8 rows, H = 48": ((4, 16, 96), (3, 5, 5), 1),
    "fixed walking, 4 rows, H = 160": ((4, 16, 320), (3, 5, 5), 1),
    "fixed walking, 2 rows, H = 480": ((4, 16, 960), (3, 3, 5), 1),
    "fixed walking, H = 1024": ((4, 16, 2048), (3, 3, 5), 1),
    "wave rows, d2 = 512": ((4, 16, 512), (3, 5, 5), 1),            # no 512 x 512 planes: not the line layout
    "run-time radix, d2 = 256, 35 rows": ((5, 7, 256), (3, 5, 5), 0),
    "run-time radix, d2 = 96, 35 rows": ((5, 7, 96), (3, 5, 5), 0),
    "run-time radix, d2 = 320, 35 rows": ((5, 7, 320), (3, 5, 5), 0),
    "run-time radix, d2 = 960, 15 rows": ((3, 5, 960), (3, 3, 5), 0),
    "run-time radix, d2 = 512, 60 rows": ((6, 10, 512), (5, 5, 5), 0),
}


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    yield b
    b.set_image_storage(0)
    b.set_memory_mode(None)
    b.l.mvn_release_cached_engines()


def make_inputs(shape, nviews, ks, seed):
    _, views, k1, k2, w, psi0 = realistic_views(shape, nviews, ks, seed=seed)
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    assert all(0 < int(u.min()) and int(u.max()) < 65535 for u in u16)
    return u16, [u.astype(np.float32) for u in u16], k1, k2, w, psi0


@pytest.fixture(scope="module")
def stacks():
    """the stacks of the (64, 64, 128) cases: computed once, shared, never modified"""
    s = make_inputs(SHAPE, V, (7, 5, 5), 71)
    for a in s[0] + [s[5]]:
        a.setflags(write=False)
    return s


def call(b, mode, psi, views, w, k1, k2, pad="none", iters=ITERS):
    """one described call in image storage mode `mode`: (psi, growth of the two image storage counters)"""
    before_pad = b.get_pad_mode()
    b.set_pad_mode(pad)
    b.set_image_storage(mode)
    try:
        c0 = b.image_storage_counters()
        got = b.deconvolve_described(psi, views, w, k1, k2, LAM, MINV, iters)
        c1 = b.image_storage_counters()
    finally:
        b.set_image_storage(0)
        b.set_pad_mode(before_pad)
    return got, (c1[0] - c0[0], c1[1] - c0[1])


def both(b, psi0, views, w, k1, k2, **kw):
    """mode 0 then mode 1 on the same stacks, each on engines of its own: (reference, result, counters of mode 1)"""
    try:
        ref, d0 = call(b, 0, psi0.copy(), views, w, k1, k2, **kw)
        assert d0 == (0, 0), "mode 0 moved the image storage counters"
        assert not np.array_equal(ref, psi0), b.l.mvn_last_error().decode()
        b.check(b.l.mvn_release_cached_engines())
        got, d1 = call(b, 1, psi0.copy(), views, w, k1, k2, **kw)
    finally:
        b.set_image_storage(0)
        b.check(b.l.mvn_release_cached_engines())
    return ref, got, d1


def window(a, off=(1, 2, 3), fill=9):
    big = np.full(tuple(s + 2 * o + 1 for s, o in zip(a.shape, off)), fill, a.dtype)
    win = big[off[0]:off[0] + a.shape[0], off[1]:off[1] + a.shape[1], off[2]:off[2] + a.shape[2]]
    win[...] = a
    return win


@pytest.mark.parametrize("form", list(FORMS))
def test_every_kernel_form_divides_by_the_uint16_image(gpu, form):
    shape, ks, fx_rows = FORMS[form]
    assert gpu.plan_describe(shape)["fx_rows"] == fx_rows, "the shape does not run the kernel form it is listed for"
    nv, iters = 2, 2
    u16, _, k1, k2, w, psi0 = make_inputs(shape, nv, ks, 23)
    ref, got, d = both(gpu, psi0, u16, w, k1, k2, iters=iters)
    assert np.array_equal(got, ref), form
    # one divide pass per (view, iteration); dense host stacks under "none" are placed by the copy: no ingest pass
    assert d == (iters * nv, 0), (form, d)


def test_line_layout_and_fused_middle_pass(gpu):
    # as test_fused_middle_pass_on_described_stacks: the product's own form decision, no switch is set
    shape, nv, iters = (40, 512, 512), 2, 2
    u16, _, k1, _, w, psi0 = make_inputs(shape, nv, (13, 7, 5), 61)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        ref, _ = call(gpu, 0, psi0.copy(), u16, w, k1, k2, iters=iters)
        gpu.check(gpu.l.mvn_release_cached_engines())
        m0 = gpu.l.mvn_mid_fused_launch_count()
        got, d = call(gpu, 1, psi0.copy(), u16, w, k1, k2, iters=iters)
        assert gpu.l.mvn_mid_fused_launch_count() - m0 == iters * nv * 2, "the fused middle pass did not run"
    finally:
        gpu.set_image_storage(0)
        gpu.check(gpu.l.mvn_release_cached_engines())
    assert np.array_equal(got, ref) and d == (iters * nv, 0), d


@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
def test_padding_policies(gpu, stacks, pad):
    u16, f32, k1, k2, w, psi0 = stacks
    views = list(u16)
    if pad == "zero":  # a block of exact zeros: the guarded quotient is 0 there
        z = views[1].copy()
        z[10:20, 8:40, 16:80] = 0
        views[1] = z
    ref, got, d = both(gpu, psi0, views, w, k1, k2, pad=pad)
    assert np.array_equal(got, ref)
    assert np.isfinite(got).all()
    # the padded policies embed the stacks: one uint16 -> uint16 ingest pass per view
    assert d == (ITERS * V, 0 if pad == "none" else V), d
    if pad == "none":  # the anchor outside the code under test
        from oracle import binding as orc
        o = orc.cpu_deconvolve(psi0, WorkspaceHolder(f32, k1, k2, w, LAM, MINV, ITERS), 4)
        assert np.abs(got - o).max() <= 1e-4 * np.abs(o).max()


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_unaligned_windows(gpu, stacks, pad):
    u16, _, k1, k2, w, psi0 = stacks
    wins = [window(u) for u in u16]
    assert all(x.ctypes.data % 16 != 0 and not x.flags["C_CONTIGUOUS"] for x in wins)
    ref, got, d = both(gpu, psi0, wins, w, k1, k2, pad=pad)
    assert np.array_equal(got, ref)
    assert d == (ITERS * V, 0 if pad == "none" else V), d


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_mixed_element_types(gpu, stacks, pad):
    u16, f32, k1, k2, w, psi0 = stacks
    views = [u16[v] if v % 2 == 0 else f32[v] for v in range(V)]
    ref, got, d = both(gpu, psi0, views, w, k1, k2, pad=pad)
    assert np.array_equal(got, ref)
    assert d == (ITERS * 2, 0 if pad == "none" else 2), d


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_streamed_views(gpu, stacks, pad):
    u16, _, k1, k2, w, psi0 = stacks
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        ref, _ = call(gpu, 0, psi0.copy(), u16, w, k1, k2, pad=pad)
        for n in (V, 2):
            gpu.set_memory_mode("stream:%d" % n)
            out = {}
            for mode in (0, 1):
                gpu.check(gpu.l.mvn_release_cached_engines())
                s0 = gpu.stream_counters()
                got, d = call(gpu, mode, psi0.copy(), u16, w, k1, k2, pad=pad)
                out[mode] = (got, d, [b - a for a, b in zip(s0, gpu.stream_counters())])
            assert np.array_equal(out[0][0], ref) and np.array_equal(out[1][0], ref), n
            assert out[1][2] == out[0][2] == [1, n * ITERS, n * ITERS * (u16[0].nbytes + w[0].nbytes)], (n, out[1][2])
            assert out[1][1] == (ITERS * V, 0 if pad == "none" else (V - n) + n * ITERS), (n, out[1][1])
    finally:
        gpu.set_memory_mode(None)
        gpu.set_image_storage(0)
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_engine_api(gpu, stacks):
    u16, f32, k1, k2, w, psi0 = stacks
    out = {}
    try:
        for mode in (0, 1):
            gpu.set_image_storage(mode)
            c0 = gpu.image_storage_counters()
            e = gpu.engine(SHAPE, V)
            try:
                for v in range(V):
                    e.set_view(v, window(u16[v]) if v == 1 else (u16[v] if v != 2 else f32[v]), w[v], k1[v], k2[v])
                e.set_psi(psi0)
                e.iterate(ITERS, LAM, MINV)
                seq = e.get_psi()
                e.set_psi(psi0)  # one simultaneous step
                e.compute_delta(LAM, MINV)
                e.apply_delta()
                e.sync()
                sim = e.get_psi()
            finally:
                e.close()
            c1 = gpu.image_storage_counters()
            out[mode] = (seq, sim, (c1[0] - c0[0], c1[1] - c0[1]))
    finally:
        gpu.set_image_storage(0)
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    assert not np.array_equal(out[0][0], out[0][1])
    assert out[0][2] == (0, 0) and out[1][2] == (3 * (ITERS + 1), 0), out


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import test_gpu_image_storage as t
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
dev = torch.device("cuda:0")
u16, f32, k1, k2, w, psi0 = t.make_inputs(t.SHAPE, t.V, (7, 5, 5), 71)
have_u16 = hasattr(torch, "uint16")
print("torch.uint16:", have_u16)
kw = dict(int16_is_uint16=not have_u16)
D_u16 = [torch.from_numpy(u if have_u16 else u.view(np.int16)).to(dev) for u in u16]
# one view as an unaligned window of a larger tensor, one with a non-unit last stride
big = torch.empty((t.SHAPE[0] + 2, t.SHAPE[1] + 3, t.SHAPE[2] + 5), dtype=D_u16[0].dtype, device=dev)
win = big[1:1 + t.SHAPE[0], 2:2 + t.SHAPE[1], 3:3 + t.SHAPE[2]]
win.copy_(D_u16[1])
perm = D_u16[2].permute(2, 1, 0).contiguous().permute(2, 1, 0)
assert perm.stride(2) != 1
views = [D_u16[0], win, perm, D_u16[3]]
D_w = [torch.from_numpy(x).to(dev) for x in w]
torch.cuda.synchronize()
for pad in ("none", "zero"):
    gpu.set_pad_mode(pad)
    res = {}
    for mode in (0, 1):
        gpu.check(gpu.l.mvn_release_cached_engines())
        gpu.set_image_storage(mode)
        c0 = gpu.image_storage_counters()
        psi = torch.from_numpy(psi0.copy()).to(dev)
        gpu.deconvolve_described(psi, views, D_w, k1, k2, t.LAM, t.MINV, t.ITERS, **kw)
        c1 = gpu.image_storage_counters()
        res[mode] = (psi.cpu().numpy(), (c1[0] - c0[0], c1[1] - c0[1]))
    gpu.set_image_storage(0)
    assert not np.array_equal(res[0][0], psi0)
    assert np.array_equal(res[1][0], res[0][0]), pad
    # stacks in device memory are read where they lie: one uint16 -> uint16 ingest pass per view
    assert res[0][1] == (0, 0) and res[1][1] == (t.ITERS * t.V, t.V), (pad, res[0][1], res[1][1])
gpu.set_pad_mode(None)
gpu.check(gpu.l.mvn_release_cached_engines())
torch.cuda.synchronize()
print("ok")
"""


def test_images_in_device_memory_in_a_child_process(gpu):
    # (the module's own library handle stays idle meanwhile: one GPU process works at a time.  Time limit: loading
    # torch and the library into a new process takes seconds, the four calls less)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ))
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])


def test_mode_0_after_mode_1_has_been_used(gpu, stacks):
    u16, _, k1, k2, w, psi0 = stacks
    try:
        got1, d1 = call(gpu, 1, psi0.copy(), u16, w, k1, k2, pad="zero")
        got0, d0 = call(gpu, 0, psi0.copy(), u16, w, k1, k2, pad="zero")  # on the engine mode 1 left
    finally:
        gpu.set_image_storage(0)
        gpu.check(gpu.l.mvn_release_cached_engines())
    assert d1 == (ITERS * V, V) and d0 == (0, 0)
    assert np.array_equal(got0, got1)
