"""Image storage mode 1 (mvn_set_image_storage, include/mvn_engine_api.h) on the host emulation: uint16 image stacks of
described calls stay uint16 on the "device" - 2 bytes per voxel in the view's volume, read by the divide epilogue
MVN_EPI_DIVIDE_U16 (csrc/mvn_pass_bodies.hpp), written by the uint16 -> uint16 form of the ingest pass
(csrc/mvn_ingest.hpp) or placed by the copy itself.

The reference everywhere is the SAME call in mode 0, which must match bit for bit (np.array_equal): uint16 -> float32 is
exact, so the quotient sees the same float.  Mode 0 is anchored to the CPU oracle by the existing suite; one case here is
held to the oracle as well, under padding "none", with the bound tests/test_gpu_described_stacks.py uses (1e-4 of the
maximum).  Every case restores mode 0 and releases the cached engines in a `finally`.  tests/test_gpu_image_storage.py
runs the same cases on the device."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_DEVICE, WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")
MB = 1 << 20
LAM, MINV = 0.006, 1e-4

# case -> (shape, views, iterations, PSF extents, fx_rows of the plan).  The fixed-length and wave-row kernels take
# whole tiles only (rows_fixed, csrc/mvn_engine.cpp: d0 * d1 a multiple of the tile's rows): the (4, 16, d2) shapes are
# the smallest that run each of those forms, and the plan is asked that it does.  The shapes with 35, 15 and 60 rows
# fall to the run-time-radix kernels at the same last extents (long rows, partial tiles of ITS geometry).
FORMS = {
    "run-time radix, odd d2": ((13, 17, 19), 2, 2, (5, 5, 5), 0),      # scalar epilogue, RP = d2 + 1
    "run-time radix, even d2": ((12, 16, 24), 2, 2, (5, 5, 5), 0),
    "fixed tiled, H = 32": ((4, 16, 64), 2, 2, (3, 5, 5), 1),
    "fixed tiled, H = 128": ((4, 16, 256), 2, 2, (3, 5, 5), 1),
    "fixed walking, 8 rows, H = 48": ((4, 16, 96), 2, 2, (3, 5, 5), 1),
    "fixed walking, 4 rows, H = 160": ((4, 16, 320), 2, 2, (3, 5, 5), 1),
    "fixed walking, 2 rows, H = 480": ((4, 16, 960), 2, 2, (3, 3, 5), 1),
    "fixed walking, H = 1024": ((4, 16, 2048), 2, 2, (3, 3, 5), 1),
    "wave rows, d2 = 512": ((4, 16, 512), 2, 2, (3, 5, 5), 1),           # no 512 x 512 planes: not the line layout
    "run-time radix, d2 = 256, 35 rows": ((5, 7, 256), 2, 2, (3, 5, 5), 0),
    "run-time radix, d2 = 96, 35 rows": ((5, 7, 96), 2, 2, (3, 5, 5), 0),
    "run-time radix, d2 = 320, 35 rows": ((5, 7, 320), 2, 2, (3, 5, 5), 0),
    "run-time radix, d2 = 960, 15 rows": ((3, 5, 960), 2, 2, (3, 3, 5), 0),
    "run-time radix, d2 = 512, 60 rows": ((6, 10, 512), 2, 2, (5, 5, 5), 0),
}
# the shape of the further cases: an even last extent whose uint16 volume is a whole number of 4 KiB pages
# (2 * 16 * 32 * 32 bytes), and an odd one
EVEN, ODD = (16, 32, 32), (20, 36, 45)
V, ITERS = 4, 3


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    b = native.Binding(native.EMU_SO)
    yield b
    b.set_image_storage(0)
    b.set_memory_mode(None)
    b.set_memory_budget(None)
    b.l.mvn_release_cached_engines()


# the suite's pin of the direct dim0 leg (tests/conftest.py) and the product's defaults, as in test_emu_engine.py
@pytest.fixture(params=["suite pin", "product defaults"])
def leg(request, emu, monkeypatch):
    if request.param == "product defaults":
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    emu.l.mvn_release_cached_engines()
    yield request.param
    emu.l.mvn_release_cached_engines()


@functools.lru_cache(maxsize=None)
def inputs(shape, nviews=V, ks=(5, 5, 5), seed=23):
    """(uint16 views, the same values as float32, k1, k2, weights, psi0); computed once, never modified"""
    _, views, k1, k2, w, psi0 = realistic_views(shape, nviews, ks, seed=seed)
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    assert all(0 < int(u.min()) and int(u.max()) < 65535 for u in u16)
    for a in u16 + [psi0]:
        a.setflags(write=False)
    return u16, [u.astype(np.float32) for u in u16], k1, k2, w, psi0


def call(b, mode, psi, views, w, k1, k2, pad="none", iters=ITERS, locations=None, lam=LAM):
    """one described call in image storage mode `mode`: (psi, growth of the two image storage counters)"""
    before_pad = b.get_pad_mode()
    b.set_pad_mode(pad)
    b.set_image_storage(mode)
    try:
        c0 = b.image_storage_counters()
        c = b.describe_call(psi, views, w, k1, k2, lam, MINV, iters)
        for key, loc in (locations or {}).items():
            getattr(c, key[0])[key[1]].location = loc
        got = c.run()
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
        b.l.mvn_release_cached_engines()
        got, d1 = call(b, 1, psi0.copy(), views, w, k1, k2, **kw)
    finally:
        b.set_image_storage(0)
        b.l.mvn_release_cached_engines()
    return ref, got, d1


def window(a, off=(1, 2, 3), fill=9):
    """`a` as a window of a larger array of the same dtype: rows start 2 * off[2] bytes into a row of the larger one"""
    big = np.full(tuple(s + 2 * o + 1 for s, o in zip(a.shape, off)), fill, a.dtype)
    win = big[off[0]:off[0] + a.shape[0], off[1]:off[1] + a.shape[1], off[2]:off[2] + a.shape[2]]
    win[...] = a
    return win


@pytest.mark.parametrize("form", list(FORMS))
def test_every_kernel_form_divides_by_the_uint16_image(emu, leg, form):
    shape, nv, iters, ks, fx_rows = FORMS[form]
    assert emu.plan_describe(shape)["fx_rows"] == fx_rows, "the shape does not run the kernel form it is listed for"
    u16, _, k1, k2, w, psi0 = inputs(shape, nv, ks)
    ref, got, d = both(emu, psi0, u16, w, k1, k2, iters=iters)
    assert np.array_equal(got, ref), form
    # one divide pass per (view, iteration); dense host stacks under "none" are placed by the copy: no ingest pass
    assert d == (iters * nv, 0), (form, d)


def test_line_layout_and_fused_middle_pass(emu, monkeypatch):
    # 512 x 512 planes with PSFs of 3 planes under MVN_MID_FUSED=2, as tests/test_emu_acceleration.py makes its own
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    emu.l.mvn_release_cached_engines()
    shape, nv, iters = (12, 512, 512), 2, 2
    u16, _, k1, _, w, psi0 = inputs(shape, nv, (3, 5, 3), seed=60)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    try:
        ref, _ = call(emu, 0, psi0.copy(), u16, w, k1, k2, iters=iters)
        emu.l.mvn_release_cached_engines()
        m0 = emu.l.mvn_mid_fused_launch_count()
        got, d = call(emu, 1, psi0.copy(), u16, w, k1, k2, iters=iters)
        assert emu.l.mvn_mid_fused_launch_count() - m0 == iters * nv * 2, "the fused middle pass did not run"
    finally:
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    assert np.array_equal(got, ref) and d == (iters * nv, 0), d


def test_anchor_outside_the_code_under_test(emu):
    u16, f32, k1, k2, w, psi0 = inputs(EVEN)
    try:
        got, d = call(emu, 1, psi0.copy(), u16, w, k1, k2)
    finally:
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    assert d == (ITERS * V, 0)
    o = orc.cpu_deconvolve(psi0, WorkspaceHolder(f32, k1, k2, w, LAM, MINV, ITERS), 4)
    assert np.abs(got - o).max() <= 1e-4 * np.abs(o).max()


@pytest.mark.parametrize("shape", [EVEN, ODD], ids=str)
@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
def test_padding_policies(emu, shape, pad):
    u16, _, k1, k2, w, psi0 = inputs(shape)
    views = list(u16)
    if pad == "zero":  # a block of exact zeros: the guarded quotient is 0 there
        z = views[1].copy()
        z[2:7, 3:11, 4:15] = 0
        views[1] = z
    ref, got, d = both(emu, psi0, views, w, k1, k2, pad=pad)
    assert np.array_equal(got, ref)
    assert np.isfinite(got).all()
    # the padded policies embed the stacks: one uint16 -> uint16 ingest pass per view
    assert d == (ITERS * V, 0 if pad == "none" else V), d


@pytest.mark.parametrize("shape", [EVEN, ODD], ids=str)
@pytest.mark.parametrize("pad", ["none", "zero"])
def test_unaligned_windows(emu, shape, pad):
    u16, _, k1, k2, w, psi0 = inputs(shape)
    wins = [window(u) for u in u16]
    assert all(x.ctypes.data % 16 != 0 and not x.flags["C_CONTIGUOUS"] for x in wins)
    ref, got, d = both(emu, psi0, wins, w, k1, k2, pad=pad)
    assert np.array_equal(got, ref)
    assert d == (ITERS * V, 0 if pad == "none" else V), d


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_mixed_element_types(emu, pad):
    u16, f32, k1, k2, w, psi0 = inputs(EVEN)
    views = [u16[v] if v % 2 == 0 else f32[v] for v in range(V)]
    ref, got, d = both(emu, psi0, views, w, k1, k2, pad=pad)
    assert np.array_equal(got, ref)
    assert d == (ITERS * 2, 0 if pad == "none" else 2), d


@pytest.mark.parametrize("shape", [EVEN, ODD], ids=str)
@pytest.mark.parametrize("pad", ["none", "zero"])
def test_images_in_device_memory(emu, shape, pad):
    # (the emulation takes any pointer as device memory: the ingest pass reads the stacks where they lie)
    u16, _, k1, k2, w, psi0 = inputs(shape)
    wins = [window(u) if v % 2 else u for v, u in enumerate(u16)]
    loc = {("image", v): MVN_DEVICE for v in range(V)}
    ref, got, d = both(emu, psi0, wins, w, k1, k2, pad=pad, locations=loc)
    assert np.array_equal(got, ref)
    assert d == (ITERS * V, V), d


@pytest.mark.parametrize("pad", ["none", "zero"])
@pytest.mark.parametrize("n", [V, 2])
def test_streamed_views(emu, pad, n):
    u16, _, k1, k2, w, psi0 = inputs(ODD)
    try:
        ref, _ = call(emu, 0, psi0.copy(), u16, w, k1, k2, pad=pad)
        emu.l.mvn_release_cached_engines()
        emu.set_memory_mode("stream:%d" % n)
        out = {}
        for mode in (0, 1):
            s0 = emu.stream_counters()
            got, d = call(emu, mode, psi0.copy(), u16, w, k1, k2, pad=pad)
            out[mode] = (got, d, [b - a for a, b in zip(s0, emu.stream_counters())])
            emu.l.mvn_release_cached_engines()
    finally:
        emu.set_memory_mode(None)
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    assert np.array_equal(out[0][0], ref) and np.array_equal(out[1][0], ref)
    assert out[1][2] == out[0][2] == [1, n * ITERS, n * ITERS * (u16[0].nbytes + w[0].nbytes)], out
    # every upload of a streamed view under a padded policy is one ingest pass into its ring slot
    resident = V - n
    assert out[1][1] == (ITERS * V, 0 if pad == "none" else resident + n * ITERS), out[1][1]


def test_streamed_views_of_both_types_share_a_float32_ring(emu):
    # the ring's slots are as wide as the widest streamed image: with a float32 view among the streamed ones the
    # streamed uint16 views are converted as in mode 0, the resident ones stay uint16
    u16, f32, k1, k2, w, psi0 = inputs(EVEN)
    views = [u16[0], f32[1], u16[2], u16[3]]
    try:
        ref, _ = call(emu, 0, psi0.copy(), views, w, k1, k2)
        emu.l.mvn_release_cached_engines()
        emu.set_memory_mode("stream:2")  # (views 1 and 3 stream)
        got, d = call(emu, 1, psi0.copy(), views, w, k1, k2)
    finally:
        emu.set_memory_mode(None)
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    assert np.array_equal(got, ref)
    assert d == (ITERS * 2, 0), d


def test_engine_api(emu):
    u16, f32, k1, k2, w, psi0 = inputs(EVEN)
    out = {}
    try:
        for mode in (0, 1):
            emu.set_image_storage(mode)
            c0 = emu.image_storage_counters()
            e = emu.engine(EVEN, V)
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
            c1 = emu.image_storage_counters()
            out[mode] = (seq, sim, (c1[0] - c0[0], c1[1] - c0[1]))
    finally:
        emu.set_image_storage(0)
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    assert not np.array_equal(out[0][0], out[0][1])
    assert out[0][2] == (0, 0)
    # three uint16 views: ITERS sweeps and one simultaneous step; the window (view 1) takes no pass either - 2-D copies
    assert out[1][2] == (3 * (ITERS + 1), 0), out[1][2]


def test_prices(emu):
    u16, f32, k1, k2, w, psi0 = inputs(EVEN)
    d0, d1, d2 = EVEN
    assert (2 * d0 * d1 * d2) % 4096 == 0  # (the model rounds every allocation up to 4 KiB pages)
    emu.set_pad_mode("none")
    try:
        h = WorkspaceHolder(f32, k1, k2, w, LAM, MINV, ITERS)
        c16 = emu.describe_call(psi0.copy(), u16, w, k1, k2, LAM, MINV, ITERS)
        c32 = emu.describe_call(psi0.copy(), f32, w, k1, k2, LAM, MINV, ITERS)
        mixed = emu.describe_call(psi0.copy(), [u16[0], f32[1], u16[2], f32[3]], w, k1, k2, LAM, MINV, ITERS)
        for s in (0, 2, V):
            plain = emu.deconvolve_memory(h, s)
            assert emu.deconvolve_memory_described(c16, s) == plain  # mode 0
            assert emu.deconvolve_memory_described(h, s) == plain    # no descriptors
            emu.set_image_storage(1)
            assert emu.deconvolve_memory_described(h, s) == plain
            assert emu.deconvolve_memory_described(c32, s) == plain  # float32 images are never narrowed
            # resident views save half a volume each; the two ring slots of streamed uint16 views a quarter each
            saved = ((V - s) + (2 if s else 0)) * 2 * d0 * d1 * d2
            assert emu.deconvolve_memory_described(c16, s) == plain - saved, s
            emu.set_image_storage(0)
        emu.set_image_storage(1)
        assert emu.deconvolve_memory_described(mixed, 0) == emu.deconvolve_memory(h, 0) - 2 * 2 * d0 * d1 * d2
        # views 1 and 3 stream, both float32: the ring stays float32, the resident views 0 and 2 are uint16
        assert emu.deconvolve_memory_described(mixed, 2) == emu.deconvolve_memory(h, 2) - 2 * 2 * d0 * d1 * d2
    finally:
        emu.set_image_storage(0)
        emu.set_pad_mode(None)


def test_the_planner_plans_with_the_prices(emu):
    u16, _, k1, k2, w, psi0 = inputs(EVEN)
    emu.set_pad_mode("none")
    try:
        emu.set_image_storage(1)
        budget = emu.deconvolve_memory_described(emu.describe_call(psi0.copy(), u16, w, k1, k2, LAM, MINV, ITERS), 0)
        emu.set_image_storage(0)
        emu.set_memory_mode("auto")
        emu.set_memory_budget(budget)
        emu.l.mvn_release_cached_engines()
        s0 = emu.stream_counters()
        got, d = call(emu, 1, psi0.copy(), u16, w, k1, k2)
        assert emu.stream_counters() == s0, "mode 1 streamed views inside its own resident figure"
        assert d == (ITERS * V, 0)
        emu.l.mvn_release_cached_engines()
        ref, _ = call(emu, 0, psi0.copy(), u16, w, k1, k2)
        s1 = emu.stream_counters()
        assert s1[0] == s0[0] + 1 and s1[1] >= s0[1] + ITERS, "mode 0 fits the mode-1 figure"
    finally:
        emu.set_memory_mode(None)
        emu.set_memory_budget(None)
        emu.set_image_storage(0)
        emu.set_pad_mode(None)
        emu.l.mvn_release_cached_engines()
    assert np.array_equal(got, ref)


_CHILD = r"""
import os, sys
import numpy as np
root, pad = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import test_emu_image_storage as t
emu = native.Binding(native.EMU_SO)
MB = 1 << 20
shape = (32, 128, 126)
u16, f32, k1, k2, w, psi0 = t.inputs(shape, 3, (5, 5, 5), 11)
emu.set_pad_mode(pad)
ref, _ = t.call(emu, 0, psi0.copy(), u16, w, k1, k2, pad=pad, iters=2)
emu.check(emu.l.mvn_release_cached_engines())
emu.check(emu.l.mvn_plan_store_clear())
emu.set_image_storage(1)
c = emu.describe_call(psi0.copy(), u16, w, k1, k2, t.LAM, t.MINV, 2)
need = emu.deconvolve_memory_described(c, 0)
assert need < emu.deconvolve_memory(c, 0)
# the model's figure is what the call allocates ("auto": the exact planner)
os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need // MB))
emu.set_memory_mode("auto")
before = emu.stream_counters()
got = c.run()
assert emu.stream_counters() == before, "the call streamed views"
assert np.array_equal(got, ref)
assert emu.image_storage_counters()[0] == 2 * 3
assert not emu.l.mvn_last_error().decode(), emu.l.mvn_last_error().decode()
print("ok")
"""


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_the_model_is_what_is_allocated(emu, pad):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("MVN_EMU_TOTAL_MB", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, pad], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout.split("\n")[-2], (r.stdout[-2000:], r.stderr[-4000:])
    assert "exhausted" not in r.stderr, r.stderr[-4000:]


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_a_cached_engine_changes_element_type(emu, pad):
    u16, f32, k1, k2, w, psi0 = inputs(ODD)
    emu.l.mvn_release_cached_engines()
    try:
        ref, _ = call(emu, 0, psi0.copy(), u16, w, k1, k2, pad=pad)
        hits0 = emu.psf_cache_counters()[0]
        a, da = call(emu, 1, psi0.copy(), u16, w, k1, k2, pad=pad)   # uint16, on the engine mode 0 left
        b, db = call(emu, 1, psi0.copy(), f32, w, k1, k2, pad=pad)   # the same views as float32
        c, dc = call(emu, 1, psi0.copy(), u16, w, k1, k2, pad=pad)   # uint16 again
        m, dm = call(emu, 1, psi0.copy(), [u16[0], f32[1], f32[2], u16[3]], w, k1, k2, pad=pad)
        # the engine was re-used every time: its PSF forms stayed
        assert emu.psf_cache_counters()[0] - hits0 == 4 * 2 * V
    finally:
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    for got in (a, b, c, m):
        assert np.array_equal(got, ref)
    ing = 0 if pad == "none" else 1
    assert da == dc == (ITERS * V, ing * V) and db == (0, 0) and dm == (ITERS * 2, ing * 2), (da, db, dc, dm)


def test_a_streamed_ring_follows_the_element_type(emu):
    u16, f32, k1, k2, w, psi0 = inputs(ODD)
    emu.l.mvn_release_cached_engines()
    try:
        ref, _ = call(emu, 0, psi0.copy(), u16, w, k1, k2, pad="zero")
        emu.l.mvn_release_cached_engines()
        emu.set_memory_mode("stream")
        a, da = call(emu, 1, psi0.copy(), u16, w, k1, k2, pad="zero")  # a uint16 ring
        b, db = call(emu, 1, psi0.copy(), f32, w, k1, k2, pad="zero")  # float32 streams through it: rebuilt
        c, dc = call(emu, 1, psi0.copy(), u16, w, k1, k2, pad="zero")
    finally:
        emu.set_memory_mode(None)
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    for got in (a, b, c):
        assert np.array_equal(got, ref)
    assert da == dc == (ITERS * V, ITERS * V) and db == (0, 0), (da, db, dc)


def test_refusals(emu):
    u16, f32, k1, k2, w, psi0 = inputs(EVEN)
    assert emu.l.mvn_set_image_storage(2) < 0 and emu.l.mvn_set_image_storage(-1) < 0
    assert "image storage" in emu.l.mvn_last_error().decode()
    assert emu.get_image_storage() == 0
    hook = lambda spectrum, view, conv: None  # noqa: E731
    try:
        emu.set_image_storage(1)
        assert emu.get_image_storage() == 1
        e = emu.engine(EVEN, 1)
        try:
            e.set_view(0, u16[0], w[0], k1[0], k2[0])
            with pytest.raises(native.MvnError, match="uint16 image"):
                e.set_halo_hook(hook)
            e.set_view(0, f32[0], w[0], k1[0], k2[0])  # float32 in the slot again: the hook is accepted
            e.set_halo_hook(hook)
            e.set_halo_hook(None)
        finally:
            e.close()
        # the hook first: the image stays float32 and the divide counter stands still
        e = emu.engine(EVEN, 1)
        try:
            c0 = emu.image_storage_counters()
            e.set_halo_hook(hook)
            e.set_view(0, u16[0], w[0], k1[0], k2[0])
            e.set_halo_hook(None)
            e.set_psi(psi0)
            e.iterate(1, LAM, MINV)
            assert emu.image_storage_counters() == c0
        finally:
            e.close()
    finally:
        emu.set_image_storage(0)


def test_mode_0_after_mode_1_has_been_used(emu):
    u16, _, k1, k2, w, psi0 = inputs(EVEN)
    try:
        got1, d1 = call(emu, 1, psi0.copy(), u16, w, k1, k2, pad="zero")
        got0, d0 = call(emu, 0, psi0.copy(), u16, w, k1, k2, pad="zero")  # on the engine mode 1 left
    finally:
        emu.set_image_storage(0)
        emu.l.mvn_release_cached_engines()
    assert d1 == (ITERS * V, V) and d0 == (0, 0)
    assert np.array_equal(got0, got1)


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.asan
def test_stand_alone_program_under_sanitizers():
    """tools/image_storage_standalone.cpp: a C++ main on the emulation, both under AddressSanitizer + UBSan (csrc/Makefile,
    target image-storage-asan).  Nothing is preloaded and nothing is loaded into Python."""
    if not (_runtime("libasan.so") and _runtime("libubsan.so")):
        pytest.skip("no libasan / libubsan next to gcc")
    subprocess.check_call(["make", "-C", CSRC, "image-storage-asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "libmultiviewnative_amd", "lib", "image_storage_standalone")
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), tail
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
    assert r.stdout.count("equal") == 10, tail
