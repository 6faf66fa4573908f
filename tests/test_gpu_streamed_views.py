"""Out-of-core views on the MI355X (memory modes of inplace_gpu_deconvolve, csrc/mvn_abi.cpp): a streamed view's
image and weights cross PCIe into a ring of device slots on the upload stream while the compute stream works on the
other views.  Every streamed result must equal the resident one bit for bit - a slot read before its upload has landed,
or overwritten while a view update still reads it, changes psi, because every view differs.  Budgets come from
mvn_deconvolve_memory; modes and budgets are restored whatever happens."""
import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import realistic_views

pytestmark = pytest.mark.gpu

MAX_REL = 1e-4  # the suite's float32 tolerance against the CPU oracle (tests/test_gpu_parity.py)
RMS_REL = 1e-5


@pytest.fixture(scope="module")
def gpu():
    import os
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    return b


def rel_err(got, ref):
    d = got.astype(np.float64) - ref.astype(np.float64)
    return (np.abs(d).max() / max(np.abs(ref).max(), 1e-30),
            np.sqrt(np.mean(d * d)) / max(np.sqrt(np.mean(ref.astype(np.float64) ** 2)), 1e-30))


def _call(gpu, h, psi0, mode, budget=None, pad="none"):
    """one blocking call in `mode` under `budget` (bytes); returns psi and the change of mvn_stream_counters"""
    gpu.set_memory_mode(mode)
    gpu.set_memory_budget(budget)
    try:
        before = gpu.stream_counters()
        got = gpu.gpu_deconvolve(psi0, h, pad_mode=pad)
        # (a failed call leaves psi untouched; mvn_last_error keeps the last failure of ANY earlier call)
        assert not np.array_equal(got, psi0), (mode, gpu.l.mvn_last_error().decode())
        return got, [b - a for a, b in zip(before, gpu.stream_counters())]
    finally:
        gpu.set_memory_budget(None)
        gpu.set_memory_mode(None)


def _memory(gpu, h, s, pad):
    before = gpu.get_pad_mode()
    gpu.set_pad_mode(pad)
    try:
        return gpu.deconvolve_memory(h, s)
    finally:
        gpu.set_pad_mode(before)


@pytest.mark.parametrize("pad", ["none", "zero"])
@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_every_streamed_count_and_ring_is_bit_equal_to_resident(gpu, pad, lam):
    shape, V, iters = (64, 64, 128), 4, 3
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (7, 5, 5), seed=71)
    h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, iters)
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        ref, d = _call(gpu, h, psi0, "resident", pad=pad)
        assert d == [0, 0, 0]
        pair = _memory(gpu, h, 1, pad) - _memory(gpu, h, 0, pad)  # one ring slot: an image + weights pair
        host_bytes = 2 * views[0].nbytes
        for s in range(1, V + 1):
            need = _memory(gpu, h, s, pad)  # ring of 2
            for ring, budget in ((2, need), (1, need - pair)):
                got, d = _call(gpu, h, psi0, "stream:%d" % s, budget=budget, pad=pad)
                assert d == [1, s * iters, s * iters * host_bytes], (s, ring, d)
                assert np.array_equal(got, ref), (s, ring, float(np.abs(got - ref).max()))
        # auto under a budget the resident call does not fit in: it streams, and still agrees
        got, d = _call(gpu, h, psi0, "auto", budget=_memory(gpu, h, 0, pad) - 1, pad=pad)
        assert d[0] == 1 and d[1] >= 2 * iters and np.array_equal(got, ref), d
        # auto with room for everything: resident
        got, d = _call(gpu, h, psi0, "auto", pad=pad)
        assert d == [0, 0, 0] and np.array_equal(got, ref)
    finally:
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_fused_middle_pass_runs_streamed(gpu, monkeypatch):
    # 512 x 512 planes with (31, 7, 5) PSFs: the sequential sweep takes the fused middle pass (mvn_mid_fused.hpp)
    # whose taps stay resident while the views' stacks stream
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    shape, V, iters = (64, 512, 512), 3, 3
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (31, 7, 5), seed=61)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, iters)
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        c0 = gpu.l.mvn_mid_fused_launch_count()
        ref, _ = _call(gpu, h, psi0, "resident")
        assert gpu.l.mvn_mid_fused_launch_count() - c0 == iters * V * 2
        for mode in ("stream", "stream:1"):
            c0 = gpu.l.mvn_mid_fused_launch_count()
            got, d = _call(gpu, h, psi0, mode)
            assert gpu.l.mvn_mid_fused_launch_count() - c0 == iters * V * 2
            assert d[0] == 1 and d[1] == iters * (V if mode == "stream" else 1), (mode, d)
            assert np.array_equal(got, ref), mode
    finally:
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_full_size_512_six_views_two_streamed(gpu):
    from oracle import binding as orc
    from ref_fixtures import structured_views
    shape, V, iters = (512, 512, 512), 6, 2
    views, k1, k2, w, psi0 = structured_views(shape, V, (31, 31, 31))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, iters)
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        ref, _ = _call(gpu, h, psi0, "resident")
        gpu.check(gpu.l.mvn_release_cached_engines())
        got, d = _call(gpu, h, psi0, "stream:2", budget=_memory(gpu, h, 2, "none"))
        assert d == [1, 2 * iters, 2 * iters * 2 * views[0].nbytes], d
        assert np.array_equal(got, ref)
    finally:
        gpu.check(gpu.l.mvn_release_cached_engines())
    o = orc.cpu_deconvolve(psi0, h, -1)
    mx, rms = rel_err(got, o)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


def test_submit_wait_streamed_blocks(gpu):
    shape, V = (48, 64, 96), 3
    blocks = []
    for b in range(3):
        _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=80 + b)
        blocks.append((WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3), psi0))
    refs = [_call(gpu, h, psi0, "resident")[0] for h, psi0 in blocks]
    gpu.set_pad_mode("none")
    gpu.set_memory_mode("auto")
    gpu.set_memory_budget(gpu.deconvolve_memory(blocks[0][0], 0) - 1)
    try:
        before = gpu.stream_counters()
        outs = [psi0.copy() for _, psi0 in blocks]
        tickets = [gpu.deconvolve_submit(o, h) for o, (h, _) in zip(outs, blocks)]
        for t in tickets:
            gpu.deconvolve_wait(t)
        d = [b - a for a, b in zip(before, gpu.stream_counters())]
    finally:
        gpu.set_memory_budget(None)
        gpu.set_memory_mode(None)
        gpu.set_pad_mode(None)
        gpu.check(gpu.l.mvn_release_cached_engines())
    assert d[0] == 3, d
    for o, r in zip(outs, refs):
        assert np.array_equal(o, r)
