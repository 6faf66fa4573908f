"""CPU-only validation of the product's plans, index math and RL driver through the test-only
host emulation of its device backend (lib/libmvn_emu.so runs the very same workgroup bodies on
the CPU).  The -m gpu tests repeat the same comparisons on the real kernels."""
import os
import subprocess

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import Fixture3D, GOLDEN_SUMS, realistic_views, synthetic_views
from nonfinite_util import nonfinite_cases

CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    return native.Binding(native.EMU_SO)


# the suite's pin of the direct dim0 leg (tests/conftest.py) and the product's defaults: see tests/test_gpu_parity.py
@pytest.fixture(params=["suite pin", "product defaults"])
def leg(request, emu, monkeypatch):
    if request.param == "product defaults":
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    emu.l.mvn_release_cached_engines()
    yield request.param
    emu.l.mvn_release_cached_engines()


SHAPES = [(8, 8, 8), (4, 6, 10), (13, 17, 19), (16, 18, 14), (6, 10, 15), (32, 20, 64), (3, 5, 2),
          (12, 7, 9), (1, 1, 4), (2, 3, 1), (24, 40, 22), (64, 64, 64), (5, 4, 46)]


# shapes that take the compile-time specialised kernels (mvn_fixed.hpp): (fx_rows, fx_ax1, fx_ax0)
FIXED_SHAPES = {(64, 64, 64): (1, 1, 1), (64, 128, 256): (1, 1, 1), (128, 64, 512): (1, 1, 1),
                (256, 64, 64): (1, 1, 1), (64, 512, 64): (1, 1, 1), (1024, 64, 32): (0, 1, 1),
                (64, 64, 1024): (1, 1, 1), (8, 64, 2048): (1, 1, 0), (16, 1024, 64): (1, 1, 0),
                (32, 20, 64): (1, 0, 0)}


@pytest.mark.parametrize("shape", sorted(FIXED_SHAPES))
def test_fixed_kernels_roundtrip_and_forward(emu, shape):
    info = emu.plan_describe(shape)
    assert (info["fx_rows"], info["fx_ax1"], info["fx_ax0"]) == FIXED_SHAPES[shape]
    rng = np.random.default_rng(9)
    x = rng.standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = emu.rfft3(x)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6
    back = emu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 1e-5


# mixed-radix (2^a 3^b 5^c) lengths served by the compile-time kernels: (fx_rows, fx_ax1, fx_ax0)
MIXED_FIXED_SHAPES = {(96, 160, 288): (1, 1, 1), (288, 96, 160): (1, 1, 1), (160, 288, 96): (1, 1, 1),
                      (64, 192, 384): (1, 1, 1), (320, 64, 640): (1, 1, 1), (64, 576, 192): (1, 1, 1),
                      (2, 1920, 1920): (1, 1, 0), (1280, 16, 64): (1, 0, 1), (960, 16, 576): (1, 0, 1),
                      (768, 16, 960): (1, 0, 1), (640, 384, 64): (1, 1, 1), (16, 64, 1536): (1, 1, 0),
                      (16, 64, 1280): (1, 1, 0)}


@pytest.mark.parametrize("shape", sorted(MIXED_FIXED_SHAPES))
def test_mixed_radix_fixed_kernels(emu, shape):
    info = emu.plan_describe(shape)
    assert (info["fx_rows"], info["fx_ax1"], info["fx_ax0"]) == MIXED_FIXED_SHAPES[shape]
    rng = np.random.default_rng(10)
    x = rng.standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = emu.rfft3(x)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6
    back = emu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5


def test_mixed_radix_fixed_deconvolve_vs_oracle(emu):
    shape = (64, 192, 320)
    assert emu.plan_describe(shape)["fx_rows"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 7, 9))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    got = emu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 8)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


# every last-axis length of the walking (row-major tile) kernels through the fused c2r + pointwise + r2c passes
WALKING_D2 = [96, 160, 288, 320, 384, 576, 640, 768, 960, 1280, 1536, 1920, 2048]


@pytest.mark.parametrize("d2", WALKING_D2)
def test_walking_rows_kernels_deconvolve_vs_oracle(emu, d2):
    shape = (4, 16, d2)
    assert emu.plan_describe(shape)["fx_rows"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (3, 3, 5))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    got = emu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 4)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    assert np.sqrt(np.mean((got - ref) ** 2)) <= 1e-5 * np.sqrt(np.mean(ref ** 2))


def test_direct_dim0_halo_mode_on_one_rank(emu, monkeypatch):
    # HaloSlabDriver with a cyclic self-exchange: the engine hook before every dim0 leg, plane copies in and out of
    # the halo planes, on the extended slab - against the sequential oracle on the plain volume
    from libmultiviewnative_amd.sharded import HaloSlabDriver
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")
    shape, V, ks = (24, 16, 32), 2, (7, 3, 5)
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    ref = orc.cpu_deconvolve(psi0, h, 4)
    drv = HaloSlabDriver(emu, shape, V, ks[0])
    try:
        for v in range(V):
            drv.set_view(v, views[v], w[v], k1[v], k2[v])
        drv.set_psi(psi0)
        drv.run(3, 0.006, 1e-4)
        got = drv.get_psi()
    finally:
        drv.close()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    # a PSF deeper than the direct leg takes cannot run in this mode: refused, not computed wrongly
    _, views, k1, k2, w, psi0 = realistic_views((80, 8, 16), 1, (35, 3, 3))
    drv = HaloSlabDriver(emu, (80, 8, 16), 1, 35)
    try:
        with pytest.raises(ValueError):  # when the PSF is handed over, not in the middle of a sweep
            drv.set_view(0, views[0], w[0], k1[0], k2[0])
    finally:
        drv.close()


def test_packed_nyquist_layout_is_not_used_beyond_its_dim0_limit(emu, monkeypatch):
    # a DC-pair workgroup of the packed layout keeps two dim0 columns in 64 KB of LDS: volumes with more than
    # ~4000 planes keep the separate Nyquist plane (the launch would be refused), forced or not
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")
    shape = (4096, 4, 8)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 1, (3, 3, 3))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    ref = orc.cpu_deconvolve(psi0, h, 4)
    for forced in (None, "1"):
        if forced:
            monkeypatch.setenv("MVN_NYQ_PACKED", forced)
        emu.set_pad_mode("none")
        try:
            got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
        finally:
            emu.set_pad_mode(None)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


def test_fixed_kernels_deconvolve_vs_oracle(emu, leg):
    shape = (64, 64, 128)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 7, 9))
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 2)
        got = emu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
        assert np.sqrt(np.mean((got - ref) ** 2)) <= 1e-5 * np.sqrt(np.mean(ref ** 2))


def test_fused_pipeline_invariants(emu):
    # the 8-pass pipeline (c2r+divide+r2c and c2r+update+r2c fused) keeps the loop invariants:
    # N iterations == N x 1 iteration bit for bit, and the last pass leaves psi complete
    shape = (32, 32, 64)
    assert emu.plan_describe(shape)["fx_rows"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, 3, (5, 5, 5))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    three = emu.gpu_deconvolve(psi0, h)
    h.with_iterations(1)
    one = psi0
    for _ in range(3):
        one = emu.gpu_deconvolve(one, h)
    assert np.array_equal(one, three)
    h.with_iterations(3)
    ref = orc.cpu_deconvolve(psi0, h, 4)
    assert np.abs(three - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_vs_pocketfft(emu, shape):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = emu.rfft3(x)
    assert np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30) < 5e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_vs_pocketfft(emu, shape):
    rng = np.random.default_rng(8)
    x = rng.standard_normal(shape)
    spec = np.fft.rfftn(x).astype(np.complex64)
    ref = np.fft.irfftn(spec.astype(np.complex128), s=shape, axes=(0, 1, 2)) * np.prod(shape)
    got = emu.irfft3(spec, shape[2])
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6


# lengths with a prime factor > 31 take the chirp-z (Bluestein) route inside the same passes
BLUESTEIN_SHAPES = [(37, 41, 74), (4, 271, 6), (271, 4, 8), (6, 5, 542), (67, 8, 134), (3, 3, 37)]


@pytest.mark.parametrize("shape", BLUESTEIN_SHAPES)
def test_bluestein_axes(emu, shape):
    rng = np.random.default_rng(12)
    x = rng.standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = emu.rfft3(x)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-5
    back = emu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 5e-5


def test_bluestein_deconvolve_vs_oracle(emu):
    shape = (37, 12, 74)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 3, 7))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    got = emu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 4)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


def test_ramp_roundtrip_exact(emu):
    # tests/test_plan_store.cu (GPU twin of test_plan_store.cpp:83-142)
    x = np.arange(512, dtype=np.float32).reshape(8, 8, 8)
    back = emu.irfft3(emu.rfft3(x), 8) / np.float32(512)
    assert np.array_equal(back, x)


def test_plan_store_semantics(emu):
    l = emu.l
    emu.check(l.mvn_plan_store_clear())
    assert l.mvn_plan_store_empty() == 1
    d = (native.C.c_int * 3)(8, 8, 8)
    assert l.mvn_plan_store_has_key(0, d) == 0
    emu.check(l.mvn_plan_store_add(0, d))
    assert l.mvn_plan_store_has_key(0, d) == 1 and l.mvn_plan_store_size() == 1
    emu.check(l.mvn_plan_store_add(0, d))
    assert l.mvn_plan_store_size() == 1
    info = emu.plan_describe((8, 8, 8))
    assert info["h"] == 4 and info["C"] == 4 and info["RP"] == 8 and info["even"] == 1


@pytest.mark.parametrize("name", ["identity", "horizont", "vertical", "depth", "all1"])
def test_convolution_fixture_sums(emu, name, leg):
    fx = Fixture3D()
    out = emu.gpu_convolution(fx.padded_image, getattr(fx, name))
    got = float(out[fx.interior].astype(np.float64).sum())
    assert abs(got - GOLDEN_SUMS[name]) / GOLDEN_SUMS[name] < 1e-6
    ref = orc.cpu_convolution(fx.padded_image, getattr(fx, name))
    assert np.abs(out - ref).max() <= 2e-6 * np.abs(ref).max()


@pytest.mark.parametrize("shape,kshape", [((16, 18, 14), (3, 3, 3)), ((13, 17, 19), (5, 3, 7)),
                                          ((20, 12, 9), (4, 3, 2)), ((8, 8, 8), (8, 8, 8))])
def test_convolution_vs_oracle(emu, shape, kshape):
    rng = np.random.default_rng(5)
    im = rng.uniform(0, 10, shape).astype(np.float32)
    k = rng.uniform(0, 1, kshape).astype(np.float32)
    got = emu.gpu_convolution(im, k)
    ref = orc.cpu_convolution(im, k)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 3e-6
    assert np.array_equal(got, emu.gpu_convolution(im, k, legacy=True))


def test_kernel_larger_than_image_is_rejected(emu, capfd):
    im = np.ones((4, 4, 4), np.float32)
    out = emu.gpu_convolution(im, np.ones((5, 3, 3), np.float32))
    assert np.array_equal(out, im)  # failure leaves the buffer untouched
    assert "kernel extent" in capfd.readouterr().err


@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("shape,kshape,nv", [((16, 20, 18), (5, 5, 5), 3), ((13, 17, 19), (3, 5, 3), 2),
                                             ((8, 12, 10), (3, 3, 3), 1)])
def test_deconvolve_vs_oracle(emu, shape, kshape, nv, lam, leg):
    _, views, k1, k2, w, psi0 = realistic_views(shape, nv, kshape)
    h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
    got = emu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 2)
    # stated float32 tolerance: max|d| <= 1e-4 max|psi|, rms <= 1e-5 rms
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    assert np.sqrt(np.mean((got - ref) ** 2)) <= 1e-5 * np.sqrt(np.mean(ref ** 2))


def test_deconvolve_closed_form_and_loop_invariants(emu, leg):
    shape = (16, 16, 16)
    views, k1, k2, w = synthetic_views(shape, 6, 3, 5)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 2)
    psi0 = np.full(shape, 3.0, np.float32)
    psi = emu.gpu_deconvolve(psi0, h)
    assert np.abs(psi - 37.72946).max() < 2e-4 * 37.72946
    h.with_iterations(0)
    assert np.array_equal(emu.gpu_deconvolve(psi0, h), psi0)
    h.with_iterations(1)
    two = emu.gpu_deconvolve(emu.gpu_deconvolve(psi0, h), h)
    assert np.array_equal(two, psi)  # N iterations == N x 1 iteration


def test_zero_psi_recovers(emu, leg):
    shape = (8, 8, 8)
    views, k1, k2, w = synthetic_views(shape, 1, 3, 3)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 1)
    psi = emu.gpu_deconvolve(np.zeros(shape, np.float32), h)
    assert np.array_equal(psi, orc.cpu_deconvolve(np.zeros(shape, np.float32), h, 1))


def test_mismatched_views_leave_psi_untouched(emu, capfd):
    views, k1, k2, w = synthetic_views((8, 8, 8), 2, 3, 3)
    views[1] = np.ones((8, 8, 4), np.float32)
    w[1] = np.ones((8, 8, 4), np.float32)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 1)
    psi0 = np.full((8, 8, 8), 2.0, np.float32)
    assert np.array_equal(emu.gpu_deconvolve(psi0, h), psi0)
    assert "share image_dims_" in capfd.readouterr().err


@pytest.mark.parametrize("shape", [(12, 10, 14), (64, 64, 64)])
def test_engine_simultaneous_mode(emu, shape, leg):
    _, views, k1, k2, w, psi0 = realistic_views(shape, 3, (3, 3, 3))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    eng = emu.engine(shape, 3)
    for v in range(3):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    for _ in range(2):
        eng.compute_delta(0.006, 1e-4)
        eng.apply_delta()
    eng.sync()
    got = eng.get_psi()
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 2)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    eng.close()


def test_psf_buffers_replaced_on_a_live_engine_equal_fresh_engines(emu, monkeypatch):
    """tests/psf_replace_case.py: taps of 16 planes -> 32 planes -> 3-D spectrum -> taps again on ONE engine, psi after
    every stage bit for bit that of a fresh engine given only that stage's kernels (tests/test_gpu_scoped.py runs the
    same body on the device)."""
    import psf_replace_case
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    psf_replace_case.run(emu)


def test_pointwise_entry_points(emu):
    rng = np.random.default_rng(0)
    n = 1000
    view = rng.uniform(0, 5, n).astype(np.float32)
    blurred = rng.uniform(-1, 5, n).astype(np.float32)
    blurred[:3] = [0, np.nan, np.inf]
    a, b = emu.compute_quotient(view, blurred), orc.compute_quotient(view, blurred)
    assert np.array_equal(a, b, equal_nan=True)
    psi = rng.uniform(0.5, 10, n).astype(np.float32)
    integral = rng.uniform(-0.1, 1, n).astype(np.float32)
    integral[:3] = [np.nan, np.inf, -np.inf]
    w = rng.uniform(0, 1, n).astype(np.float32)
    for lam in (0.0, 0.006):
        assert np.array_equal(emu.compute_final_values(psi, integral, w, 1e-4, lam),
                              orc.final_values(psi, integral, w, 1e-4, lam))


def _zero_padd_reference(orc, psi0, views, k1, k2, w, lam, minv, its):
    """The reference GPU entry's zero_padd policy applied by hand (inc/padd_utils.h:121-138,
    src/gpu_deconvolve_methods.cuh:366-449,537-549), run through the CPU oracle."""
    dims = psi0.shape
    kmax = [max(max(a.shape[d], b.shape[d]) for a, b in zip(k1, k2)) for d in range(3)]
    ext = tuple(dims[d] + kmax[d] - 1 for d in range(3))
    off = tuple((kmax[d] - 1) // 2 for d in range(3))
    sl = tuple(slice(off[d], off[d] + dims[d]) for d in range(3))

    def embed(x):
        out = np.zeros(ext, np.float32)
        out[sl] = x
        return out

    h = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], lam, minv, its)
    return orc.cpu_deconvolve(embed(psi0), h, 4)[sl]


def test_zero_padd_mode_matches_reference_gpu_policy(emu, monkeypatch, leg):
    shape = (20, 16, 24)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 3, 7))
    k2[1] = k2[1][:3]  # kernels of different extents: the policy takes the maxima
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    cyclic = emu.gpu_deconvolve(psi0, h)  # pad_mode="none", the CPU path's policy
    padded = emu.gpu_deconvolve(psi0, h, pad_mode="zero_exact")  # exactly image + kernel - 1
    ref = _zero_padd_reference(orc, psi0, views, k1, k2, w, 0.006, 1e-4, 3)
    assert np.abs(padded - ref).max() <= 1e-4 * np.abs(ref).max()
    assert np.abs(padded - cyclic).max() > 1e-3 * np.abs(ref).max()  # the two policies do differ
    # the same selection through the environment (what round 1 offered), the setter left alone
    monkeypatch.setenv("MVN_PAD_MODE", "zero_exact")
    assert np.array_equal(emu.gpu_deconvolve(psi0, h, pad_mode=False), padded)
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    assert np.array_equal(emu.gpu_deconvolve(psi0, h, pad_mode=False), cyclic)
    monkeypatch.delenv("MVN_PAD_MODE")


def test_zero_padd_good_size_mode(emu, monkeypatch, leg):
    # The library's DEFAULT policy (the reference GPU entry's zero_padd, src/multiviewnative.cu:
    # 26-27,128) with FFT-friendly padded extents: they grow to 2^a 3^b 5^c 7^d (here 19+5-1=23 -> 24,
    # 13+3-1=15, 17+7-1=23 -> 24) and the quotient is guarded where the view is exactly 0.
    # Delta PSFs make the blurred estimate EXACTLY 0 in the border: without the guard -> NaN.
    shape = (19, 13, 17)
    views, k1, k2, w = synthetic_views(shape, 2, 5, 7)
    k1 = [k[:, 1:4, :] for k in k1]
    k2 = [k[1:6, 2:5, :] for k in k2]
    k1 = [np.ascontiguousarray(k) for k in k1]
    k2 = [np.ascontiguousarray(k) for k in k2]
    psi0 = np.full(shape, 3.0, np.float32)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 2)
    monkeypatch.delenv("MVN_PAD_MODE", raising=False)
    monkeypatch.delenv("MVN_PAD_GOOD_SIZE", raising=False)
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)  # no setter, no environment: the default
    assert np.array_equal(got, emu.gpu_deconvolve(psi0, h, pad_mode="zero"))
    assert np.isfinite(got).all()
    # oracle on hand-padded stacks of the same good size, same guard
    ext, off = (24, 15, 24), (2, 1, 3)
    sl = tuple(slice(o, o + s) for o, s in zip(off, shape))

    def embed(x):
        out = np.zeros(ext, np.float32)
        out[sl] = x
        return out

    hp = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], 0.006, 1e-3, 2)
    orc.set_quotient_guard(True)
    try:
        ref = orc.cpu_deconvolve(embed(psi0), hp, 2)[sl]
    finally:
        orc.set_quotient_guard(False)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    # the closed form of the synthetic data holds in the interior (constant views, delta PSFs)
    assert abs(float(got[9, 6, 8]) - 30.0 * (np.sqrt(1 + 2 * 0.006 * 30.0) - 1) / (0.006 * 30.0)) < 1e-2


@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_golden_rl_small(emu, lam, leg):
    from golden_util import rl_small
    psi0, h, seq, _ = rl_small(lam)
    got = emu.gpu_deconvolve(psi0, h)
    assert np.abs(got - seq).max() <= 1e-4 * np.abs(seq).max()


def test_deconvolve_staging_error_leaves_psi_untouched(emu, capfd):
    # the PSF of the second view is larger than the stack: the uploader thread fails while the main
    # thread already iterates on view 0 -- the call must come back cleanly with psi untouched
    shape = (8, 8, 8)
    views, k1, k2, w = synthetic_views(shape, 2, 3, 3)
    k1[1] = np.ones((9, 3, 3), np.float32)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 2)
    psi0 = np.full(shape, 2.0, np.float32)
    assert np.array_equal(emu.gpu_deconvolve(psi0, h), psi0)
    assert "kernel extent" in capfd.readouterr().err


def _legacy_case(seed, shape, kshape):
    rng = np.random.default_rng(seed)
    image = rng.uniform(1, 20, shape).astype(np.float32)
    kernel = rng.uniform(0, 1, kshape).astype(np.float32)
    kernel /= kernel.sum()
    return image, kernel


@pytest.mark.parametrize("shape,kshape", [((16, 16, 16), (3, 3, 3)), ((12, 10, 9), (5, 3, 3))])
def test_iterate_fft_legacy_steps(emu, shape, kshape):
    # src/multiviewnative.cu:395-600: one RL step with kernel2 = 0.1, weights = 1
    image, kernel = _legacy_case(3, shape, kshape)
    got = emu.iterate_fft(image, kernel)
    ref = orc.iterate_fft(image, kernel)
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    for lam in (0.006, 0.5):
        got = emu.iterate_fft(image, kernel, 1e-3, lam)
        ref = orc.iterate_fft(image, kernel, 1e-3, lam)
        assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    # an integral of 0.1 * sum(quotient) is far above minValue: the legacy blend returns t itself
    integral = orc.cpu_convolution(orc.compute_quotient(image, orc.cpu_convolution(image, kernel)),
                                   np.full_like(kernel, .1))
    lf = np.float32(0.006)
    t = ((np.sqrt(1.0 + 2.0 * np.float64(lf) * (image * integral).astype(np.float64)) - 1.0)
         / np.float64(lf)).astype(np.float32)
    got = emu.iterate_fft(image, kernel, 1e-3, 0.006)
    assert np.abs(got - t).max() <= 2e-6 * np.abs(t).max()


def test_batched_forward_matches_single_and_numpy(emu):
    # bench/bench_gpu_many_nd_fft.cu:403-463: V stacks of one shape through one plan
    rng = np.random.default_rng(11)
    for shape in ((8, 12, 10), (16, 16, 18), (5, 6, 7)):
        stacks = rng.standard_normal((3,) + shape).astype(np.float32)
        many = emu.rfft3_many(stacks)
        assert many.shape == (3,) + shape[:2] + (shape[2] // 2 + 1,)
        for b in range(3):
            assert np.array_equal(many[b], emu.rfft3(stacks[b]))
            ref = np.fft.rfftn(stacks[b].astype(np.float64))
            assert np.abs(many[b] - ref).max() <= 2e-5 * np.abs(ref).max()
    assert emu.fft3_many_time((8, 8, 8), 2, 0, 1) >= 0.0


def test_psf_spectra_reused_across_calls(emu):
    # block-after-block calls with the same PSFs re-use the resident spectra;
    # a changed kernel invalidates exactly its own spectrum
    shape = (12, 10, 16)
    rng = np.random.default_rng(5)
    _, views, k1, k2, w, _ = realistic_views(shape, 2, (5, 5, 5), seed=9)
    emu.l.mvn_release_cached_engines()

    def run(vs, a, b):
        h = WorkspaceHolder(vs, a, b, w, lambda_=0.006, min_value=1e-4, iterations=2)
        psi0 = np.full(shape, np.float32(vs[0].mean()), np.float32)
        got = emu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 2)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()

    h0, m0 = emu.psf_cache_counters()
    run(views, k1, k2)
    h1, m1 = emu.psf_cache_counters()
    assert (h1 - h0, m1 - m0) == (0, 4)
    other = [(v * rng.uniform(0.5, 1.5, shape)).astype(np.float32) for v in views]
    run(other, k1, k2)  # new stacks, same PSFs: every spectrum re-used
    h2, m2 = emu.psf_cache_counters()
    assert (h2 - h1, m2 - m1) == (4, 0)
    k1b = [k.copy() for k in k1]
    k1b[1][0, 0, 0] += np.float32(1e-3)
    run(other, k1b, k2)  # one kernel differs in one tap: prepared again, the other three re-used
    h3, m3 = emu.psf_cache_counters()
    assert (h3 - h2, m3 - m2) == (3, 1)
    emu.l.mvn_release_cached_engines()


def _slab_ranks_in_one_process(emu, shape, V, P, its=2):
    """P slab engines in this process; the all-to-all exchanges are done by hand on their
    (host-emulation) buffers: block j of rank i's send buffer -> block i of rank j's receive buffer."""
    import ctypes as C
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (3, 3, 3), seed=31)
    zs = [r * shape[0] // P for r in range(P + 1)]
    engs = [emu.slab_engine(shape, P, r, V) for r in range(P)]
    for r, e in enumerate(engs):
        for v in range(V):
            e.set_view(v, views[v][zs[r]:zs[r + 1]], w[v][zs[r]:zs[r + 1]], k1[v], k2[v])
        e.set_psi(psi0[zs[r]:zs[r + 1]])
    nm, nn = engs[0].buffer_sizes()

    def arr(ptr, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n,)) if n else None

    bufs = []
    for e in engs:
        a, b, an, bn = e.buffers()
        bufs.append((arr(a, nm), arr(b, nm), arr(an, nn), arr(bn, nn)))

    def exchange(src, dst):  # src/dst: index of the buffer in the tuple (0 = A, 1 = B)
        for off, n in ((0, nm), (2, nn)):
            if not n:
                continue
            blk = n // P
            for i in range(P):
                for j in range(P):
                    bufs[j][dst + off][i * blk:(i + 1) * blk] = bufs[i][src + off][j * blk:(j + 1) * blk]

    for it in range(its):
        for v in range(V):
            last = it == its - 1 and v == V - 1
            for conv in (0, 1):
                for e in engs:
                    e.pack(v, conv)
                exchange(0, 1)
                for e in engs:
                    e.mid(v, conv)
                exchange(1, 0)
                for e in engs:
                    e.unpack(v, conv, 0.006, 1e-4, not last)
    got = np.concatenate([e.get_psi() for e in engs], axis=0)
    for e in engs:
        e.close()
    one = emu.engine(shape, V)
    for v in range(V):
        one.set_view(v, views[v], w[v], k1[v], k2[v])
    one.set_psi(psi0)
    one.iterate(its, 0.006, 1e-4)
    one.sync()
    ref = one.get_psi()
    one.close()
    return got, ref


@pytest.mark.parametrize("shape,V,P", [((8, 12, 16), 2, 2), ((12, 9, 10), 2, 3), ((16, 16, 9), 1, 4),
                                       ((64, 64, 32), 1, 2)])
def test_slab_engines_exchanging_by_hand_equal_the_resident_engine(emu, shape, V, P):
    got, ref = _slab_ranks_in_one_process(emu, shape, V, P)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()


def test_slab_engine_rejects_bad_decompositions(emu, capfd):
    for shape, P in (((9, 12, 16), 2), ((8, 9, 16), 2), ((4, 12, 16), 4)):
        with pytest.raises(native.MvnError):
            emu.slab_engine(shape, P, 0, 1)
    e = emu.slab_engine((8, 12, 16), 2, 1, 1)
    with pytest.raises(native.MvnError):
        e.bind_buffers(e.buffers()[0], None, None, None)  # partial binding
    e.close()
    capfd.readouterr()


# ---- the ABI call's engine cache: several devices, memory heuristic -------------
_CACHE_CHILD = r"""
import os, sys, threading
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views
emu = native.Binding(native.EMU_SO)
mode = sys.argv[2]

def case(shape, V, seed):
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (3, 3, 3), seed=seed)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    return h, psi0, orc.cpu_deconvolve(psi0, h, 1)

if mode == "two_devices":
    # Fiji's one-host-thread-per-device mode: both threads go through the process-wide engine cache
    # (erase + insert on every call, shapes alternate so that engines are also replaced)
    assert emu.l.getNumDevicesCUDA() == 2
    cases = [[case((12, 10, 14), 2, 1), case((8, 12, 10), 1, 2)], [case((10, 8, 12), 2, 3), case((12, 10, 14), 1, 4)]]
    emu.set_pad_mode("none")
    bad = []
    def work(dev):
        for rep in range(12):
            h, psi0, ref = cases[dev][rep % 2]
            got = emu.gpu_deconvolve(psi0, h, device=dev, pad_mode=False)
            if not np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max():
                bad.append((dev, rep))
    ts = [threading.Thread(target=work, args=(d,)) for d in (0, 1)]
    [t.start() for t in ts]; [t.join() for t in ts]
    emu.check(emu.l.mvn_release_cached_engines())
    assert not bad, bad
    print("ok")
elif mode == "memory":
    # total 16 MB; 64^3 x 2 views needs (4*2+2) * 1.08 MB * 1.02 = 11 MB > total / 2
    big = case((64, 64, 64), 2, 5)
    other = case((64, 64, 32), 2, 6)      # 5.6 MB: fits only once the stale engine has been freed
    huge = case((64, 64, 128), 2, 7)      # 21.7 MB: never fits
    emu.set_pad_mode("none")
    for h, psi0, ref in (big, big, other, big):
        got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), "a call that fits was rejected or wrong"
    h, psi0, ref = huge
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert np.array_equal(got, psi0), "psi must be left untouched when the stacks do not fit"
    assert "memory constraints" in emu.l.mvn_last_error().decode()
    h, psi0, ref = big                    # and the library keeps working afterwards
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    print("ok")
"""


def _run_cache_child(mode, env_extra, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="2", **env_extra)
    r = subprocess.run([sys.executable, "-c", _CACHE_CHILD, root, mode], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])
    return r


def test_engine_cache_two_host_threads_two_devices(tmp_path):
    # the cache map is process-wide, calls are serialised per device only: two host threads on two
    # (emulated) devices must not corrupt it (mvn_abi.cpp: engine_cache_mutex)
    _run_cache_child("two_devices", {"MVN_EMU_DEVICES": "2"}, tmp_path)


def test_memory_heuristic_counts_the_cached_engine(tmp_path):
    # src/multiviewnative.cu:94-140 restated: the check must not reject a block of the shape whose
    # engine is already resident, nor count a stale engine that is about to be freed
    r = _run_cache_child("memory", {"MVN_EMU_TOTAL_MB": "16"}, tmp_path)
    assert "memory constraints" in r.stderr


def test_padded_extents_of_common_blocks_have_fixed_kernels(emu):
    # where 64-, 128-, 256- and 512-blocks land with a 31-tap PSF under the default policy: the
    # smallest smooth length, because each of them has compile-time kernels on every axis
    from ref_fixtures import expected_good_extent
    for block, want in ((64, 96), (128, 160), (256, 288), (512, 576)):
        for last in (False, True):
            assert expected_good_extent(emu, block + 31 - 1, last) == want, (block, last)


def test_default_padding_policy_on_a_block(emu, leg):
    # the library default (zero_padd with FFT-friendly extents, stacks embedded / cropped by
    # strided device copies): oracle on hand-padded stacks of the same extents, guard on
    from ref_fixtures import expected_good_extent
    shape = (20, 18, 22)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 5, 5), seed=2)
    k2 = [np.ascontiguousarray(k[1:4, 1:4, 1:4]) for k in k2]
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    emu.l.mvn_release_cached_engines()
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert got.shape == shape and np.isfinite(got).all()
    ext = [expected_good_extent(emu, n + 4, d == 2) for d, n in enumerate(shape)]
    sl = tuple(slice(2, 2 + s) for s in shape)

    def embed(x):
        out = np.zeros(ext, np.float32)
        out[sl] = x
        return out

    hp = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], 0.006, 1e-4, 3)
    orc.set_quotient_guard(True)
    try:
        ref = orc.cpu_deconvolve(embed(psi0), hp, 4)[sl]
    finally:
        orc.set_quotient_guard(False)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), ext
    # a second block of the same shape re-uses the cached (padded) engine; then a dense call of the
    # padded shape itself must not see stale padding state
    again = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert np.array_equal(again, got)
    dense = emu.gpu_deconvolve(embed(psi0), hp, pad_mode="none")[sl]
    orc_dense = orc.cpu_deconvolve(embed(psi0), hp, 4)[sl]
    assert np.abs(dense - orc_dense).max() <= 1e-4 * np.abs(orc_dense).max()
    third = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert np.array_equal(third, got)
    emu.l.mvn_release_cached_engines()


@pytest.mark.parametrize("mask", ["31", "28", "0"])
def test_wave_row_kernels_d2_512(emu, monkeypatch, mask):
    # d2 = 512: the last-axis passes in which a row never leaves its half-wave (mvn_wave_rows.hpp):
    # every pass (mask 31), the product default (28: fused divide, fused update / store, c2r + DELTA), none (the
    # tiled kernels).  The emulation reads the mask at every launch; the HIP backend once per process
    # (tests/test_gpu_parity.py::test_wave_row_variants_in_a_child_process covers it there).
    monkeypatch.setenv("MVN_WAVE_ROWS_MASK", mask)
    shape = (4, 12, 512)  # 48 rows = 24 row pairs: ragged last sweep of the emulation's small grid
    assert emu.plan_describe(shape)["fx_rows"] == 1
    x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = emu.rfft3(x)
    assert np.abs(got - ref).max() <= 5e-6 * np.abs(ref).max()
    back = emu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (3, 5, 7), seed=3)
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
        got = emu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    e = emu.engine(shape, 2)
    for v in range(2):
        e.set_view(v, views[v], w[v], k1[v], k2[v])
    e.set_psi(psi0)
    for _ in range(2):
        e.compute_delta(0.006, 1e-4)
        e.apply_delta()
    got = e.get_psi()
    e.close()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 4)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("shape", [(2, 6, 1920), (3, 4, 2048), (2, 5, 1280), (2, 4, 1536)])
def test_long_rows_small_tile_walking_kernels(emu, shape):
    # rows longer than 1024 floats (H > 512): 2-row tiles, workgroups that walk over the tiles with
    # their tables built once, per-thread loops guarded where the counts do not divide (H = 960:
    # 240 stage-0 butterflies on 256 threads)
    assert emu.plan_describe(shape)["fx_rows"] == 1
    x = np.random.default_rng(2).standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = emu.rfft3(x)
    assert np.abs(got - ref).max() <= 5e-6 * np.abs(ref).max()
    back = emu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (1, 3, 9), seed=4)
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 2)
        got = emu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    e = emu.engine(shape, 2)
    for v in range(2):
        e.set_view(v, views[v], w[v], k1[v], k2[v])
    e.set_psi(psi0)
    e.compute_delta(0.006, 1e-4)
    e.apply_delta()
    got = e.get_psi()
    e.close()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 4)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


def _blocks(shape, n, V, kshape, its):
    out = []
    for b in range(n):
        _, views, k1, k2, w, psi0 = realistic_views(shape, V, kshape, seed=20 + b)
        out.append((WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, its), psi0))
    return out


def test_submit_wait_pipeline_equals_blocking_calls(emu, capfd):
    # mvn_deconvolve_submit / mvn_deconvolve_wait: three blocks in flight on the two engine lanes of a
    # device give, bit for bit, what three blocking inplace_gpu_deconvolve calls give (both policies);
    # tickets are single-use; a failing block reports through its own wait and leaves its psi alone
    shape = (12, 20, 16)
    blocks = _blocks(shape, 3, 2, (3, 5, 3), 3)
    for mode in ("none", "zero"):
        emu.set_pad_mode(mode)
        try:
            want = [emu.gpu_deconvolve(psi0, h, pad_mode=False) for h, psi0 in blocks]
            psis = [np.ascontiguousarray(psi0.copy()) for _, psi0 in blocks]
            tickets = [emu.deconvolve_submit(psi, h) for psi, (h, _) in zip(psis, blocks)]
            assert len(set(tickets)) == 3 and all(t > 0 for t in tickets)
            for t in reversed(tickets):  # any order
                emu.deconvolve_wait(t)
            for got, ref in zip(psis, want):
                assert np.array_equal(got, ref)
        finally:
            emu.set_pad_mode(None)
    with pytest.raises(native.MvnError):
        emu.deconvolve_wait(tickets[0])  # already awaited
    with pytest.raises(native.MvnError):
        emu.deconvolve_wait(12345678)
    # a block whose views disagree in shape fails in ITS wait; the neighbours are unaffected
    h_ok, psi_ok = blocks[0]
    _, views, k1, k2, w, _ = realistic_views(shape, 2, (3, 5, 3), seed=31)
    views[1] = np.ascontiguousarray(views[1][:, :10, :])
    w[1] = np.ascontiguousarray(w[1][:, :10, :])
    bad = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    emu.set_pad_mode("none")
    try:
        a, b = psi_ok.copy(), psi_ok.copy()
        ta = emu.deconvolve_submit(a, h_ok)
        tb = emu.deconvolve_submit(b, bad)
        emu.deconvolve_wait(ta)
        with pytest.raises(native.MvnError, match="share image_dims_"):
            emu.deconvolve_wait(tb)
        assert np.array_equal(b, psi_ok) and np.array_equal(a, emu.gpu_deconvolve(psi_ok, h_ok, pad_mode=False))
    finally:
        emu.set_pad_mode(None)
    capfd.readouterr()
    emu.l.mvn_release_cached_engines()


@pytest.mark.parametrize("k0", [1, 2, 3, 4, 9, 16, 21, 33])
def test_direct_dim0_leg_vs_fft_leg_and_oracle(emu, monkeypatch, k0):
    # mvn_dim0_direct.hpp: the dim0 leg as a direct convolution with the PSF's planes (odd and even
    # depths, the largest instantiated one, a zero tap appended for even depths), with staggered and
    # unstaggered walks, against the fused FFT leg of the same engine and against the oracle;
    # sequential sweep and simultaneous step, lambda 0 and > 0
    shape = (40, 12, 18)  # d0 >= 33 + 4
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (k0, 5, 3), seed=50 + k0)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]  # an asymmetric second kernel of the same depth
    monkeypatch.setenv("MVN_DIM0_DIRECT_MAX", "33")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_PLANE", "0")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")  # (by default the leg is for planes of >= 98304 bins)
    results = {}
    # "direct" / "staggered": Nyquist bins packed into the DC column (opt-in, every kernel is in the direct form);
    # "split": the separate Nyquist plane under the direct leg (the default)
    for tag, env in (("fft", {"MVN_DIM0_DIRECT": "0", "MVN_NYQ_PACKED": "1"}),
                     ("direct", {"MVN_DIM0_DIRECT": "1", "MVN_D0_STAGGER": "0", "MVN_NYQ_PACKED": "1",
                                 "MVN_DIM0_DIRECT_MIN_PLANE": "0", "MVN_DIM0_DIRECT_MIN_ITEMS": "0"}),
                     ("staggered", {"MVN_DIM0_DIRECT": "1", "MVN_D0_STAGGER": "7", "MVN_NYQ_PACKED": "1"}),
                     ("split", {"MVN_DIM0_DIRECT": "1", "MVN_D0_STAGGER": "7", "MVN_NYQ_PACKED": "0"}),
                     # columns cut into pieces (planes with few bins; falls back to the FFT leg where a piece
                     # would be shorter than 2 K + 8 planes)
                     ("pieces", {"MVN_DIM0_DIRECT": "1", "MVN_NYQ_PACKED": "0", "MVN_DIM0_DIRECT_MIN_PLANE": "250"}),
                     ("pieces packed", {"MVN_DIM0_DIRECT": "1", "MVN_NYQ_PACKED": "1", "MVN_DIM0_DIRECT_MIN_PLANE": "250"})):
        for kk, vv in env.items():
            monkeypatch.setenv(kk, vv)
        emu.l.mvn_release_cached_engines()
        for lam in (0.0, 0.006):
            h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
            results[(tag, lam)] = emu.gpu_deconvolve(psi0, h)
        e = emu.engine(shape, 2)
        for v in range(2):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        for _ in range(2):
            e.compute_delta(0.006, 1e-4)
            e.apply_delta()
        results[(tag, "sim")] = e.get_psi()
        e.close()
    emu.l.mvn_release_cached_engines()
    for lam in (0.0, 0.006):
        ref = orc.cpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3), 4)
        for tag in ("fft", "direct", "staggered", "split", "pieces", "pieces packed"):
            assert np.abs(results[(tag, lam)] - ref).max() <= 1e-4 * np.abs(ref).max(), (tag, lam)
        assert np.array_equal(results[("direct", lam)], results[("staggered", lam)])  # same sums, another start plane
    ref = orc.cpu_deconvolve_simultaneous(psi0, WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2), 4)
    for tag in ("fft", "direct", "staggered", "split", "pieces", "pieces packed"):
        assert np.abs(results[(tag, "sim")] - ref).max() <= 1e-4 * np.abs(ref).max(), tag


def test_direct_dim0_leg_limits_and_nonfinite(emu, monkeypatch):
    # too deep a PSF / too shallow a volume fall back to the FFT leg; a non-finite voxel floods the
    # volume exactly as the FFT leg does (the update then clamps everything to minValue)
    monkeypatch.setenv("MVN_DIM0_DIRECT_MAX", "33")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_PLANE", "0")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")
    emu.l.mvn_release_cached_engines()
    for shape, kshape in (((40, 10, 12), (35, 3, 3)), ((12, 10, 12), (9, 3, 3)), ((8, 6, 10), (3, 3, 3))):
        _, views, k1, k2, w, psi0 = realistic_views(shape, 2, kshape, seed=7)
        h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
        got = emu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), shape
    shape = (24, 10, 12)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 1, (5, 3, 3), seed=8)
    views[0][17, 3, 4] = 0.0
    psi_bad = psi0.copy()
    psi_bad[5, 5, 5] = np.inf
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    got = emu.gpu_deconvolve(psi_bad, h)
    ref = orc.cpu_deconvolve(psi_bad, h, 2)
    assert np.array_equal(got, ref, equal_nan=True) and np.isfinite(got).sum() >= got.size - 1  # all clamped; the voxel itself stays NaN
    emu.l.mvn_release_cached_engines()


@pytest.mark.parametrize("env", [{}, {"MVN_NYQ_PACKED": "0"}, {"MVN_DIM0_DIRECT_MIN_PLANE": "250"},
                                 {"MVN_DIM0_DIRECT_MIN_PLANE": "250", "MVN_NYQ_PACKED": "0"}],
                         ids=["product defaults", "split nyquist", "short pieces", "short pieces split"])
def test_nonfinite_voxel_floods_the_volume_in_every_form_of_the_direct_leg(emu, monkeypatch, env):
    # VERDICT r03 weak 1 / ADVICE r03: columns cut into pieces (the product default below 512 x 512 planes), the
    # packed DC-pair workgroups and the Nyquist pieces used to spoil only the pieces that met the value.  Now a
    # work item that meets one reports it (poison word) and the last-axis pass that ends the convolution emits NaN
    # everywhere.  No suite pins here: MVN_DIM0_DIRECT_MIN_* are the product's defaults unless `env` says otherwise.
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    emu.l.mvn_release_cached_engines()
    try:
        # Inf in the middle of a piece: 4 pieces of 48 / 4 of 64 planes under the defaults; 3 pieces of 22 planes
        # (the ADVICE case) with MIN_PLANE = 250
        for shape, kshape, pos in (((192, 16, 32), (5, 3, 3), (100, 5, 5)), ((256, 16, 32), (5, 3, 3), (100, 5, 5)),
                                   ((64, 10, 12), (5, 3, 3), (5, 5, 5))):
            nonfinite_cases(emu, shape, kshape, pos)
    finally:
        emu.l.mvn_release_cached_engines()


def test_default_policy_keeps_dim0_exact_under_the_direct_leg(emu, monkeypatch):
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_PLANE", "0")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")
    # zero_padd with FFT-friendly extents pads dim1 / dim2 to good sizes but leaves dim0 at the reference's exact
    # image + kernel - 1 when every PSF is thin enough for the direct dim0 leg (no transform along dim0) and d1
    # keeps whole last-axis tiles: 20 + 4 - 1 = 23 planes (not 24), 26 + 7 - 1 = 32, 30 + 3 - 1 = 32.  With the
    # direct leg switched off the old rule applies (24 planes).
    from ref_fixtures import expected_good_extent
    shape = (20, 26, 30)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (4, 7, 3), seed=12)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    off = (1, 3, 1)  # (kernel - 1) / 2
    sl = tuple(slice(o, o + s) for o, s in zip(off, shape))

    def reference(ext):
        def embed(x):
            out = np.zeros(ext, np.float32)
            out[sl] = x
            return out
        hp = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], 0.006, 1e-4, 3)
        orc.set_quotient_guard(True)
        try:
            return orc.cpu_deconvolve(embed(psi0), hp, 4)[sl]
        finally:
            orc.set_quotient_guard(False)

    import ctypes

    def has_plan(ext):  # the engine of a call takes its plan from the plan store
        return emu.l.mvn_plan_store_has_key(0, (ctypes.c_int * 3)(*ext)) == 1

    emu.l.mvn_release_cached_engines()
    emu.check(emu.l.mvn_plan_store_clear())
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert expected_good_extent(emu, 32, False) == 32 and expected_good_extent(emu, 32, True) == 32
    assert has_plan((23, 32, 32)) and not has_plan((24, 32, 32))
    exact, rounded = reference((23, 32, 32)), reference((24, 32, 32))
    assert np.abs(got - exact).max() <= 1e-4 * np.abs(exact).max()
    # (the extra plane holds zeros the guarded quotient never lets in: the two paddings agree to rounding)
    assert np.abs(exact - rounded).max() <= 1e-5 * np.abs(exact).max()
    monkeypatch.setenv("MVN_DIM0_DIRECT", "0")
    emu.l.mvn_release_cached_engines()
    emu.check(emu.l.mvn_plan_store_clear())
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert has_plan((24, 32, 32)) and not has_plan((23, 32, 32))
    assert np.abs(got - rounded).max() <= 1e-4 * np.abs(rounded).max()
    emu.l.mvn_release_cached_engines()


def test_engine_has_the_last_word_on_the_exact_dim0_extent(emu, monkeypatch):
    # the padding policy keeps dim0 exact when the static rule says the direct leg applies, but the
    # engine decides per kernel and also wants the tap arrays' plan to be of the volume plan's kernel family.
    # Forced disagreement: the (23, 64, 64) plan enters the plan store built WITHOUT the fixed-length kernels,
    # the engine's own tap plan is built with them -> the engine refuses the direct leg, and the call must then
    # pad dim0 like the other axes (24) instead of sending 23 planes through the FFT leg.
    import ctypes
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_PLANE", "0")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")
    shape = (20, 58, 58)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (4, 7, 7), seed=13)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    off = (1, 3, 3)
    sl = tuple(slice(o, o + s) for o, s in zip(off, shape))

    def has_plan(ext):
        return emu.l.mvn_plan_store_has_key(0, (ctypes.c_int * 3)(*ext)) == 1

    def reference(ext):
        def embed(x):
            out = np.zeros(ext, np.float32)
            out[sl] = x
            return out
        hp = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], 0.006, 1e-4, 2)
        orc.set_quotient_guard(True)
        try:
            return orc.cpu_deconvolve(embed(psi0), hp, 4)[sl]
        finally:
            orc.set_quotient_guard(False)

    emu.l.mvn_release_cached_engines()
    emu.check(emu.l.mvn_plan_store_clear())
    try:
        # the agreeing case first: exact dim0
        got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
        assert has_plan((23, 64, 64)) and not has_plan((24, 64, 64))
        ref = reference((23, 64, 64))
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
        emu.l.mvn_release_cached_engines()
        emu.check(emu.l.mvn_plan_store_clear())
        monkeypatch.setenv("MVN_NO_FIXED", "1")
        emu.check(emu.l.mvn_plan_store_add(0, (ctypes.c_int * 3)(23, 64, 64)))
        assert emu.plan_describe((23, 64, 64))["fx_rows"] == 0
        monkeypatch.delenv("MVN_NO_FIXED")
        got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
        assert has_plan((24, 64, 64)) and emu.plan_describe((24, 64, 64))["fx_rows"] == 1
        ref = reference((24, 64, 64))
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    finally:
        emu.l.mvn_release_cached_engines()
        emu.check(emu.l.mvn_plan_store_clear())


# ---- MVN_DEVICES: the blocking ABI call on several devices (mvn_multi.cpp) ----------------------------------------
@pytest.mark.parametrize("pad", ["none", "zero"])
@pytest.mark.parametrize("devices,emu_devices", [("0,0", None), ("0,1,0", "2"), ("0,0,0,0", None)])
def test_mvn_devices_runs_the_abi_call_as_halo_slabs(emu, monkeypatch, capfd, devices, emu_devices, pad):
    # VERDICT r03 missing 1: MVN_DEVICES=0,1,.. makes inplace_gpu_deconvolve (inc/multiviewnative.h:66-67) cut the
    # padded volume into dim0 slabs, one resident engine and one host thread per entry, halos pulled from the
    # neighbours before every dim0 leg - the reference's sequential sweep, so the result is that of the one-device
    # call BIT FOR BIT (same kernels on the same values; an entry may repeat: "0,0" = two slabs on one device).
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    if emu_devices:
        monkeypatch.setenv("MVN_EMU_DEVICES", emu_devices)
    shape, V, ks = (48, 16, 32), 2, (7, 3, 5)
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=21)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    emu.l.mvn_release_cached_engines()
    try:
        single = emu.gpu_deconvolve(psi0, h, pad_mode=pad)
        monkeypatch.setenv("MVN_DEVICES", devices)
        before = emu.l.mvn_multi_device_calls()
        multi = emu.gpu_deconvolve(psi0, h, pad_mode=pad)
        again = emu.gpu_deconvolve(psi0, h, pad_mode=pad)  # the cached group of slab engines
        assert emu.l.mvn_multi_device_calls() == before + 2  # (not a silent fall-back to one device)
        assert np.array_equal(multi, single) and np.array_equal(again, single)
        if pad == "none":
            ref = orc.cpu_deconvolve(psi0, h, 4)
            assert np.abs(multi - ref).max() <= 1e-5 * np.abs(ref).max()
            # one Inf voxel deep inside the first slab: every slab floods (the legs report to every slab's word)
            bad = psi0.copy()
            bad[5, 5, 5] = np.inf
            got = emu.gpu_deconvolve(bad, h, pad_mode=pad)
            assert np.array_equal(got, orc.cpu_deconvolve(bad, h, 4), equal_nan=True)
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
        emu.l.mvn_release_cached_engines()


def test_mvn_devices_falls_back_to_one_device(emu, monkeypatch, capfd):
    # a PSF deeper than the direct leg takes, slabs thinner than the halo, an odd last extent, a device that does
    # not exist: the call runs on one device as if the variable were not set
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    emu.l.mvn_release_cached_engines()
    try:
        for shape, ks, devices in (((80, 8, 16), (35, 3, 3), "0,0"), ((24, 8, 16), (9, 3, 3), "0,0,0,0,0,0,0,0"),
                                   ((24, 8, 15), (5, 3, 3), "0,0"), ((24, 8, 16), (5, 3, 3), "0,7")):
            _, views, k1, k2, w, psi0 = realistic_views(shape, 1, ks, seed=22)
            h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
            monkeypatch.delenv("MVN_DEVICES", raising=False)
            single = emu.gpu_deconvolve(psi0, h)
            monkeypatch.setenv("MVN_DEVICES", devices)
            before = emu.l.mvn_multi_device_calls()
            got = emu.gpu_deconvolve(psi0, h)
            assert emu.l.mvn_multi_device_calls() == before, shape
            assert np.array_equal(got, single), shape
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
        emu.l.mvn_release_cached_engines()


def test_resident_group_of_slab_engines(emu, monkeypatch):
    # mvn_group_*: the slabs of MVN_DEVICES as a resident object (load once, iterate in pieces, read back) - the
    # sweeps of several mvn_group_iterate calls add up to one engine's, bit for bit
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    shape, V, ks = (40, 16, 32), 2, (5, 3, 5)
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=23)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    e = emu.engine(shape, V)
    for v in range(V):
        e.set_view(v, views[v], w[v], k1[v], k2[v])
    e.set_psi(psi0)
    e.iterate(3, 0.006, 1e-4)
    one = e.get_psi()
    e.close()
    g = emu.group([0, 0, 0], shape, ks[0] // 2, V)
    try:
        g.load(psi0, h)
        assert g.iterate(1, 0.006, 1e-4) > 0
        g.iterate(2, 0.006, 1e-4)
        assert np.array_equal(g.get_psi(), one)
        with pytest.raises(native.MvnError):  # a PSF the direct leg does not take
            _, v2, k1b, k2b, w2, _ = realistic_views(shape, V, (35, 3, 3), seed=24)
            g.load(psi0, WorkspaceHolder(v2, k1b, k2b, w2, 0.006, 1e-4, 1))
    finally:
        g.close()
    with pytest.raises(native.MvnError):  # more halo planes than planes per slab
        emu.group([0, 0, 0, 0], (16, 16, 32), 5, V)


def test_slabs_of_a_large_volume_keep_the_split_nyquist_layout(emu, monkeypatch):
    # Above 256 MB a volume keeps its Nyquist plane (the packed DC column costs 6 % at 512^3), the plane's dim1 lines
    # ride in the main dim1 launches, and the slabs of MVN_DEVICES run that same layout whatever their own size:
    # the Nyquist plane has halo planes of its own, exchanged with the main array's.  Forced here on a small volume
    # (MVN_NYQ_PACKED=0) with fixed-length dim1 kernels (d1 = 64): bit-equal to one engine, and to the oracle's
    # flood through an Inf voxel.
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    monkeypatch.setenv("MVN_NYQ_PACKED", "0")
    shape, V, ks = (48, 64, 64), 2, (7, 5, 3)
    assert emu.plan_describe(shape)["fx_ax1"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=25)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    emu.l.mvn_release_cached_engines()
    try:
        single = emu.gpu_deconvolve(psi0, h)
        for devices in ("0,0", "0,0,0"):
            monkeypatch.setenv("MVN_DEVICES", devices)
            before = emu.l.mvn_multi_device_calls()
            multi = emu.gpu_deconvolve(psi0, h)
            assert emu.l.mvn_multi_device_calls() == before + 1
            assert np.array_equal(multi, single), devices
            bad = psi0.copy()
            bad[5, 5, 5] = np.inf
            assert np.array_equal(emu.gpu_deconvolve(bad, h), orc.cpu_deconvolve(bad, h, 4), equal_nan=True)
            monkeypatch.delenv("MVN_DEVICES")
        ref = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(single - ref).max() <= 1e-5 * np.abs(ref).max()
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
        emu.l.mvn_release_cached_engines()


# ---- round 4: the fused middle pass on the line layout (csrc/mvn_mid_fused.hpp) ----------------------------------
def _lines_case(shape, kshape, nviews=2, seed=60):
    _, views, k1, k2, w, psi0 = realistic_views(shape, nviews, kshape, seed=seed)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]  # an asymmetric second kernel of the same depth
    return views, k1, k2, w, psi0


@pytest.mark.parametrize("shape,kshape", [((12, 512, 512), (3, 5, 3)), ((40, 512, 512), (31, 5, 3)),
                                          ((36, 512, 512), (16, 3, 3)), ((20, 512, 512), (1, 3, 3))])
def test_fused_middle_pass_on_the_line_layout_vs_oracle(emu, monkeypatch, shape, kshape):
    # 512 x 512 planes, PSFs of at most 31 planes: the sequential sweep runs last-axis pass -> ONE middle pass
    # (dim1 forward, K-tap direct convolution along dim0, dim1 inverse) -> last-axis pass on a half-spectrum whose
    # lines along dim1 are contiguous, Nyquist bins packed into the DC column.  Odd / even / single-plane / deepest
    # instantiated PSF depths, lambda 0 and > 0, against the oracle; MVN_MID_FUSED=0 keeps the three-pass middle.
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")  # (by default only for volumes of at least three PSF depths of planes)
    emu.l.mvn_release_cached_engines()
    views, k1, k2, w, psi0 = _lines_case(shape, kshape)
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 2)
        c0 = emu.l.mvn_mid_fused_launch_count()
        got = emu.gpu_deconvolve(psi0, h)
        assert emu.l.mvn_mid_fused_launch_count() - c0 == 2 * 2 * 2  # iterations x views x convolutions
        ref = orc.cpu_deconvolve(psi0, h, 8)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), (shape, kshape, lam)
    if kshape[0] == 3:
        monkeypatch.setenv("MVN_MID_FUSED", "0")
        emu.l.mvn_release_cached_engines()
        c0 = emu.l.mvn_mid_fused_launch_count()
        three = emu.gpu_deconvolve(psi0, h)
        assert emu.l.mvn_mid_fused_launch_count() == c0
        assert np.abs(three - got).max() <= 1e-5 * np.abs(got).max()
        monkeypatch.setenv("MVN_MID_FUSED", "2")
    if kshape[0] == 31:  # 40 planes at 31 taps: the default rule keeps the three passes
        monkeypatch.delenv("MVN_MID_FUSED")
        emu.l.mvn_release_cached_engines()
        c0 = emu.l.mvn_mid_fused_launch_count()
        three = emu.gpu_deconvolve(psi0, h)
        assert emu.l.mvn_mid_fused_launch_count() == c0
        assert np.abs(three - got).max() <= 1e-5 * np.abs(got).max()
    emu.l.mvn_release_cached_engines()


def test_fused_middle_pass_nonfinite_voxel_and_other_loops(emu, monkeypatch):
    # a non-finite voxel floods the volume through the fused middle pass as it does through an FFT along dim0
    # (poison word, mvn_dim0_direct.hpp); the simultaneous step of the same engine keeps the three-pass middle
    # (nonfinite_cases runs both); a PSF deeper than 31 planes on the same shape falls back as a whole
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    emu.l.mvn_release_cached_engines()
    try:
        c0 = emu.l.mvn_mid_fused_launch_count()
        nonfinite_cases(emu, (24, 512, 512), (5, 3, 3), (11, 100, 7), its_list=(2,))
        assert emu.l.mvn_mid_fused_launch_count() > c0
        shape = (40, 512, 512)
        views, k1, k2, w, psi0 = _lines_case(shape, (33, 3, 3), nviews=1)
        h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
        c0 = emu.l.mvn_mid_fused_launch_count()
        got = emu.gpu_deconvolve(psi0, h)
        assert emu.l.mvn_mid_fused_launch_count() == c0
        ref = orc.cpu_deconvolve(psi0, h, 8)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    finally:
        emu.l.mvn_release_cached_engines()


def test_fused_middle_pass_in_the_simultaneous_loop(emu):
    # the simultaneous (Jacobi) step of the sharded driver on 512 x 512 planes: psi's last-axis spectrum once per
    # step (line layout), per view ONE middle pass -> fused divide -> ONE middle pass -> correction; whole steps,
    # the chunked form with the next step's spectrum fed chunk by chunk (Engine::apply_delta_chunk), and a
    # sequential sweep on the same engine afterwards
    shape = (24, 512, 512)
    views, k1, k2, w, psi0 = _lines_case(shape, (5, 3, 3))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 8)
    e = emu.engine(shape, 2)
    try:
        for v in range(2):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        c0 = emu.l.mvn_mid_fused_launch_count()
        for _ in range(2):
            e.compute_delta(0.006, 1e-4)
            e.apply_delta()
        assert emu.l.mvn_mid_fused_launch_count() - c0 == 2 * 2 * 2
        whole = e.get_psi()
        assert np.abs(whole - ref).max() <= 1e-5 * np.abs(ref).max()
        e.set_psi(psi0)
        n = e.delta_chunks(4)
        for _ in range(2):
            e.compute_delta_head(0.006, 1e-4)
            for c in range(n):
                e.compute_delta_chunk(c, n)
            for c in range(n):
                e.apply_delta_chunk(c, n, True)
        assert np.array_equal(e.get_psi(), whole)
        e.set_psi(psi0)
        e.iterate(2, 0.006, 1e-4)
        seq = orc.cpu_deconvolve(psi0, h, 8)
        assert np.abs(e.get_psi() - seq).max() <= 1e-5 * np.abs(seq).max()
    finally:
        e.close()


def test_default_padding_policy_reaches_the_fused_middle_pass(emu):
    # blocks whose rows and columns pad to 512 - 482 + 31 - 1 - run the fused middle pass under the library's DEFAULT
    # policy (zero padding to FFT-friendly extents, dim0 exact under the direct leg): what a host program that sizes
    # its blocks for it gets; oracle on hand-padded stacks, guard on
    shape, ks = (12, 482, 482), (5, 31, 31)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, ks, seed=2)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    emu.l.mvn_release_cached_engines()
    c0 = emu.l.mvn_mid_fused_launch_count()
    got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert emu.l.mvn_mid_fused_launch_count() - c0 == 2 * 2 * 2
    ext, off = (16, 512, 512), (2, 15, 15)
    sl = tuple(slice(o, o + s) for o, s in zip(off, shape))

    def embed(x):
        out = np.zeros(ext, np.float32)
        out[sl] = x
        return out

    hp = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], 0.006, 1e-4, 2)
    orc.set_quotient_guard(True)
    try:
        ref = orc.cpu_deconvolve(embed(psi0), hp, 8)[sl]
    finally:
        orc.set_quotient_guard(False)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    emu.l.mvn_release_cached_engines()


@pytest.mark.parametrize("devices,emu_devices", [("0,0", None), ("0,1,0", "2")])
def test_slabs_run_the_fused_middle_pass(emu, monkeypatch, devices, emu_devices):
    # MVN_DEVICES on planes of 512 x 512: the slabs exchange halo planes of the MIDDLE's input, so they all take the
    # fused middle pass or none does (HaloGroup::load decides; Engine::set_lines_in_halo_mode) - last-axis pass on the
    # boundary planes first, the neighbours pull them, ONE middle pass per convolution walks every column from the
    # lower halo to the upper one.  Bit-equal to the one-device call, the oracle's flood through an Inf voxel.
    if emu_devices:
        monkeypatch.setenv("MVN_EMU_DEVICES", emu_devices)
    shape = (48, 512, 512)
    views, k1, k2, w, psi0 = _lines_case(shape, (5, 3, 3))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    emu.l.mvn_release_cached_engines()
    try:
        single = emu.gpu_deconvolve(psi0, h)
        monkeypatch.setenv("MVN_DEVICES", devices)
        before, c0 = emu.l.mvn_multi_device_calls(), emu.l.mvn_mid_fused_launch_count()
        multi = emu.gpu_deconvolve(psi0, h)
        assert emu.l.mvn_multi_device_calls() == before + 1
        assert emu.l.mvn_mid_fused_launch_count() - c0 == 2 * 2 * 2 * len(devices.split(","))
        assert np.array_equal(multi, single)
        bad = psi0.copy()
        bad[30, 5, 5] = np.inf
        assert np.array_equal(emu.gpu_deconvolve(bad, h), orc.cpu_deconvolve(bad, h, 8), equal_nan=True)
        monkeypatch.delenv("MVN_DEVICES")
        ref = orc.cpu_deconvolve(psi0, h, 8)
        assert np.abs(single - ref).max() <= 1e-5 * np.abs(ref).max()
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
        emu.l.mvn_release_cached_engines()
