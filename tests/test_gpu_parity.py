"""Parity of the HIP hot path (through the C-ABI of lib/libmultiviewnative.so) against the CPU
oracle, the committed golden values and size-independent properties.  Needs a real MI355X."""
import os

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import Fixture3D, GOLDEN_SUMS, realistic_views, synthetic_views

pytestmark = pytest.mark.gpu

# stated float32 tolerance of the RL result vs the CPU path
MAX_REL = 1e-4
RMS_REL = 1e-5


@pytest.fixture(scope="module")
def gpu():
    import os
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):  # fresh checkout on the GPU box: compile, never fall back
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()  # raises if the HIP library is missing: no fallback
    assert b.backend_name() == "hip-gfx950"
    assert b.l.getNumDevicesCUDA() >= 1
    return b


@pytest.fixture(scope="module")
def orc():
    from oracle import binding
    return binding


# The suite pins the direct dim0 leg to large planes (tests/conftest.py) so that the many small-shape cases keep
# validating the fused FFT dim0 pass; a host program gets the PRODUCT DEFAULTS - the direct leg at every size,
# columns cut into pieces, the Nyquist bins packed into the DC column.  Tests that take this fixture run under
# both.  The switches are read per engine / per call: cached engines are dropped either side.
@pytest.fixture(params=["suite pin", "product defaults"])
def leg(request, gpu, monkeypatch):
    if request.param == "product defaults":
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    gpu.check(gpu.l.mvn_release_cached_engines())
    yield request.param
    gpu.check(gpu.l.mvn_release_cached_engines())


def rel_err(got, ref):
    d = got.astype(np.float64) - ref.astype(np.float64)
    return (np.abs(d).max() / max(np.abs(ref).max(), 1e-30),
            np.sqrt(np.mean(d * d)) / max(np.sqrt(np.mean(ref.astype(np.float64) ** 2)), 1e-30))


def test_device_queries(gpu):
    l = gpu.l
    n = l.getNumDevicesCUDA()
    assert n >= 1
    name = (b"\0" * 256)
    import ctypes
    buf = ctypes.create_string_buffer(256)
    l.getNameDeviceCUDA(0, buf)
    assert len(buf.value) > 0
    assert l.getMemDeviceCUDA(0) > (100 << 30)  # 288 GB HBM3E
    assert l.getCUDAcomputeCapabilityMajorVersion(0) == 95
    assert l.getCUDAcomputeCapabilityMinorVersion(0) == 0
    assert 0 <= l.selectDeviceWithHighestComputeCapability() < n


SHAPES = [(8, 8, 8), (4, 6, 10), (13, 17, 19), (16, 18, 14), (6, 10, 15), (32, 20, 64), (3, 5, 2),
          (12, 7, 9), (1, 1, 4), (2, 3, 1), (24, 40, 22), (64, 64, 64), (5, 4, 46), (128, 96, 160),
          (40, 30, 250), (7, 542, 6), (27, 25, 49)]


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_vs_pocketfft(gpu, shape):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = gpu.rfft3(x)
    assert np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30) < 5e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_vs_pocketfft(gpu, shape):
    rng = np.random.default_rng(8)
    x = rng.standard_normal(shape)
    spec = np.fft.rfftn(x).astype(np.complex64)
    ref = np.fft.irfftn(spec.astype(np.complex128), s=shape, axes=(0, 1, 2)) * np.prod(shape)
    got = gpu.irfft3(spec, shape[2])
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6


# shapes served by the compile-time specialised kernels: expected (fx_rows, fx_ax1, fx_ax0)
FIXED_SHAPES = {(64, 64, 64): (1, 1, 1), (64, 128, 256): (1, 1, 1), (128, 64, 512): (1, 1, 1),
                (256, 64, 64): (1, 1, 1), (64, 512, 64): (1, 1, 1), (1024, 64, 32): (0, 1, 1),
                (64, 64, 1024): (1, 1, 1), (8, 64, 2048): (1, 1, 0), (16, 1024, 64): (1, 1, 0),
                (32, 20, 64): (1, 0, 0), (256, 256, 256): (1, 1, 1)}


@pytest.mark.parametrize("shape", sorted(FIXED_SHAPES))
def test_fixed_kernels_forward_and_roundtrip(gpu, shape):
    info = gpu.plan_describe(shape)
    assert (info["fx_rows"], info["fx_ax1"], info["fx_ax0"]) == FIXED_SHAPES[shape]
    x = np.random.default_rng(9).standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = gpu.rfft3(x)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6
    back = gpu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5


MIXED_FIXED_SHAPES = {(96, 160, 288): (1, 1, 1), (288, 96, 160): (1, 1, 1), (160, 288, 96): (1, 1, 1),
                      (64, 192, 384): (1, 1, 1), (320, 64, 640): (1, 1, 1), (64, 576, 192): (1, 1, 1),
                      (2, 1920, 1920): (1, 1, 0), (1280, 16, 64): (1, 0, 1), (960, 16, 576): (1, 0, 1),
                      (768, 16, 960): (1, 0, 1), (640, 384, 64): (1, 1, 1), (16, 64, 1536): (1, 1, 0),
                      (16, 64, 1280): (1, 1, 0)}


@pytest.mark.parametrize("shape", sorted(MIXED_FIXED_SHAPES))
def test_mixed_radix_fixed_kernels(gpu, shape):
    info = gpu.plan_describe(shape)
    assert (info["fx_rows"], info["fx_ax1"], info["fx_ax0"]) == MIXED_FIXED_SHAPES[shape]
    x = np.random.default_rng(10).standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = gpu.rfft3(x)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6
    back = gpu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5


def test_mixed_radix_fixed_deconvolve_vs_oracle(gpu, orc):
    shape = (64, 192, 320)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 7, 9))
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
        mx, rms = rel_err(gpu.gpu_deconvolve(psi0, h), orc.cpu_deconvolve(psi0, h, 8))
        assert mx <= MAX_REL and rms <= RMS_REL


# every last-axis length of the walking (row-major tile) kernels through the fused c2r + pointwise + r2c passes,
# with tiles left over for the walk (rows = 96: more tiles than one sweep of some lengths, fewer of others)
@pytest.mark.parametrize("d2", [96, 160, 288, 320, 384, 576, 640, 768, 960, 1280, 1536, 1920, 2048])
def test_walking_rows_kernels_deconvolve_vs_oracle(gpu, orc, d2):
    shape = (6, 16, d2)
    assert gpu.plan_describe(shape)["fx_rows"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (3, 3, 5))
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
        mx, rms = rel_err(gpu.gpu_deconvolve(psi0, h), orc.cpu_deconvolve(psi0, h, 8))
        assert mx <= MAX_REL and rms <= RMS_REL


BLUESTEIN_SHAPES = [(37, 41, 74), (4, 271, 6), (271, 4, 8), (6, 5, 542), (67, 8, 134), (3, 3, 37),
                    (127, 131, 262)]


@pytest.mark.parametrize("shape", BLUESTEIN_SHAPES)
def test_bluestein_axes(gpu, shape):
    # lengths with a prime factor > 31 take the chirp-z (Bluestein) route inside the same passes
    x = np.random.default_rng(12).standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = gpu.rfft3(x)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-5
    back = gpu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 5e-5


def test_bluestein_deconvolve_vs_oracle(gpu, orc):
    shape = (37, 12, 74)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 3, 7))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    mx, rms = rel_err(gpu.gpu_deconvolve(psi0, h), orc.cpu_deconvolve(psi0, h, 4))
    assert mx <= MAX_REL and rms <= 3 * RMS_REL  # the chirp-z route costs a few extra ulps


def test_fixed_and_generic_kernels_agree(gpu, orc, monkeypatch):
    # the same shape through the run-time-radix kernels (MVN_NO_FIXED=1) and the specialised ones
    shape = (64, 64, 128)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 7, 9))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    ref = orc.cpu_deconvolve(psi0, h, 8)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("MVN_NO_FIXED", flag)
        gpu.check(gpu.l.mvn_plan_store_clear())
        assert gpu.plan_describe(shape)["fx_rows"] == (1 if flag == "0" else 0)
        outs.append(gpu.gpu_deconvolve(psi0, h))
    monkeypatch.delenv("MVN_NO_FIXED")
    gpu.check(gpu.l.mvn_plan_store_clear())
    for o in outs:
        mx, rms = rel_err(o, ref)
        assert mx <= MAX_REL and rms <= RMS_REL
    assert np.abs(outs[0] - outs[1]).max() <= 2e-5 * np.abs(ref).max()


def test_fused_pipeline_invariants(gpu, orc):
    # 8-pass pipeline with the fused last-axis passes: no hidden state across calls, i.e. N
    # iterations == N x 1 iteration.  The last pass of a call runs the un-fused kernel, whose
    # butterflies the compiler contracts into FMAs differently, so equality is to rounding (a few
    # float32 ulps), not bit for bit (it is bit for bit in the FMA-free emulation, test_emu_engine)
    shape = (64, 64, 128)
    assert gpu.plan_describe(shape)["fx_rows"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, 3, (5, 5, 5))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    three = gpu.gpu_deconvolve(psi0, h)
    h.with_iterations(1)
    one = psi0
    for _ in range(3):
        one = gpu.gpu_deconvolve(one, h)
    assert np.abs(one - three).max() <= 1e-6 * np.abs(three).max()
    h.with_iterations(3)
    mx, rms = rel_err(three, orc.cpu_deconvolve(psi0, h, 8))
    assert mx <= MAX_REL and rms <= RMS_REL


def test_forward_matches_oracle_fft(gpu, orc):
    x = np.random.default_rng(3).standard_normal((24, 20, 36)).astype(np.float32)
    a, b = gpu.rfft3(x), orc.rfft3_forward(x, 4)
    assert np.abs(a - b).max() / np.abs(b).max() < 3e-6


def test_ramp_roundtrip(gpu):
    # tests/test_plan_store.cpp:83-142 demands exact equality of the 8^3 integer ramp after
    # r2c -> c2r -> /512 from FFTW (pinned on the oracle in test_oracle_fft.py); the reference's GPU
    # twin (tests/test_plan_store.cu) has no such check.  The HIP butterflies contract to FMAs, so
    # here the bound is one float32 ulp of the largest value (511 -> 2^-15 * 2 = 6.1e-5).
    x = np.arange(512, dtype=np.float32).reshape(8, 8, 8)
    back = gpu.irfft3(gpu.rfft3(x), 8) / np.float32(512)
    assert np.abs(back - x).max() <= 6.2e-5
    assert np.array_equal(np.rint(back), x)


@pytest.mark.parametrize("shape", [(13, 17, 19), (16, 16, 16), (9, 27, 3), (27, 9, 81), (5, 25, 125),
                                   (7, 49, 7)])
def test_roundtrip_mse(gpu, shape):
    # tests/test_fftw_numerical_stability.cpp:32-664 on the GPU transforms
    n = int(np.prod(shape))
    x = np.arange(n, dtype=np.float32).reshape(shape)
    back = gpu.irfft3(gpu.rfft3(x), shape[2]) / np.float32(n)
    mse = float(np.mean((back.astype(np.float64) - x) ** 2))
    assert mse < 1e-4 * max(1.0, (n / 4096.0) ** 2)


def test_large_roundtrip_and_parseval(gpu):
    # full-size property checks (no CPU reference needed): 256^3 roundtrip + Parseval
    shape = (256, 256, 256)
    x = np.random.default_rng(11).standard_normal(shape).astype(np.float32)
    spec = gpu.rfft3(x)
    back = gpu.irfft3(spec, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5
    # Parseval over the half spectrum: bins 1..N/2-1 count twice
    w = np.full(shape[2] // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    e_spec = float((np.abs(spec.astype(np.complex128)) ** 2 * w).sum()) / np.prod(shape)
    e_real = float((x.astype(np.float64) ** 2).sum())
    assert abs(e_spec - e_real) / e_real < 1e-5


def test_plan_store_semantics(gpu):
    import ctypes as C
    l = gpu.l
    gpu.check(l.mvn_plan_store_clear())
    assert l.mvn_plan_store_empty() == 1
    d = (C.c_int * 3)(8, 8, 8)
    assert l.mvn_plan_store_has_key(0, d) == 0
    gpu.check(l.mvn_plan_store_add(0, d))
    assert l.mvn_plan_store_has_key(0, d) == 1 and l.mvn_plan_store_size() == 1


@pytest.mark.parametrize("name", ["identity", "horizont", "vertical", "depth", "all1"])
def test_convolution_fixture_sums(gpu, orc, name):
    # tests/test_gpu_convolve.cpp:9-327: both convolution entry points vs the fixture sums, 1e-5 %
    fx = Fixture3D()
    for legacy in (False, True):
        out = gpu.gpu_convolution(fx.padded_image, getattr(fx, name), legacy=legacy)
        got = float(out[fx.interior].astype(np.float64).sum())
        assert abs(got - GOLDEN_SUMS[name]) / GOLDEN_SUMS[name] * 100 < 1e-5 * 100
        ref = orc.cpu_convolution(fx.padded_image, getattr(fx, name))
        assert np.abs(out - ref).max() <= 2e-6 * np.abs(ref).max()


def test_asymm_delta_reproduces_kernel(gpu):
    fx = Fixture3D()
    for name in ("asymm_cross", "asymm_one", "asymm_identity"):
        kernel = getattr(fx, name)
        one = gpu.gpu_convolution(fx.padded_one, kernel)[fx.interior]
        pos = tuple(slice(s // 2 - k // 2, s // 2 - k // 2 + k) for s, k in zip(one.shape, kernel.shape))
        assert np.array_equal(np.floor(one[pos] + 0.5), kernel)
        assert abs(float(one.sum()) - float(kernel.sum())) / float(kernel.sum()) < 1e-5


def test_identity_16x18x14(gpu):
    # tests/test_gpu_convolve_impl.cu:422-529: 16x18x14 identity -> per-voxel |d| < 1e-3
    rng = np.random.default_rng(2)
    im = rng.uniform(0, 100, (16, 18, 14)).astype(np.float32)
    k = np.zeros((3, 3, 3), np.float32)
    k[1, 1, 1] = 1
    assert np.abs(gpu.gpu_convolution(im, k) - im).max() < 1e-3


@pytest.mark.parametrize("shape,kshape", [((16, 18, 14), (3, 3, 3)), ((13, 17, 19), (5, 3, 7)),
                                          ((20, 12, 9), (4, 3, 2)), ((8, 8, 8), (8, 8, 8)),
                                          ((64, 48, 80), (15, 15, 15)), ((30, 57, 81), (23, 9, 5))])
def test_convolution_vs_oracle(gpu, orc, shape, kshape):
    rng = np.random.default_rng(5)
    im = rng.uniform(0, 10, shape).astype(np.float32)
    k = rng.uniform(0, 1, kshape).astype(np.float32)
    got = gpu.gpu_convolution(im, k)
    ref = orc.cpu_convolution(im, k, 4)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 3e-6


def test_kernel_larger_than_image_is_rejected(gpu, capfd):
    im = np.ones((4, 4, 4), np.float32)
    out = gpu.gpu_convolution(im, np.ones((5, 3, 3), np.float32))
    assert np.array_equal(out, im)
    assert "kernel extent" in capfd.readouterr().err


def test_pointwise_entry_points_bit_exact(gpu, orc):
    # tests/test_gpu_kernels_impl.cu:57-351: bit-for-bit vs the CPU kernels, incl. 256x255x257-like
    # ragged sizes and NaN/Inf flow
    rng = np.random.default_rng(0)
    for n in (1, 63, 1000, 256 * 255 + 7):
        view = rng.uniform(0, 5, n).astype(np.float32)
        blurred = rng.uniform(-1, 5, n).astype(np.float32)
        blurred[:min(3, n)] = [0, np.nan, np.inf][:min(3, n)]
        assert np.array_equal(gpu.compute_quotient(view, blurred), orc.compute_quotient(view, blurred),
                              equal_nan=True)
        psi = rng.uniform(0.5, 10, n).astype(np.float32)
        integral = rng.uniform(-0.1, 1, n).astype(np.float32)
        integral[:min(3, n)] = [np.nan, np.inf, -np.inf][:min(3, n)]
        w = rng.uniform(0, 1, n).astype(np.float32)
        for lam in (0.0, 0.006):
            assert np.array_equal(gpu.compute_final_values(psi, integral, w, 1e-4, lam),
                                  orc.final_values(psi, integral, w, 1e-4, lam))
    # constants of the reference test: psi=5, integral=42, w=.1, lambda=.006, min=1e-4
    c = gpu.compute_final_values(np.full(64, 5, np.float32), np.full(64, 42, np.float32),
                                 np.full(64, .1, np.float32), 1e-4, 0.0)
    assert np.all(c == np.float32(0.1) * (np.float32(210) - np.float32(5)) + np.float32(5))
    q = gpu.compute_quotient(np.ones(100, np.float32), np.full(100, 5, np.float32))
    assert np.all(q == np.float32(0.2))


@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("shape,kshape,nv,its", [((16, 20, 18), (5, 5, 5), 3, 3),
                                                 ((13, 17, 19), (3, 5, 3), 2, 3),
                                                 ((8, 12, 10), (3, 3, 3), 1, 5),
                                                 ((64, 64, 64), (9, 9, 9), 3, 10),
                                                 ((48, 60, 40), (7, 11, 5), 6, 4)])
def test_deconvolve_vs_oracle(gpu, orc, shape, kshape, nv, its, lam, leg):
    _, views, k1, k2, w, psi0 = realistic_views(shape, nv, kshape)
    h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, its)
    got = gpu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 8)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)
    # the reference's own acceptance: sum of squared differences < 1 (test_gpu_deconvolve_impl.cu:200)
    assert float(((got.astype(np.float64) - ref) ** 2).sum()) < 1


def test_baseline_config0_64cubed(gpu, orc, leg):
    # BASELINE.json configs[0]: 64^3, 1 view, 3^3 PSF, 5 iterations (reference synthetic data)
    shape = (64, 64, 64)
    views, k1, k2, w = synthetic_views(shape, 1, 3, 3)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 5)
    psi0 = np.full(shape, 3.0, np.float32)
    got = gpu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 8)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL
    assert np.abs(got - 29.40588).max() < 2e-4 * 29.40588


def test_baseline_config1_256cubed_vs_oracle(gpu, orc, leg):
    # BASELINE.json configs[1]: 256^3, 1 view, 15^3 Gaussian PSF, 10 iterations; oracle on all cores
    from ref_fixtures import gaussian_psf
    shape = (256, 256, 256)
    rng = np.random.default_rng(42)
    truth = np.full(shape, 10.0, np.float32)
    for _ in range(40):
        c = [int(rng.uniform(0.1 * s, 0.9 * s)) for s in shape]
        truth[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3] += rng.uniform(50, 500)
    psf = gaussian_psf((15, 15, 15), (2.0, 2.0, 3.0))
    view = orc.cpu_convolution(truth, psf, 8)
    h = WorkspaceHolder([view], [psf], [np.ascontiguousarray(psf[::-1, ::-1, ::-1])],
                        [np.ones(shape, np.float32)], 0.006, 1e-4, 10)
    psi0 = np.full(shape, np.float32(view.mean()), np.float32)
    got = gpu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, 8)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


@pytest.mark.parametrize("n_views,want", [(1, 29.40588), (6, 37.72946), (8, 43.75619)])
def test_synthetic_closed_form(gpu, n_views, want):
    shape = (32, 32, 32)
    views, k1, k2, w = synthetic_views(shape, n_views, 21, 25)  # the reference's 21^3 / 25^3 kernels
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 2)
    psi = gpu.gpu_deconvolve(np.full(shape, 3.0, np.float32), h)
    assert np.abs(psi - want).max() < 2e-4 * want


def test_full_size_512_closed_form(gpu):
    # BASELINE.json configs[2] size (512^3, 6 views) through a size-independent property: the
    # reference's synthetic data has a closed-form fixed point in every voxel
    shape = (512, 512, 512)
    eng = gpu.engine(shape, 6)
    views, k1, k2, w = synthetic_views((1, 1, 1), 6, 31, 31)
    ones = np.ones(shape, np.float32)
    for v in range(6):
        eng.set_view(v, np.full(shape, 16.0 + 4.0 * v, np.float32), ones, k1[v], k2[v])
    eng.set_psi(np.full(shape, 3.0, np.float32))
    eng.iterate(2, 0.006, 1e-3)
    psi = eng.get_psi()
    eng.close()
    assert np.abs(psi - 37.72946).max() < 2e-4 * 37.72946


def test_full_size_config5_closed_form(gpu):
    # BASELINE.json configs[4] shape (320 x 1920 x 1920, dims[2] fastest; mixed radix 2^a*3*5 on
    # every axis) through the same size-independent property, 2 of its 6 views to bound host memory
    shape = (320, 1920, 1920)
    eng = gpu.engine(shape, 2)
    _, k1, k2, _ = synthetic_views((1, 1, 1), 2, 31, 31)
    ones = np.ones(shape, np.float32)
    buf = np.empty(shape, np.float32)
    for v in range(2):
        buf.fill(16.0 + 4.0 * v)
        eng.set_view(v, buf, ones, k1[v], k2[v])
    buf.fill(3.0)
    eng.set_psi(buf)
    eng.iterate(2, 0.006, 1e-3)
    psi = eng.get_psi()
    eng.close()
    want = (np.sqrt(1 + 2 * 0.006 * (20.0 * 3 / 2)) - 1) / 0.006  # f((16+4v)(v+2)/(v+1)), v = 1
    assert np.abs(psi - want).max() < 2e-4 * want


def test_loop_invariants(gpu, orc, leg):
    shape = (16, 16, 16)
    views, k1, k2, w = synthetic_views(shape, 3, 3, 5)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 2)
    psi0 = np.random.default_rng(1).uniform(1, 4, shape).astype(np.float32)
    two = gpu.gpu_deconvolve(psi0, h)
    h.with_iterations(0)  # tests/test_gpu_deconvolve_impl.cu:333-376
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h), psi0)
    h.with_iterations(1)  # N iterations == N x 1 iteration, to rounding (fused vs un-fused last pass)
    again = gpu.gpu_deconvolve(gpu.gpu_deconvolve(psi0, h), h)
    assert np.abs(again - two).max() <= 1e-6 * np.abs(two).max()
    # zero start: Inf/NaN flow through the FFT and are caught by the clamp chain, as on the CPU
    z = np.zeros(shape, np.float32)
    assert np.array_equal(gpu.gpu_deconvolve(z, h), orc.cpu_deconvolve(z, h, 1))


def test_errors_leave_psi_untouched(gpu, capfd):
    views, k1, k2, w = synthetic_views((8, 8, 8), 2, 3, 3)
    views[1] = np.ones((8, 8, 4), np.float32)
    w[1] = np.ones((8, 8, 4), np.float32)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 1)
    psi0 = np.full((8, 8, 8), 2.0, np.float32)
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h), psi0)
    assert "share image_dims_" in capfd.readouterr().err
    views, k1, k2, w = synthetic_views((8, 8, 8), 1, 3, 3)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 1)
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h, device=99), psi0)
    assert "no usable GPU" in capfd.readouterr().err


def test_device_minus_one_autoselects(gpu, orc):
    shape = (8, 8, 8)
    views, k1, k2, w = synthetic_views(shape, 1, 3, 3)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 1)
    psi0 = np.full(shape, 2.0, np.float32)
    assert np.allclose(gpu.gpu_deconvolve(psi0, h, device=-1), orc.cpu_deconvolve(psi0, h, 1), rtol=1e-5)


@pytest.mark.parametrize("shape", [(24, 20, 28), (64, 64, 128)])
def test_simultaneous_mode_vs_oracle(gpu, orc, shape, leg):
    _, views, k1, k2, w, psi0 = realistic_views(shape, 4, (5, 5, 5))
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    eng = gpu.engine(shape, 4)
    for v in range(4):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    for _ in range(3):
        eng.compute_delta(0.006, 1e-4)
        eng.apply_delta()
    got = eng.get_psi()
    eng.close()
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 4)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL


def test_device_pointer_convolution_core(gpu, orc):
    # convolution3DfftCUDAInPlace_core takes DEVICE pointers (src/multiviewnative.cu:243-319);
    # the caller allocates them with the HIP runtime, as the reference's callers do with CUDA's
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the product library is already linked to
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    H2D, D2H = 1, 2
    for shape in ((16, 18, 14), (9, 8, 7)):
        rng = np.random.default_rng(4)
        im = rng.uniform(0, 10, shape).astype(np.float32)
        k = rng.uniform(0, 1, (3, 3, 3)).astype(np.float32)
        n = im.size + 2 * shape[0] * shape[1]  # the reference's in-place r2c allocation
        d_im, d_k = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_im), n * 4) == 0
        assert hip.hipMalloc(C.byref(d_k), k.size * 4) == 0
        assert hip.hipMemcpy(d_im, im.ctypes.data_as(C.c_void_p), im.size * 4, H2D) == 0
        assert hip.hipMemcpy(d_k, k.ctypes.data_as(C.c_void_p), k.size * 4, H2D) == 0
        idims = np.array(shape, np.int32)
        kdims = np.array(k.shape, np.int32)
        gpu.l.convolution3DfftCUDAInPlace_core(d_im, idims.ctypes.data_as(C.POINTER(C.c_int)), d_k,
                                               kdims.ctypes.data_as(C.POINTER(C.c_int)), 0)
        got = np.empty(shape, np.float32)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_im, im.size * 4, D2H) == 0
        hip.hipFree(d_im)
        hip.hipFree(d_k)
        ref = orc.cpu_convolution(im, k, 2)
        assert np.abs(got - ref).max() / np.abs(ref).max() < 3e-6


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


def test_zero_padd_mode_matches_reference_gpu_policy(gpu, orc, monkeypatch, leg):
    shape = (20, 16, 24)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 3, 7))
    k2[1] = k2[1][:3]  # kernels of different extents: the policy takes the maxima
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    cyclic = gpu.gpu_deconvolve(psi0, h)  # pad_mode="none", the CPU path's policy
    padded = gpu.gpu_deconvolve(psi0, h, pad_mode="zero_exact")  # exactly image + kernel - 1
    ref = _zero_padd_reference(orc, psi0, views, k1, k2, w, 0.006, 1e-4, 3)
    assert np.abs(padded - ref).max() <= 1e-4 * np.abs(ref).max()
    assert np.abs(padded - cyclic).max() > 1e-3 * np.abs(ref).max()  # the two policies do differ
    # the same selection through the environment (what round 1 offered), the setter left alone
    monkeypatch.setenv("MVN_PAD_MODE", "zero_exact")
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h, pad_mode=False), padded)
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h, pad_mode=False), cyclic)
    monkeypatch.delenv("MVN_PAD_MODE")


def test_zero_padd_good_size_mode(gpu, orc, monkeypatch, leg):
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
    got = gpu.gpu_deconvolve(psi0, h, pad_mode=False)  # no setter, no environment: the default
    assert np.array_equal(got, gpu.gpu_deconvolve(psi0, h, pad_mode="zero"))
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


def test_concurrent_abi_calls_are_serialised_per_device(gpu, orc):
    # the reference is not re-entrant (SURVEY.md 8b "Threading"); here concurrent callers on one
    # device queue up behind a per-device mutex and every one gets the right answer
    import threading
    shape = (32, 24, 40)
    cases = []
    for seed in range(4):
        _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 5, 5), seed=seed)
        cases.append((WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3), psi0))
    out = [None] * len(cases)

    def work(i):
        out[i] = gpu.gpu_deconvolve(cases[i][1], cases[i][0], pad_mode=False)

    gpu.set_pad_mode("none")  # process-wide: set once around the concurrent callers
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(cases))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    gpu.set_pad_mode(None)
    for i, (h, psi0) in enumerate(cases):
        mx, rms = rel_err(out[i], orc.cpu_deconvolve(psi0, h, 4))
        assert mx <= MAX_REL and rms <= RMS_REL


def test_degenerate_inputs(gpu, capfd):
    shape = (8, 8, 8)
    views, k1, k2, w = synthetic_views(shape, 1, 3, 3)
    psi0 = np.full(shape, 2.0, np.float32)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 1)
    h.ws.num_views_ = 0  # empty workspace: nothing to do, psi unchanged, no diagnostics
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h), psi0)
    assert capfd.readouterr().err == ""
    h.ws.num_views_ = 1
    h.ws.num_iterations_ = -3  # negative iteration counts behave like zero
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h), psi0)
    # 1-voxel-thick stacks and a kernel as large as the image
    thin = (1, 6, 10)
    v = [np.random.default_rng(0).uniform(1, 2, thin).astype(np.float32)]
    k = [np.random.default_rng(1).uniform(0, 1, thin).astype(np.float32)]
    k[0] /= k[0].sum()
    hh = WorkspaceHolder(v, k, k, [np.ones(thin, np.float32)], 0.0, 1e-4, 2)
    from oracle import binding as orc2
    got = gpu.gpu_deconvolve(np.ones(thin, np.float32), hh)
    ref = orc2.cpu_deconvolve(np.ones(thin, np.float32), hh, 1)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("name", ["identity", "horizont", "vertical", "depth", "all1"])
def test_golden_fixture_a(gpu, name, leg):
    # committed golden vectors (tests/golden/fixture_a.npz): the reference's fixture and its
    # FFT-independent expectations
    from golden_util import fixture_a
    g = fixture_a()
    out = gpu.gpu_convolution(g["padded_image"], g["kernel_" + name])[1:9, 1:9, 1:9]
    want = g["expect_" + name]
    assert np.abs(out - want).max() <= 3e-6 * np.abs(want).max()


@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_golden_rl_small(gpu, lam, leg):
    # committed RL vectors computed by the float64 numpy restatement (independent of the C oracle)
    from golden_util import rl_small
    psi0, h, seq, sim = rl_small(lam)
    got = gpu.gpu_deconvolve(psi0, h)
    assert np.abs(got - seq).max() <= MAX_REL * np.abs(seq).max()
    nv = h.ws.num_views_
    eng = gpu.engine(psi0.shape, nv)
    for v in range(nv):
        eng.set_view(v, h.views[v], h.weights[v], h.kernels1[v], h.kernels2[v])
    eng.set_psi(psi0)
    for _ in range(h.ws.num_iterations_):
        eng.compute_delta(lam, 1e-4)
        eng.apply_delta()
    got = eng.get_psi()
    eng.close()
    assert np.abs(got - sim).max() <= MAX_REL * np.abs(sim).max()


def test_deconvolve_staging_error_leaves_psi_untouched(gpu, capfd):
    # the PSF of the second view is larger than the stack: the uploader thread fails while the main
    # thread already iterates on view 0 -- the call must come back cleanly with psi untouched
    shape = (8, 8, 8)
    views, k1, k2, w = synthetic_views(shape, 2, 3, 3)
    k1[1] = np.ones((9, 3, 3), np.float32)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-3, 2)
    psi0 = np.full(shape, 2.0, np.float32)
    assert np.array_equal(gpu.gpu_deconvolve(psi0, h), psi0)
    assert "kernel extent" in capfd.readouterr().err


def _legacy_case(seed, shape, kshape):
    rng = np.random.default_rng(seed)
    image = rng.uniform(1, 20, shape).astype(np.float32)
    kernel = rng.uniform(0, 1, kshape).astype(np.float32)
    kernel /= kernel.sum()
    return image, kernel


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kshape", [((16, 16, 16), (3, 3, 3)), ((12, 10, 9), (5, 3, 3))])
def test_iterate_fft_legacy_steps(gpu, orc, shape, kshape):
    # src/multiviewnative.cu:395-600: one RL step with kernel2 = 0.1, weights = 1
    image, kernel = _legacy_case(3, shape, kshape)
    got = gpu.iterate_fft(image, kernel)
    ref = orc.iterate_fft(image, kernel)
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    for lam in (0.006, 0.5):
        got = gpu.iterate_fft(image, kernel, 1e-3, lam)
        ref = orc.iterate_fft(image, kernel, 1e-3, lam)
        assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    # an integral of 0.1 * sum(quotient) is far above minValue: the legacy blend returns t itself
    integral = orc.cpu_convolution(orc.compute_quotient(image, orc.cpu_convolution(image, kernel)),
                                   np.full_like(kernel, .1))
    lf = np.float32(0.006)
    t = ((np.sqrt(1.0 + 2.0 * np.float64(lf) * (image * integral).astype(np.float64)) - 1.0)
         / np.float64(lf)).astype(np.float32)
    got = gpu.iterate_fft(image, kernel, 1e-3, 0.006)
    assert np.abs(got - t).max() <= 2e-6 * np.abs(t).max()


@pytest.mark.gpu
def test_batched_forward_matches_single_and_numpy(gpu):
    # bench/bench_gpu_many_nd_fft.cu:403-463: V stacks of one shape through one plan
    rng = np.random.default_rng(11)
    for shape in ((8, 12, 10), (16, 16, 18), (5, 6, 7)):
        stacks = rng.standard_normal((3,) + shape).astype(np.float32)
        many = gpu.rfft3_many(stacks)
        assert many.shape == (3,) + shape[:2] + (shape[2] // 2 + 1,)
        for b in range(3):
            assert np.array_equal(many[b], gpu.rfft3(stacks[b]))
            ref = np.fft.rfftn(stacks[b].astype(np.float64))
            assert np.abs(many[b] - ref).max() <= 2e-5 * np.abs(ref).max()
    assert gpu.fft3_many_time((8, 8, 8), 2, 0, 1) >= 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,V", [((64, 64, 128), 2), ((12, 10, 9), 2), ((128, 256, 64), 1)])
def test_slab_engine_one_rank_equals_resident_engine(gpu, shape, V):
    # with one rank the two all-to-all exchanges are plain copies A -> B and
    # B -> A; pack / dim0 pass / unpack must then reproduce the resident engine's sweep
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    D2D = 3
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=4)
    se = gpu.slab_engine(shape, 1, 0, V)
    for v in range(V):
        se.set_view(v, views[v], w[v], k1[v], k2[v])
    se.set_psi(psi0)
    a, b, an, bn = se.buffers()
    nm, nn = se.buffer_sizes()

    def copy(dst, src, n):
        # a device-to-device hipMemcpy may return before the copy has run, and the engine's stream is
        # non-blocking (no implicit ordering against the null stream): drain the device explicitly
        if n:
            assert hip.hipMemcpy(dst, src, n * 4, D2D) == 0
            assert hip.hipDeviceSynchronize() == 0

    its = 2
    for it in range(its):
        for v in range(V):
            for conv in (0, 1):
                se.pack(v, conv)
                se.sync()
                copy(b, a, nm)
                copy(bn, an, nn)
                se.mid(v, conv)
                se.sync()
                copy(a, b, nm)
                copy(an, bn, nn)
                se.unpack(v, conv, 0.006, 1e-4, not (it == its - 1 and v == V - 1))
    se.sync()
    got = se.get_psi()
    se.close()
    e = gpu.engine(shape, V)
    for v in range(V):
        e.set_view(v, views[v], w[v], k1[v], k2[v])
    e.set_psi(psi0)
    e.iterate(its, 0.006, 1e-4)
    e.sync()
    ref = e.get_psi()
    e.close()
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    # and against the CPU oracle of the reference's loop, not only against the resident engine
    from oracle import binding as orc
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, its)
    mx, rms = rel_err(got, orc.cpu_deconvolve(psi0, h, 4))
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


# (shared by the child, which replays captured sweeps, and the parent, which launches directly)
_GRAPH_RUNS = r"""
def graph_runs(lib, shape, np, realistic_views):
    V, its = 3, 6
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=12)
    e = lib.engine(shape, V)
    for v in range(V):
        e.set_view(v, views[v], w[v], k1[v], k2[v])
    out = []
    for lam in (0.006, 0.0, 0.0):      # second and third: re-capture on a parameter change, then re-use
        e.set_psi(psi0); e.iterate(its, lam, 1e-4); e.sync(); out.append(e.get_psi())
    # one Inf voxel: the flooded convolutions of a replayed sweep report under the epochs of the capture
    bad = psi0.copy(); bad[shape[0] // 2, 3, 3] = np.inf
    e.set_psi(bad); e.iterate(its, 0.0, 1e-4); e.sync(); out.append(e.get_psi())
    e.set_psi(psi0); e.iterate(its, 0.0, 1e-4); e.sync(); out.append(e.get_psi())  # and a clean run behind it
    # other PSFs of another depth on the same engine (ADVICE r03: the captured sweep holds the PSF buffers,
    # their form and their depth - it has to be captured again)
    _, _, k1b, k2b, _, _ = realistic_views(shape, V, (3, 5, 5), seed=13)
    for v in range(V):
        e.set_view(v, views[v], w[v], k1b[v], k2b[v])
    e.set_psi(psi0); e.iterate(its, 0.0, 1e-4); e.sync(); out.append(e.get_psi())
    e.close()
    return np.stack(out)
"""

_GRAPH_CHILD = _GRAPH_RUNS + r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from libmultiviewnative_amd import native
from ref_fixtures import realistic_views
shape = tuple(int(x) for x in sys.argv[3:6])
np.save(sys.argv[2], graph_runs(native.lib(), shape, np, realistic_views))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(32, 32, 32), (64, 64, 128), (24, 20, 18)])
def test_graph_replayed_sweeps_equal_direct_launches(gpu, shape, tmp_path, leg):
    # MVN_GRAPH=1 (opt-in): sweeps 2..n-1 of a call are replayed from a captured graph on small
    # volumes (Engine::iterate).  A child process runs with it, this process with direct launches;
    # same kernels in the same order, so the results must be bit-identical - with the fused FFT dim0 pass
    # (suite pin) and with the direct leg in pieces + packed Nyquist layout (product defaults), through a
    # non-finite voxel and across a change of PSF depth on the same engine.
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "graph.npy")
    env = dict(os.environ, MVN_GRAPH="1")  # (the fixture has already set / removed the pins in os.environ)
    subprocess.run([sys.executable, "-c", _GRAPH_CHILD, root, out] + [str(x) for x in shape],
                   check=True, env=env, timeout=300)
    got = np.load(out)
    ns = {}
    exec(_GRAPH_RUNS, ns)
    ref = ns["graph_runs"](gpu, shape, np, realistic_views)
    assert got.shape == ref.shape == (6,) + tuple(shape)
    for i in range(6):
        assert np.isfinite(ref[i]).sum() >= ref[i].size - 1, i  # (run 3 keeps its one NaN voxel)
        assert np.array_equal(got[i], ref[i], equal_nan=True), i
    assert not np.array_equal(ref[4], ref[5])  # the other PSFs were really used


@pytest.mark.gpu
def test_long_lines_use_the_split_window_kernels(gpu):
    # lines above 1024 keep 16-column tiles by holding the tile in registers and running the inner
    # stages on half of it at a time (mvn_fixed.hpp, FxSplitCfg); inverse passes by default
    rng = np.random.default_rng(3)
    for shape in ((2, 1920, 64), (1280, 16, 64)):
        x = rng.standard_normal(shape).astype(np.float32)
        c0 = gpu.l.mvn_split_launch_count()
        spec = gpu.rfft3(x)
        y = gpu.irfft3(spec, shape[2])
        assert gpu.l.mvn_split_launch_count() - c0 >= 1
        ref = np.fft.rfftn(x.astype(np.float64))
        assert np.abs(spec - ref).max() <= 2e-6 * np.abs(ref).max()
        assert np.abs(y / x.size - x).max() <= 1e-5


# ---- round 2: non-trivial data on the HEADLINE kernel instantiations, BASELINE configs[3] / [4] ----
@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("shape", [(512, 32, 64), (512, 64, 512)])
def test_headline_instantiations_vs_oracle(gpu, orc, shape, lam):
    # kx_strided<512, FWD_MUL_INV> (the LDS-fused dim0 body: the bench's dominant kernel),
    # kx_strided<512, *> and, for d2 = 512, kx_rows_c2r_r2c<256, DIVIDE / UPDATE>, on blobs + PSFs
    info = gpu.plan_describe(shape)
    assert info["fx_ax0"] == 1 and info["fx_rows"] == 1
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (9, 7, 11), seed=3)
    h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 2)
    got = gpu.gpu_deconvolve(psi0, h)
    ref = orc.cpu_deconvolve(psi0, h, -1)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)
    assert float(((got.astype(np.float64) - ref) ** 2).sum()) < 1  # tests/test_gpu_deconvolve_impl.cu:200


def test_full_size_512_six_views_vs_oracle(gpu, orc):
    # BASELINE.json configs[2] at FULL size on non-trivial data: 512^3, 6 views, 31^3 PSFs, one
    # sequential sweep through the resident engine vs the oracle (about half a minute of CPU)
    from ref_fixtures import structured_views
    shape, V = (512, 512, 512), 6
    views, k1, k2, w, psi0 = structured_views(shape, V, (31, 31, 31))
    eng = gpu.engine(shape, V)
    for v in range(V):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    eng.iterate(1, 0.006, 1e-4)
    got = eng.get_psi()
    eng.close()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
    ref = orc.cpu_deconvolve(psi0, h, -1)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)
    assert np.abs(got - psi0).max() > 1e-2 * np.abs(psi0).max()  # the sweep did change psi


def _record(name, rows):
    """full-length parity figures for BASELINE.md section 3 (gpurun_out/ travels back from the GPU box)"""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "full_length_parity_%s.json" % name), "w") as f:
            json.dump(rows, f, indent=1)
    except OSError:
        pass
    print(name, rows)


def _full_length(gpu, orc, shape, V, kshape, checkpoints, seed):
    """Resident engine vs oracle over BASELINE's full iteration count, compared at `checkpoints`
    (cumulative sweeps): the oracle continues from its own previous result (N iterations == N x 1
    iteration, tests/test_oracle_deconvolve.py), the engine from its own."""
    from ref_fixtures import structured_views
    views, k1, k2, w, psi0 = structured_views(shape, V, kshape, seed=seed)
    eng = gpu.engine(shape, V)
    for v in range(V):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    ref, done, rows = psi0, 0, []
    n_ref = 64.0 ** 3  # the reference accepts sum(d^2) < 1 on its fixture volume; scaled per voxel of a 64^3 block
    for upto in checkpoints:
        eng.iterate(upto - done, 0.006, 1e-4)
        got = eng.get_psi()
        h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, upto - done)
        ref = orc.cpu_deconvolve(ref, h, -1)
        done = upto
        mx, rms = rel_err(got, ref)
        ssd = float(((got.astype(np.float64) - ref) ** 2).sum())
        rows.append({"sweeps": upto, "max_rel": mx, "rms_rel": rms, "sum_sq_diff": ssd,
                     "sum_sq_diff_per_64cubed": ssd * n_ref / got.size})
        assert mx <= MAX_REL and rms <= RMS_REL, rows
        # tests/test_gpu_deconvolve_impl.cu:200,260,323 (sum of squared differences < 1 after 2 / 5 / 10
        # iterations), scaled to the volume
        assert ssd * n_ref / got.size < 1, rows
    eng.close()
    assert np.abs(got - psi0).max() > 1e-2 * np.abs(psi0).max()
    return rows


def test_full_length_config2_512_six_views_ten_iterations_vs_oracle(gpu, orc):
    # BASELINE.json configs[2] at FULL size AND full length: 512^3, 6 views, 31^3 PSFs, 10 sequential
    # sweeps, compared after 1 / 5 / 10 (error growth over 60 Gauss-Seidel view updates); about a
    # minute of oracle time on the box's cores
    _record("config2", _full_length(gpu, orc, (512, 512, 512), 6, (31, 31, 31), (1, 5, 10), seed=7))


def test_full_length_config4_kernels_six_views_twenty_iterations_vs_oracle(gpu, orc):
    # BASELINE.json configs[4]'s kernels at its full length: a 16-plane slab of 320 x 1920 x 1920
    # (1920-lines, 960-bin rows, split-window passes), 6 views, 20 sweeps, compared after 1 / 10 / 20
    shape = (16, 1920, 1920)
    info = gpu.plan_describe(shape)
    assert info["fx_rows"] == 1 and info["fx_ax1"] == 1
    _record("config4", _full_length(gpu, orc, shape, 6, (9, 31, 31), (1, 10, 20), seed=5))


def test_config3_eight_views_simultaneous_512_vs_oracle(gpu, orc):
    # BASELINE.json configs[3] on ONE GPU: 512^3, 8 views, simultaneous (Jacobi) update -- what the 8
    # ranks of the sharded run compute together -- in 4 dim0 chunks (the overlapped form), one
    # iteration vs oracle_deconvolve_simultaneous
    from ref_fixtures import structured_views
    shape, V = (512, 512, 512), 8
    views, k1, k2, w, psi0 = structured_views(shape, V, (31, 31, 31), seed=11, terms=3)
    eng = gpu.engine(shape, V)
    for v in range(V):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    n = eng.delta_chunks(4)
    assert n == 4
    eng.compute_delta_head(0.006, 1e-4)
    for c in range(n):
        eng.compute_delta_chunk(c, n)
    for c in range(n):
        eng.apply_delta_chunk(c, n, False)
    got = eng.get_psi()
    eng.close()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, -1)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


def test_config4_long_line_kernels_vs_oracle(gpu, orc):
    # BASELINE.json configs[4]'s kernels (1920-long lines on dim1, 960-bin last-axis tiles, the
    # split-window passes) on non-trivial data: a 16-plane slab of the 320 x 1920 x 1920 shape
    from ref_fixtures import structured_views
    shape = (16, 1920, 1920)
    info = gpu.plan_describe(shape)
    assert info["fx_rows"] == 1 and info["fx_ax1"] == 1
    views, k1, k2, w, psi0 = structured_views(shape, 1, (9, 31, 31), seed=5)
    c0 = gpu.l.mvn_split_launch_count()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    got = gpu.gpu_deconvolve(psi0, h)
    assert gpu.l.mvn_split_launch_count() > c0
    ref = orc.cpu_deconvolve(psi0, h, -1)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


def test_full_size_config4_one_view_vs_oracle(gpu, orc):
    # BASELINE.json configs[4] at its full extent on non-trivial data: 320 x 1920 x 1920, one view,
    # one iteration (4.7 GB per stack; the dim0 = 320 fused pass, 1920-lines with 61440 tiles per
    # launch, 614400 rows of 960 bins) against the oracle on the host cores
    from ref_fixtures import structured_views
    shape = (320, 1920, 1920)
    info = gpu.plan_describe(shape)
    assert info["fx_rows"] == 1 and info["fx_ax1"] == 1 and info["fx_ax0"] == 1
    views, k1, k2, w, psi0 = structured_views(shape, 1, (31, 31, 31), seed=11)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
    got = gpu.gpu_deconvolve(psi0, h)
    gpu.check(gpu.l.mvn_release_cached_engines())
    ref = orc.cpu_deconvolve(psi0, h, -1)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


@pytest.mark.parametrize("shape,chunks", [((64, 64, 64), 4), ((24, 20, 18), 3), ((12, 10, 9), 5)])
def test_chunked_simultaneous_steps_vs_oracle(gpu, orc, shape, chunks, leg):
    # the overlapped form of the sharded step on one rank, several iterations with the spectrum of
    # psi handed from apply_delta_chunk to the next compute_delta_head
    from libmultiviewnative_amd.sharded import SimultaneousDriver
    _, views, k1, k2, w, psi0 = realistic_views(shape, 3, (5, 5, 5), seed=8)
    eng = gpu.engine(shape, 3)
    for v in range(3):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    n = eng.delta_chunks(chunks)
    assert n >= 2
    for it in range(3):
        eng.compute_delta_head(0.006, 1e-4)
        for c in range(n):
            eng.compute_delta_chunk(c, n)
        for c in range(n):
            eng.apply_delta_chunk(c, n, it < 2)
    got = eng.get_psi()
    # and through the driver without a process group (one chunk, no collective)
    eng.set_psi(psi0)
    SimultaneousDriver(eng, None, None).run(3, 0.006, 1e-4)
    again = eng.get_psi()
    eng.close()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 4)
    for x in (got, again):
        mx, rms = rel_err(x, ref)
        assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)
    assert np.array_equal(got, again)  # same kernels on row / plane ranges


def _bench_problem(shape, V, psf_edge):
    import bench
    views, k1, k2 = [], [], []
    for v in range(V):
        a, b, c = bench.make_view(shape, v, psf_edge)
        views.append(a)
        k1.append(b)
        k2.append(c)
    w = [np.full(shape, 1.0 / V, np.float32)] * V
    psi0 = np.full(shape, np.float32(bench.start_value()), np.float32)
    return views, k1, k2, w, psi0


@pytest.mark.parametrize("launch", ["two_ranks_gloo", "one_rank_nccl", "two_ranks_gloo_hostsync",
                                    "two_ranks_gloo_with_exact_halo_mode"])
def test_bench_multi_rank_launch_path_vs_oracle(gpu, orc, tmp_path, launch):
    # `python bench.py --gpus 2 ...` exactly as typed (the parent spawns the ranks itself): 64^3, 3
    # views split 2 + 1 over two ranks that share device 0 (gloo; RCCL refuses two ranks on one
    # GPU), chunked all-reduce ordered by stream events / by host synchronisation; and the RCCL
    # path on one rank (--force-dist).  Result vs oracle_deconvolve_simultaneous.
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = str(tmp_path / "psi.npy")
    shape, V, psf, its = (64, 64, 64), 3, 9, 3
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--size", "64", "64", "64", "--views", str(V),
           "--psf", str(psf), "--steps", str(its), "--warmup", "0", "--no-profile", "--dump-psi", dump]
    exact = launch.endswith("exact_halo_mode")
    cmd += ["--full"] if exact else ["--no-side"]
    if launch == "one_rank_nccl":
        cmd += ["--gpus", "1", "--force-dist", "--backend", "nccl"]
    else:
        cmd += ["--gpus", "2", "--backend", "gloo", "--all-ranks-on-device", "0"]
        if launch.endswith("hostsync"):
            cmd += ["--host-sync"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    if exact:
        # what an N > 1 line adds when the ranks sit on their own GPUs: rank 0 starts the slab mode over all devices
        # as a child process with a time limit while the other ranks wait on the host; here both "devices" are GPU 0
        env["MVN_BENCH_EXACT_DEVICES"] = "0,0"
        for k in ("MVN_DIM0_DIRECT_MIN_ITEMS", "MVN_DIM0_DIRECT_MIN_PLANE"):
            env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    # the driver's contract: rank 0's stdout carries ONE JSON line and nothing else (RCCL's version
    # banner, which it prints on stdout, is routed to stderr by bench.py)
    line = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(line) == 1 and line[0].startswith("{"), r.stdout[-2000:]
    out = json.loads(line[0])
    assert out["n_gpus"] == (1 if launch == "one_rank_nccl" else 2) and out["scaling"] == "strong"
    assert out["config"]["views_total"] == V and out["psi_finite_positive"]
    if launch != "one_rank_nccl":
        assert out["config"]["views_per_rank"] == [2, 1]
    assert "Jacobi" in out["config"]["update_mode"]
    if exact:
        e = out["exact_halo_mode"]
        assert "error" not in e, e
        assert e["devices"] == [0, 0] and e["parity"]["bit_equal"] and e["psi_finite_positive"], e
    got = np.load(dump)
    views, k1, k2, w, psi0 = _bench_problem(shape, V, psf)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, its)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, 4)
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)


@pytest.mark.parametrize("ranks", [1, 2])
def test_halo_slab_mode_vs_the_sequential_oracle(gpu, orc, tmp_path, ranks, monkeypatch):
    # tools/halo_bench.py: ONE volume on dim0 slabs (halo exchange before every dim0 leg) in the REFERENCE's update
    # order - one rank (cyclic self-exchange, device buffers) and two gloo ranks sharing device 0 (host staging)
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = str(tmp_path / "psi.npy")
    shape, V, psf, its = (64, 64, 64), 3, 9, 3
    cmd = [sys.executable, os.path.join(root, "tools", "halo_bench.py"), "--size", "64", "64", "64", "--views", str(V),
           "--psf", str(psf), "--steps", str(its), "--warmup", "0", "--dump-psi", dump]
    if ranks > 1:
        cmd += ["--ranks", str(ranks), "--backend", "gloo", "--all-ranks-on-device", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    out = json.loads(line[-1])
    assert out["n_gpus"] == ranks and out["psi_finite_positive"] and "reference order" in out["config"]["update_mode"]
    got = np.load(dump)
    views, k1, k2, w, psi0 = _bench_problem(shape, V, psf)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, its)
    ref = orc.cpu_deconvolve(psi0, h, 4)  # sequential sweep: the mode has no Jacobi deviation
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms)
    if ranks == 2:
        # the same two slabs inside ONE blocking ABI call (MVN_DEVICES=0,0: mvn_multi.cpp - host threads, events and
        # peer copies instead of processes and a communication library): the same kernels on the same values
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
        monkeypatch.setenv("MVN_DEVICES", "0,0")
        gpu.check(gpu.l.mvn_release_cached_engines())
        before = gpu.l.mvn_multi_device_calls()
        in_process = gpu.gpu_deconvolve(psi0, h)
        assert gpu.l.mvn_multi_device_calls() == before + 1
        gpu.check(gpu.l.mvn_release_cached_engines())
        assert np.array_equal(in_process, got)


@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
def test_mvn_devices_runs_the_abi_call_as_halo_slabs(gpu, orc, monkeypatch, devices, pad):
    # VERDICT r03 missing 1: inplace_gpu_deconvolve (inc/multiviewnative.h:66-67) on several devices.  The pool
    # gives one GPU: the entries repeat device 0 (two / four slab engines, host threads and streams on one device;
    # peer copies become device copies) - against the one-device call BIT FOR BIT, against the sequential oracle
    # under both padding policies, through a non-finite voxel, and with the cached group of slab engines.
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        for shape, V, ks, its in (((48, 16, 32), 2, (7, 3, 5), 3), ((256, 64, 128), 2, (15, 7, 7), 2),
                                  ((128, 512, 64), 1, (31, 5, 5), 2)):
            _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=21)
            k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
            h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, its)
            monkeypatch.delenv("MVN_DEVICES", raising=False)
            single = gpu.gpu_deconvolve(psi0, h, pad_mode=pad)
            monkeypatch.setenv("MVN_DEVICES", devices)
            before = gpu.l.mvn_multi_device_calls()
            multi = gpu.gpu_deconvolve(psi0, h, pad_mode=pad)
            again = gpu.gpu_deconvolve(psi0, h, pad_mode=pad)
            assert gpu.l.mvn_multi_device_calls() == before + 2, shape
            assert np.array_equal(multi, single) and np.array_equal(again, single), shape
            if pad != "zero":  # ("zero" pads to FFT-friendly extents: covered by the bit-equality with one device)
                ref = (orc.cpu_deconvolve(psi0, h, 8) if pad == "none" else
                       _zero_padd_reference(orc, psi0, views, k1, k2, w, 0.006, 1e-4, its))
                mx, rms = rel_err(multi, ref)
                assert mx <= MAX_REL and rms <= RMS_REL, (shape, mx, rms)
            if pad == "none" and shape[0] == 48:
                bad = psi0.copy()
                bad[5, 5, 5] = np.inf
                assert np.array_equal(gpu.gpu_deconvolve(bad, h, pad_mode=pad), orc.cpu_deconvolve(bad, h, 4),
                                      equal_nan=True)
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_slabs_of_a_large_volume_keep_the_split_nyquist_layout(gpu, orc, monkeypatch):
    # Above 256 MB a volume keeps its Nyquist plane, whose dim1 lines ride in the main dim1 launches; the slabs of
    # MVN_DEVICES run that layout whatever their own size and exchange the plane's halo planes too.  Forced on small
    # volumes (MVN_NYQ_PACKED=0), d1 = 64 / 512 (fixed-length dim1 kernels with riders), d2 = 128 / 512 (tiled and
    # wave-row last-axis kernels): bit-equal to one engine, the oracle's flood through an Inf voxel.
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    monkeypatch.setenv("MVN_NYQ_PACKED", "0")
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        for shape, V, ks in (((48, 64, 128), 2, (7, 5, 3)), ((96, 512, 512), 1, (15, 5, 5))):
            _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=25)
            h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
            monkeypatch.delenv("MVN_DEVICES", raising=False)
            single = gpu.gpu_deconvolve(psi0, h)
            ref = orc.cpu_deconvolve(psi0, h, 8)
            mx, rms = rel_err(single, ref)
            assert mx <= MAX_REL and rms <= RMS_REL, (shape, mx, rms)
            modes = [None]
            if shape[1:] == (512, 512):
                # planes of 512 x 512: one device AND the slabs run the fused middle pass (csrc/mvn_mid_fused.hpp; the
                # group decides for all its slabs) - and both keep the three passes under MVN_MID_FUSED=0
                modes = ["fused", "three passes"]
            results = {}
            for mode in modes:
                if mode == "three passes":
                    monkeypatch.setenv("MVN_MID_FUSED", "0")
                    gpu.check(gpu.l.mvn_release_cached_engines())
                    single = gpu.gpu_deconvolve(psi0, h)
                results[mode] = single
                for devices in ("0,0", "0,0,0"):
                    monkeypatch.setenv("MVN_DEVICES", devices)
                    before = gpu.l.mvn_multi_device_calls()
                    c0 = gpu.l.mvn_mid_fused_launch_count()
                    multi = gpu.gpu_deconvolve(psi0, h)
                    assert gpu.l.mvn_multi_device_calls() == before + 1
                    assert (gpu.l.mvn_mid_fused_launch_count() > c0) == (mode == "fused"), (shape, devices, mode)
                    assert np.array_equal(multi, single), (shape, devices, mode)
                    monkeypatch.delenv("MVN_DEVICES")
            if len(modes) == 2:
                mx, rms = rel_err(results["three passes"], results["fused"])
                assert mx <= 1e-5 and rms <= 1e-6, (shape, mx, rms)
            monkeypatch.delenv("MVN_MID_FUSED", raising=False)
            # an Inf voxel met by ONE slab's leg / middle pass floods every slab's volume (poison words of the peers)
            gpu.check(gpu.l.mvn_release_cached_engines())
            monkeypatch.setenv("MVN_DEVICES", "0,0,0")
            bad = psi0.copy()
            bad[5, 5, 5] = np.inf
            assert np.array_equal(gpu.gpu_deconvolve(bad, h), orc.cpu_deconvolve(bad, h, -1), equal_nan=True), shape
            monkeypatch.delenv("MVN_DEVICES")
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
        monkeypatch.delenv("MVN_MID_FUSED", raising=False)
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_psf_cache_invalidation_on_gpu(gpu, orc):
    # SURVEY.md 8f row 3 on the device: block-after-block calls re-use the resident PSF spectra; the
    # same shape with changed kernel bytes must prepare them again and give the oracle's result
    shape = (32, 24, 40)
    rng = np.random.default_rng(5)
    _, views, k1, k2, w, _ = realistic_views(shape, 2, (5, 5, 5), seed=9)
    gpu.check(gpu.l.mvn_release_cached_engines())

    def run(vs, a, b):
        h = WorkspaceHolder(vs, a, b, w, lambda_=0.006, min_value=1e-4, iterations=2)
        psi0 = np.full(shape, np.float32(vs[0].mean()), np.float32)
        mx, rms = rel_err(gpu.gpu_deconvolve(psi0, h), orc.cpu_deconvolve(psi0, h, 2))
        assert mx <= MAX_REL and rms <= RMS_REL

    h0, m0 = gpu.psf_cache_counters()
    run(views, k1, k2)
    h1, m1 = gpu.psf_cache_counters()
    assert (h1 - h0, m1 - m0) == (0, 4)
    other = [(v * rng.uniform(0.5, 1.5, shape)).astype(np.float32) for v in views]
    run(other, k1, k2)  # new stacks, same PSFs: every spectrum re-used
    h2, m2 = gpu.psf_cache_counters()
    assert (h2 - h1, m2 - m1) == (4, 0)
    k1b = [k * np.float32(0.5) for k in k1]  # same shape, every kernel1 byte changed
    run(other, k1b, k2)
    h3, m3 = gpu.psf_cache_counters()
    assert (h3 - h2, m3 - m2) == (2, 2)
    gpu.check(gpu.l.mvn_release_cached_engines())


def test_default_padding_policy_on_a_block(gpu, orc, leg):
    # the library default (zero_padd with FFT-friendly extents): a 50 x 60 x 70 block with 9^3 / 7^3
    # PSFs runs on a padded 64-ish volume and is cropped back; oracle on hand-padded stacks, guard on
    shape = (50, 60, 70)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (9, 9, 9), seed=2)
    k2 = [np.ascontiguousarray(k[1:8, 1:8, 1:8]) for k in k2]
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    got = gpu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert got.shape == shape and np.isfinite(got).all()
    # image + kernel - 1 = (58, 68, 78) -> good extents; the offsets stay (kernel - 1) / 2 = 4
    from ref_fixtures import expected_good_extent
    ext = [expected_good_extent(gpu, n, d == 2) for d, n in enumerate((58, 68, 78))]
    sl = tuple(slice(4, 4 + s) for s in shape)

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
    mx, rms = rel_err(got, ref)
    assert mx <= MAX_REL and rms <= RMS_REL, (mx, rms, ext)


_WAVE_ROWS_CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
for shape in [(6, 40, 512), (3, 16, 512)]:   # 240 / 48 rows (the fixed last-axis kernels take multiples of 16)
    assert gpu.plan_describe(shape)["fx_rows"] == 1
    x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    ref = np.fft.rfftn(x.astype(np.float64))
    got = gpu.rfft3(x)
    assert np.abs(got - ref).max() <= 5e-6 * np.abs(ref).max(), "r2c"
    back = gpu.irfft3(got, shape[2]) / np.float32(np.prod(shape))
    assert np.abs(back - x).max() < 2e-5, "c2r"
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (3, 5, 7), seed=3)
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
        got = gpu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), ("sequential", lam)
        e = gpu.engine(shape, 2)
        for v in range(2):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        for _ in range(2):
            e.compute_delta(lam, 1e-4)
            e.apply_delta()
        got = e.get_psi()
        e.close()
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 2)
        ref = orc.cpu_deconvolve_simultaneous(psi0, h, 4)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), ("simultaneous", lam)
print("wave-row child ok", os.environ.get("MVN_WAVE_ROWS_MASK"))
"""


@pytest.mark.parametrize("mask", ["31", "0"])
def test_wave_row_variants_in_a_child_process(gpu, mask):
    # the wave-row forms the default mask (28) leaves off -- plain r2c, plain c2r with the STORE /
    # DIVIDE / UPDATE epilogues -- and, with mask 0, the tiled kernels they replace, on the
    # GPU: the HIP backend reads MVN_WAVE_ROWS_MASK once per process, hence the child.  Only the
    # hardware can check what these kernels rely on (one wave's LDS instructions execute in order,
    # no workgroup barrier between the phases of a row).
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MVN_WAVE_ROWS_MASK=mask)
    r = subprocess.run([sys.executable, "-c", _WAVE_ROWS_CHILD, root], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0 and "wave-row child ok " + mask in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_submit_wait_pipelines_three_blocks_bit_for_bit(gpu):
    # SURVEY.md 8f row 3, second half: block k+1's stacks upload into the device's second resident
    # engine while block k iterates.  Three 128^3 blocks (6 views, 15^3 PSFs, 5 iterations) through
    # mvn_deconvolve_submit / mvn_deconvolve_wait == three blocking inplace_gpu_deconvolve calls, bit
    # for bit, under the default (zero-padding) policy and under the cyclic one
    shape, V = (128, 128, 128), 6
    blocks = []
    for b in range(3):
        _, views, k1, k2, w, psi0 = realistic_views(shape, V, (15, 15, 15), seed=40 + b)
        blocks.append((WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 5), psi0))
    before = gpu.get_pad_mode()
    try:
        for mode in ("zero", "none"):
            gpu.set_pad_mode(mode)
            want = [gpu.gpu_deconvolve(psi0, h, pad_mode=False) for h, psi0 in blocks]
            psis = [np.ascontiguousarray(psi0.copy()) for _, psi0 in blocks]
            tickets = [gpu.deconvolve_submit(psi, h) for psi, (h, _) in zip(psis, blocks)]
            for t in tickets:
                gpu.deconvolve_wait(t)
            for got, ref in zip(psis, want):
                assert np.isfinite(got).all() and np.array_equal(got, ref)
    finally:
        gpu.set_pad_mode(before)
        gpu.check(gpu.l.mvn_release_cached_engines())


_DIRECT_CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
worst = 0.0
for shape, kshape in [((64, 64, 64), (1, 5, 5)), ((64, 64, 64), (4, 5, 3)), ((96, 32, 64), (15, 7, 5)),
                      ((64, 48, 512), (21, 5, 9)), ((80, 24, 40), (33, 3, 3)), ((40, 13, 17), (9, 5, 3)),
                      ((4096, 4, 8), (3, 3, 3))]:  # (the last: beyond the packed layout's dim0 limit)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, kshape, seed=sum(kshape))
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
        got = gpu.gpu_deconvolve(psi0, h)
        ref = orc.cpu_deconvolve(psi0, h, 8)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        worst = max(worst, err)
        assert err <= 1e-4, (shape, kshape, lam, err)
    e = gpu.engine(shape, 2)
    for v in range(2):
        e.set_view(v, views[v], w[v], k1[v], k2[v])
    e.set_psi(psi0)
    for _ in range(2):
        e.compute_delta(0.006, 1e-4)
        e.apply_delta()
    got = e.get_psi()
    e.close()
    ref = orc.cpu_deconvolve_simultaneous(psi0, WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2), 8)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), ("simultaneous", shape, kshape)
# a non-finite voxel floods the volume as the FFT leg does
shape = (48, 16, 32)
_, views, k1, k2, w, psi0 = realistic_views(shape, 1, (5, 3, 3), seed=8)
psi_bad = psi0.copy(); psi_bad[5, 5, 5] = np.inf
h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
assert np.array_equal(gpu.gpu_deconvolve(psi_bad, h), orc.cpu_deconvolve(psi_bad, h, 2), equal_nan=True)
print("direct child ok", os.environ.get("MVN_DIM0_DIRECT"), "%.2e" % worst)
"""


@pytest.mark.parametrize("direct", ["1", "0", "1 packed", "1 product defaults"])
def test_direct_dim0_leg_in_a_child_process(gpu, direct):
    # mvn_dim0_direct.hpp on the GPU: PSF depths 1 .. 33 (odd, even, the largest instantiated), d2 = 512
    # wave-row shapes and odd extents, sequential and simultaneous loops, against the oracle -- and the
    # same cases with the leg switched off (fused FFT pass), which is what deeper PSFs (31 planes: the
    # headline) run by default.  Child processes: the switches are read when an engine is created.
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # "1": the default (separate Nyquist plane under the direct leg); "1 packed": MVN_NYQ_PACKED=1, the Nyquist
    # bins packed into the DC column and separated inside the direct leg (no Nyquist launches, one stream)
    env = dict(os.environ, MVN_DIM0_DIRECT=direct[0], MVN_DIM0_DIRECT_MAX="33", MVN_DIM0_DIRECT_MIN_PLANE="0", MVN_DIM0_DIRECT_MIN_ITEMS="0",
               MVN_NYQ_PACKED="1" if "packed" in direct else "0")
    if "defaults" in direct:  # what a host program gets: the leg at every size, columns in pieces, packed Nyquist
        for k in ("MVN_DIM0_DIRECT_MIN_PLANE", "MVN_DIM0_DIRECT_MIN_ITEMS", "MVN_NYQ_PACKED", "MVN_DIM0_DIRECT_MAX"):
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _DIRECT_CHILD, root], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "direct child ok " + direct[0] in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("env", [{}, {"MVN_NYQ_PACKED": "0"}, {"MVN_DIM0_DIRECT_MIN_PLANE": "250"}],
                         ids=["product defaults", "split nyquist", "short pieces"])
def test_nonfinite_voxel_floods_the_volume_in_every_form_of_the_direct_leg(gpu, monkeypatch, env):
    # one Inf voxel in the middle of a PIECE of a column (the product default below 512 x 512
    # planes), in psi and in a view, sequential and simultaneous, 1 and 2 iterations, WITHOUT the suite's pins -
    # identical to the oracle (whose FFT convolution floods the volume, inc/cpu_convolve.h:256-268).  The leg
    # reports the value in the engine's poison word and the last-axis pass that ends the convolution emits NaN.
    from nonfinite_util import nonfinite_cases
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        cases = [((192, 16, 32), (5, 3, 3), (100, 5, 5)), ((256, 16, 32), (5, 3, 3), (100, 5, 5)),
                 ((64, 10, 12), (5, 3, 3), (5, 5, 5))]
        if not env:
            cases.append(((256, 256, 256), (15, 15, 15), (100, 50, 60)))  # BASELINE configs[1]'s shape: 4 pieces
        for shape, kshape, pos in cases:
            nonfinite_cases(gpu, shape, kshape, pos, nviews=1 if shape[1] == 256 else 2)
    finally:
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_default_policy_keeps_dim0_exact_under_the_direct_leg(gpu, orc, monkeypatch):
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_PLANE", "0")
    monkeypatch.setenv("MVN_DIM0_DIRECT_MIN_ITEMS", "0")  # read per call / per engine
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
        return gpu.l.mvn_plan_store_has_key(0, (ctypes.c_int * 3)(*ext)) == 1

    gpu.l.mvn_release_cached_engines()
    gpu.check(gpu.l.mvn_plan_store_clear())
    got = gpu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert expected_good_extent(gpu, 32, False) == 32 and expected_good_extent(gpu, 32, True) == 32
    assert has_plan((23, 32, 32)) and not has_plan((24, 32, 32))
    exact, rounded = reference((23, 32, 32)), reference((24, 32, 32))
    assert np.abs(got - exact).max() <= 1e-4 * np.abs(exact).max()
    # (the extra plane holds zeros the guarded quotient never lets in: the two paddings agree to rounding)
    assert np.abs(exact - rounded).max() <= 1e-5 * np.abs(exact).max()
    gpu.check(gpu.l.mvn_release_cached_engines())


def test_headline_path_is_deterministic_and_matches_the_fft_leg(gpu):
    # (96, 512, 512) x 2 views x 31-plane PSFs: the shape class of the headline - planes of 512 x 512, where the
    # three middle passes run as ONE (csrc/mvn_mid_fused.hpp; round 3 / first half of round 4: the direct dim0 leg
    # between two dim1 passes).  Two runs from the same psi are bit-identical (no atomics, no order dependence), and
    # the result agrees to rounding with the three-pass middle (MVN_MID_FUSED=0: direct leg) and with the fused FFT
    # leg (MVN_DIM0_DIRECT=0) of the same library, each in a child process (the switches are read per engine, the
    # kernels' A/B knobs once per process).
    import subprocess
    import sys
    shape, V = (96, 512, 512), 2
    from ref_fixtures import structured_views
    views, k1, k2, w, psi0 = structured_views(shape, V, (31, 9, 9), seed=3)

    def run():
        e = gpu.engine(shape, V)
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        e.profile(True)
        e.iterate(4, 0.006, 1e-4)
        e.sync()
        kinds = {n for n, (t, c) in e.profile_read().items() if c}
        e.profile(False)
        out = e.get_psi()
        e.close()
        return out, kinds

    a, kinds = run()
    b, _ = run()
    assert "mid_fused" in kinds and not {"axis0_direct", "axis0_fused", "axis1_fwd", "axis1_inv"} & kinds, kinds
    assert np.array_equal(a, b)
    code = ("import os, sys, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
            "from libmultiviewnative_amd import native\n"
            "from ref_fixtures import structured_views\n"
            "g = native.lib(); shape, V = (96, 512, 512), 2\n"
            "views, k1, k2, w, psi0 = structured_views(shape, V, (31, 9, 9), seed=3)\n"
            "e = g.engine(shape, V)\n"
            "[e.set_view(v, views[v], w[v], k1[v], k2[v]) for v in range(V)]\n"
            "e.set_psi(psi0); e.iterate(4, 0.006, 1e-4); np.save(sys.argv[1], e.get_psi()); e.close()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for tag, env in (("fft", {"MVN_DIM0_DIRECT": "0"}), ("three", {"MVN_MID_FUSED": "0"})):
            out = os.path.join(d, tag + ".npy")
            r = subprocess.run([sys.executable, "-c", code % (root, root), out], capture_output=True, text=True,
                               timeout=600, env=dict(os.environ, **env))
            assert r.returncode == 0, r.stderr[-3000:]
            mx, rms = rel_err(a, np.load(out))
            assert mx <= 1e-5 and rms <= 1e-6, (tag, mx, rms)


# ---- round 4: the fused middle pass on the line layout (csrc/mvn_mid_fused.hpp) ----------------------------------
@pytest.mark.parametrize("shape,kshape", [((64, 512, 512), (31, 7, 5)), ((48, 512, 512), (16, 3, 3)),
                                          ((40, 512, 512), (9, 31, 31)), ((33, 512, 512), (2, 3, 3))])
def test_fused_middle_pass_on_the_line_layout_vs_oracle(gpu, orc, monkeypatch, shape, kshape):
    # 512 x 512 planes, PSFs of at most 31 planes: the sequential sweep runs last-axis pass -> ONE middle pass (dim1
    # forward, K-tap direct convolution along dim0, dim1 inverse) -> last-axis pass on a half-spectrum whose lines
    # along dim1 are contiguous, Nyquist bins packed into the DC column (replaces inc/gpu_convolve.cuh:113-142 for
    # these shapes).  Through the ABI call (pipelined staging: the form is decided from the kernels' extents before
    # the last view has arrived) and through a resident engine; MVN_MID_FUSED=0 = the three-pass middle.
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")  # (by default only for volumes of at least three PSF depths of planes)
    gpu.check(gpu.l.mvn_release_cached_engines())
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, kshape, seed=61)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    got = None
    for lam in (0.0, 0.006):
        h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
        c0 = gpu.l.mvn_mid_fused_launch_count()
        got = gpu.gpu_deconvolve(psi0, h)
        assert gpu.l.mvn_mid_fused_launch_count() - c0 == 3 * 2 * 2  # iterations x views x convolutions
        ref = orc.cpu_deconvolve(psi0, h, -1)
        mx, rms = rel_err(got, ref)
        assert mx <= 1e-5 and rms <= 1e-6, (shape, kshape, lam, mx, rms)
    eng = gpu.engine(shape, 2)
    for v in range(2):
        eng.set_view(v, views[v], w[v], k1[v], k2[v])
    eng.set_psi(psi0)
    c0 = gpu.l.mvn_mid_fused_launch_count()
    eng.iterate(3, 0.006, 1e-4)
    res = eng.get_psi()
    eng.close()
    assert gpu.l.mvn_mid_fused_launch_count() - c0 == 12
    assert np.array_equal(res, got)  # same passes, same order: bit for bit
    monkeypatch.setenv("MVN_MID_FUSED", "0")
    gpu.check(gpu.l.mvn_release_cached_engines())
    c0 = gpu.l.mvn_mid_fused_launch_count()
    three = gpu.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3))
    assert gpu.l.mvn_mid_fused_launch_count() == c0
    mx, rms = rel_err(three, got)
    assert mx <= 1e-5 and rms <= 1e-6, (mx, rms)
    gpu.check(gpu.l.mvn_release_cached_engines())


@pytest.mark.parametrize("k0,d0", [(1, 12), (5, 29), (11, 24), (13, 40), (21, 33), (27, 38), (29, 39)])
def test_fused_middle_pass_other_tap_counts_vs_oracle(gpu, orc, monkeypatch, k0, d0):
    # the tap-count templates of kf_mid<K> the cases above do not reach (tools/fuzz_mid_fused.py walks all 31 depths)
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    gpu.check(gpu.l.mvn_release_cached_engines())
    shape, kshape = (d0, 512, 512), (k0, 3, 3)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, kshape, seed=100 + k0)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    c0 = gpu.l.mvn_mid_fused_launch_count()
    got = gpu.gpu_deconvolve(psi0, h)
    assert gpu.l.mvn_mid_fused_launch_count() - c0 == 2 * 2 * 2  # iterations x views x convolutions
    mx, rms = rel_err(got, orc.cpu_deconvolve(psi0, h, -1))
    assert mx <= 1e-5 and rms <= 1e-6, (k0, d0, mx, rms)
    gpu.check(gpu.l.mvn_release_cached_engines())


def test_fused_middle_pass_nonfinite_voxel_and_fallbacks(gpu, orc, monkeypatch):
    # one Inf voxel (in psi, in a view) floods the volume through the fused middle pass as it does through an FFT
    # along dim0 (inc/cpu_convolve.h:256-268 + inc/cpu_kernels.h:40-47,76-83); the simultaneous step of the same
    # shape keeps the three-pass middle (nonfinite_cases runs both loops); a PSF deeper than 31 planes falls back
    from nonfinite_util import nonfinite_cases
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        c0 = gpu.l.mvn_mid_fused_launch_count()
        nonfinite_cases(gpu, (48, 512, 512), (15, 3, 3), (20, 100, 7))
        assert gpu.l.mvn_mid_fused_launch_count() > c0
        shape = (48, 512, 512)
        _, views, k1, k2, w, psi0 = realistic_views(shape, 1, (33, 3, 3), seed=62)
        h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
        c0 = gpu.l.mvn_mid_fused_launch_count()
        got = gpu.gpu_deconvolve(psi0, h)
        assert gpu.l.mvn_mid_fused_launch_count() == c0
        mx, rms = rel_err(got, orc.cpu_deconvolve(psi0, h, -1))
        assert mx <= 1e-5 and rms <= 1e-6, (mx, rms)
    finally:
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_fused_middle_pass_in_the_simultaneous_loop(gpu, orc):
    # the simultaneous (Jacobi) step - what every rank of the view-sharded run computes - on 512 x 512 planes: psi's
    # last-axis spectrum once per step in the line layout, per view ONE middle pass -> fused divide -> ONE middle pass
    # -> correction; whole steps and the chunked form (next step's spectrum fed chunk by chunk) against the oracle's
    # simultaneous loop (test_config3_eight_views_simultaneous_512_vs_oracle runs the same path at full size)
    shape, V = (48, 512, 512), 3
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (15, 5, 3), seed=63)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    ref = orc.cpu_deconvolve_simultaneous(psi0, h, -1)
    e = gpu.engine(shape, V)
    try:
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        c0 = gpu.l.mvn_mid_fused_launch_count()
        for _ in range(2):
            e.compute_delta(0.006, 1e-4)
            e.apply_delta()
        assert gpu.l.mvn_mid_fused_launch_count() - c0 == 2 * V * 2
        whole = e.get_psi()
        mx, rms = rel_err(whole, ref)
        assert mx <= 1e-5 and rms <= 1e-6, (mx, rms)
        e.set_psi(psi0)
        n = e.delta_chunks(4)
        for _ in range(2):
            e.compute_delta_head(0.006, 1e-4)
            for c in range(n):
                e.compute_delta_chunk(c, n)
            for c in range(n):
                e.apply_delta_chunk(c, n, True)
        assert np.array_equal(e.get_psi(), whole)
    finally:
        e.close()


def test_default_padding_policy_reaches_the_fused_middle_pass(gpu, orc):
    # blocks whose rows and columns pad to 512 - 482 + 31 - 1 - run the fused middle pass under the library's DEFAULT
    # policy (zero padding to FFT-friendly extents, dim0 exact under the direct leg: inc/padd_utils.h:121-138 as the
    # reference's GPU entry applies it): what a host program that sizes its blocks for it gets; oracle on hand-padded
    # stacks, guard on
    shape, ks = (40, 482, 482), (9, 31, 31)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, ks, seed=2)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    gpu.check(gpu.l.mvn_release_cached_engines())
    c0 = gpu.l.mvn_mid_fused_launch_count()
    got = gpu.gpu_deconvolve(psi0, h, pad_mode=False)
    assert gpu.l.mvn_mid_fused_launch_count() - c0 == 3 * 2 * 2
    ext, off = (48, 512, 512), (4, 15, 15)
    sl = tuple(slice(o, o + s) for o, s in zip(off, shape))

    def embed(x):
        out = np.zeros(ext, np.float32)
        out[sl] = x
        return out

    hp = WorkspaceHolder([embed(v) for v in views], k1, k2, [embed(x) for x in w], 0.006, 1e-4, 3)
    orc.set_quotient_guard(True)
    try:
        ref = orc.cpu_deconvolve(embed(psi0), hp, -1)[sl]
    finally:
        orc.set_quotient_guard(False)
    mx, rms = rel_err(got, ref)
    assert mx <= 1e-5 and rms <= 1e-6, (mx, rms)
    gpu.check(gpu.l.mvn_release_cached_engines())
