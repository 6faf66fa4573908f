"""The direct dim0 leg (csrc/mvn_dim0_direct.hpp, kd_dim0<K>) and the fused middle pass (csrc/mvn_mid_fused.hpp, kf_mid<K>) on
the GPU with PSFs whose every tap counts and white images (tests/flat_psf_cases.py): against the float64 restatement,
within four times the C oracle's own distance to it.  Every PSF depth of both kernels, every form of the direct leg."""
import os

import pytest

import flat_psf_cases as fc

pytestmark = pytest.mark.gpu
TAG = "gpu"


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):  # fresh checkout on the GPU box: compile, never fall back
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()  # raises if the HIP library is missing: no fallback
    assert b.backend_name() == "hip-gfx950"
    return b


@pytest.fixture
def direct(gpu, monkeypatch):
    # no suite pins: MVN_DIM0_DIRECT_MIN_* are the product's defaults unless a form says otherwise
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    gpu.check(gpu.l.mvn_release_cached_engines())
    yield gpu
    gpu.check(gpu.l.mvn_release_cached_engines())


@pytest.fixture
def fused(gpu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")  # the fused pass on shallow volumes too
    gpu.check(gpu.l.mvn_release_cached_engines())
    yield gpu
    gpu.check(gpu.l.mvn_release_cached_engines())


# ---- the direct dim0 leg --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(fc.DIRECT_FORMS))
def test_direct_leg_every_depth(direct, monkeypatch, form):
    fc.direct_form(direct, monkeypatch, form, TAG)


@pytest.mark.parametrize("k", fc.SIMULTANEOUS_DEPTHS)
def test_direct_leg_in_the_simultaneous_loop(direct, k):
    fc.direct_simultaneous(direct, k, TAG)


@pytest.mark.parametrize("k", fc.DIRECT_ONE_HOT)
def test_direct_leg_one_hot_taps(direct, k):
    fc.direct_one_hot(direct, k, TAG)


def test_slabs_reject_a_psf_deeper_than_the_volume(direct, monkeypatch, capfd):
    fc.slabs_reject_a_psf_deeper_than_the_volume(direct, monkeypatch)
    assert "kernel extent must be in [1, image extent]" in capfd.readouterr().err


# ---- the fused middle pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", fc.MID_DEPTHS_GPU)
def test_fused_pass_depth(fused, k):
    fc.mid_case(fused, (fc.mid_d0(k), 512, 512), (k, 3, 3), 0.006 if k % 2 else 0.0, 6000 + k, TAG)


@pytest.mark.parametrize("k,d0", fc.MID_SHORT_WALKS)
def test_fused_pass_walk_shorter_than_a_batch(fused, k, d0):
    fc.mid_case(fused, (d0, 512, 512), (k, 3, 3), 0.006, 6500 + d0, TAG)


def test_fused_pass_wide_psf(fused):
    fc.mid_case(fused, fc.MID_WIDE[0], fc.MID_WIDE[1], 0.006, 6100, TAG)


def test_fused_pass_in_the_slab_form(fused, monkeypatch):
    fc.mid_slabs(fused, monkeypatch, TAG)


def test_fused_pass_in_the_simultaneous_loop(fused):
    fc.mid_simultaneous(fused, TAG)


@pytest.mark.parametrize("k,t1,t2", [(k, t1, t2) for k in fc.MID_ONE_HOT for t1, t2 in fc.one_hot_taps(k)])
def test_fused_pass_one_hot_taps(fused, k, t1, t2):
    fc.mid_one_hot(fused, k, t1, t2, TAG)
