"""Derived kernels on the MI355X (csrc/mvn_psf.hpp: k_psf_correlate, k_psf_sum, k_psf_scale, k_psf_pointwise, and
k_resample3d for the transform): the cases of test_emu_psf.py at the same small shapes on the real kernels - the extents
rule, kernel1 against mvn_resample_stack's image, kernel2 of all four types against the numpy restatement within 1 unit
in the last place, the surface, and mvn_deconvolve_resampled with derivation on against the same call with the derived
arrays handed in, block after block and on its errors.  The checks live in psf_reference.py."""
import os

import pytest

import psf_reference as pr
import resample_reference as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):  # fresh checkout on the GPU box: compile, never fall back
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    yield b
    b.check(b.l.mvn_release_cached_engines())


def test_extents(gpu):
    pr.check_extents(gpu)


@pytest.mark.parametrize("name", sorted(pr.GROUPS))
def test_kernel1(gpu, name):
    pr.check_kernel1(gpu, name)


@pytest.mark.parametrize("type_", pr.TYPES, ids=pr.TYPE_NAMES)
@pytest.mark.parametrize("name", sorted(pr.GROUPS))
def test_kernel2(gpu, name, type_):
    pr.check_kernel2(gpu, name, type_)


@pytest.mark.parametrize("type_", (1, 2), ids=pr.TYPE_NAMES[1:3])
def test_psfs_with_exact_zeros(gpu, type_):
    pr.check_kernel1(gpu, "three views", zeros=True)
    pr.check_kernel2(gpu, "three views", type_, zeros=True)


def test_identical_symmetric_views(gpu):
    pr.check_identical_symmetric_views(gpu)


def test_derive_errors_leave_the_outputs_untouched(gpu):
    pr.check_derive_errors(gpu)


@pytest.mark.parametrize("type_", pr.TYPES, ids=pr.TYPE_NAMES)
@pytest.mark.parametrize("mode", rs.PAD_MODES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call(gpu, key, mode, type_):
    pr.check_call(gpu, key, mode, type_)


@pytest.mark.parametrize("type_", pr.TYPES, ids=pr.TYPE_NAMES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call_without_padding_on_psfs_that_fit_the_block(gpu, key, type_):
    assert pr.check_call(gpu, key, "none", type_, pr.SMALL_PSFS) is not None


def test_the_types_give_different_results(gpu):
    pr.check_types_differ(gpu)


def test_block_after_block(gpu):
    pr.check_block_after_block(gpu)


def test_call_errors_leave_psi_untouched(gpu):
    pr.check_call_errors_leave_psi_untouched(gpu)


def test_time_utility(gpu):
    before = gpu.derive_counters()
    for type_ in pr.TYPES:
        ms = gpu.derive_time(3, (3, 5, 7), type_, reps=2)
        assert ms[0] > 0 and (ms[1] > 0) == (type_ in (1, 2))
    after = gpu.derive_counters()
    assert after[0] - before[0] == 2 * 3 * (2 + 1) and after[1:] == before[1:]
