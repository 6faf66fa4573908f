"""Derived kernels on the host emulation (csrc/mvn_psf.hpp; the emulation runs the passes' own bodies): the extents rule
on the header's table, kernel1 against mvn_resample_stack's image of the stated geometry, kernel2 of all four types
against the numpy restatement of the definition within 1 unit in the last place, the surface of mvn_derive_kernels, and
mvn_deconvolve_resampled with derivation on against the same call with the derived arrays handed in - under all four
padding policies and for all four types - block after block, and on its errors.  The checks live in psf_reference.py;
test_gpu_psf.py runs them on the device."""
import os
import subprocess

import pytest

from libmultiviewnative_amd import native
import psf_reference as pr
import resample_reference as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")
NEW = ("mvn_psf_extents", "mvn_derive_kernels", "mvn_set_kernel_derivation", "mvn_get_kernel_derivation",
       "mvn_derive_counters", "mvn_derive_time")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    b = native.Binding(native.EMU_SO)
    yield b
    b.l.mvn_release_cached_engines()


def test_symbols_declared_exported_bound(emu):
    hdr = open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read()
    exports = open(os.path.join(CSRC, "mvn_exports.map")).read()
    for n in NEW:
        assert n in native.ENGINE_ABI_SYMBOLS
        assert "MVN_API int %s(" % n in hdr, n
        assert "%s;" % n in exports, n
        assert hasattr(emu.l, n)


def test_extents(emu):
    pr.check_extents(emu)


@pytest.mark.parametrize("name", sorted(pr.GROUPS))
def test_kernel1(emu, name):
    pr.check_kernel1(emu, name)


@pytest.mark.parametrize("type_", pr.TYPES, ids=pr.TYPE_NAMES)
@pytest.mark.parametrize("name", sorted(pr.GROUPS))
def test_kernel2(emu, name, type_):
    pr.check_kernel2(emu, name, type_)


@pytest.mark.parametrize("type_", (1, 2), ids=pr.TYPE_NAMES[1:3])
def test_psfs_with_exact_zeros(emu, type_):
    pr.check_kernel1(emu, "three views", zeros=True)
    pr.check_kernel2(emu, "three views", type_, zeros=True)


def test_identical_symmetric_views(emu):
    pr.check_identical_symmetric_views(emu)


def test_derive_errors_leave_the_outputs_untouched(emu):
    pr.check_derive_errors(emu)


@pytest.mark.parametrize("type_", pr.TYPES, ids=pr.TYPE_NAMES)
@pytest.mark.parametrize("mode", rs.PAD_MODES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call(emu, key, mode, type_):
    pr.check_call(emu, key, mode, type_)


@pytest.mark.parametrize("type_", pr.TYPES, ids=pr.TYPE_NAMES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call_without_padding_on_psfs_that_fit_the_block(emu, key, type_):
    assert pr.check_call(emu, key, "none", type_, pr.SMALL_PSFS) is not None


def test_the_types_give_different_results(emu):
    pr.check_types_differ(emu)


def test_block_after_block(emu):
    pr.check_block_after_block(emu)


def test_call_errors_leave_psi_untouched(emu):
    pr.check_call_errors_leave_psi_untouched(emu)


def test_time_utility(emu):
    before = emu.derive_counters()
    for type_, launches in ((0, 0), (1, 2), (2, 1), (3, 0)):
        ms = emu.derive_time(3, (3, 5, 7), type_, reps=2)
        assert ms[0] >= 0 and ms[1] >= 0
    after = emu.derive_counters()
    # per type: (1 + reps) derivations, and (1 + reps) runs of the correlation launches alone
    assert after[0] - before[0] == 2 * 3 * (2 + 1) and after[1:] == before[1:]
