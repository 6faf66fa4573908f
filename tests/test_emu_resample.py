"""Resampled views on the host emulation (csrc/mvn_resample.hpp; the emulation runs the passes' own bodies): the pass
alone against the numpy restatement - the image bit for bit, the weights by their rule - for every case, element type
and layout of the raw stack; the call against the plain call on the library's own resampled stacks under all four
padding policies and against the CPU oracle; computed weights and the order of normalisation and mirror fill; block
after block on a cached engine; the loop's switches together; the public surface.  The checks live in
resample_reference.py; test_gpu_resample.py runs them on the device."""
import os
import subprocess

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_DEVICE
from oracle import binding as orc
import resample_reference as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    b = native.Binding(native.EMU_SO)
    yield b
    b.l.mvn_release_cached_engines()


def test_symbols_declared_exported_bound(emu):
    hdr = open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read()
    exports = open(os.path.join(CSRC, "mvn_exports.map")).read()
    for n in ("mvn_deconvolve_resampled", "mvn_deconvolve_memory_resampled", "mvn_engine_set_view_resampled",
              "mvn_engine_normalize_weights", "mvn_resample_stack", "mvn_resample_time", "mvn_resample_counters"):
        assert n in native.ENGINE_ABI_SYMBOLS
        assert "MVN_API int %s(" % n in hdr, n
        assert "%s;" % n in exports, n
        assert hasattr(emu.l, n)


def test_the_case_table_and_the_measured_tolerance():
    # the conditions on the table are asserted when the module is imported; the tolerance is measured, not chosen
    tol = rs.weight_tolerance()
    print("float32 formula against float64 over the cases: %.3g, allowed %.3g" % (rs._TOL["measured"], tol))
    assert 0 < tol < 1e-5


@pytest.mark.parametrize("layout", rs.LAYOUTS)
@pytest.mark.parametrize("dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("name", sorted(rs.CASES))
def test_pass_against_numpy(emu, name, dtype, layout):
    rs.check_stack(emu, name, dtype, layout)


@pytest.mark.parametrize("layout", rs.LAYOUTS)
@pytest.mark.parametrize("name", ["rotation by 30 degrees", "fractional shift"])
def test_pass_on_a_stack_described_as_device_memory(emu, name, layout):
    # (any pointer of the emulation may be called device memory: the pass then reads it where it lies, strides and all)
    rs.check_stack(emu, name, np.uint16, layout,
                   resample=lambda a, g, s: rs.resample_direct(emu, a, g, s, location=MVN_DEVICE))


@pytest.mark.parametrize("mode", rs.PAD_MODES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call_image_route(emu, key, mode):
    rs.check_image_route(emu, key, mode, orc if mode == "none" else None)


@pytest.mark.parametrize("mode", ["zero", "reflect"])
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call_weights_route(emu, key, mode):
    c, want = rs.check_weights_route(emu, key, mode)
    got = rs.resampled_call(emu, c, mode, location=MVN_DEVICE)
    assert np.array_equal(got, want)


def test_reflect_fill_runs_behind_the_normalisation(emu):
    # mirrored first and normalised second would leave other margins: W of the window's voxels only is what counts
    c, want = rs.check_weights_route(emu, "even block", "reflect")
    _, zero = rs.check_weights_route(emu, "even block", "zero")
    assert not np.array_equal(want, zero)


@pytest.mark.parametrize("location", [None, MVN_DEVICE], ids=["host raw stacks", "resident raw stacks"])
def test_block_after_block(emu, location):
    rs.check_block_after_block(emu, location)


def test_composition_with_acceleration_tv_background_and_statistics(emu):
    rs.check_composition(emu)


def test_errors_leave_psi_untouched(emu):
    rs.check_errors_leave_psi_untouched(emu)


def test_memory_figure(emu):
    rs.check_memory_figure(emu)


def test_halo_engine_refuses(emu):
    rs.check_halo_engine_refuses(emu)


def test_engine_api(emu):
    rs.check_engine_api(emu)


def test_image_storage_mode_1_leaves_resampled_images_float32(emu):
    rs.check_image_storage_stays_float32(emu)


def test_time_utility(emu):
    before = emu.resample_counters()
    for u16 in (False, True):
        ms = emu.resample_time(rs.geometry("anisotropic scale"), (10, 14, 70), u16=u16, reps=2)
        assert ms[0] >= 0 and ms[1] >= 0
    assert emu.resample_counters()[0] - before[0] == 2 * 3
