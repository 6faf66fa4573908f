"""Bead detection on the host emulation (csrc/mvn_detect.hpp; the emulation runs the passes' own bodies):
mvn_detect_dog and mvn_detect_beads bit for bit against the numpy restatement of the definition - both element types,
host memory and what the emulation calls device memory, a stack narrower than the radius, one with several workgroups
in every pass, four sigma sets, maxima and minima -, the closed form of one impulse, planted beads through
mvn_extract_psf, fits that leave the voxel or have no determinant, the errors, the memory figure, the counters and the
timing utility.  The checks live in detect_reference.py; test_gpu_detect.py runs them on the device."""
import os
import subprocess

import pytest

from libmultiviewnative_amd import native
import detect_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")
NEW = ("mvn_detect_beads", "mvn_detect_taps", "mvn_detect_dog", "mvn_detect_memory", "mvn_detect_counters",
       "mvn_detect_time")


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
    assert "#define MVN_DETECT_MAX_RADIUS %d" % native.DETECT_MAX_RADIUS in hdr
    assert "MVN_DETECT_MINIMA = %d" % native.DETECT_MINIMA in hdr


def test_the_remark_that_left_detection_to_the_caller_is_gone():
    txt = " ".join(open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read().split())
    assert "Out of scope: detecting the beads" not in txt
    for name in ("include/mvn_engine_api.h", "INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "mvn_detect_beads" in open(os.path.join(ROOT, name)).read(), name


def test_taps(emu):
    dr.apart(dr.check_taps, emu)


@pytest.mark.parametrize("sig", range(len(dr.SIGMAS)))
@pytest.mark.parametrize("m", dr.STACKS, ids=str)
def test_dog_bit_for_bit(emu, m, sig):
    dr.check_dog(emu, m, sig, dr.EMU_PLACES)


@pytest.mark.parametrize("sig", range(len(dr.SIGMAS)))
@pytest.mark.parametrize("m", dr.STACKS, ids=str)
def test_detections_bit_for_bit(emu, m, sig):
    dr.check_detections(emu, m, sig, dr.EMU_PLACES if m != dr.STACKS[2] else dr.HOST)


def test_a_row_pitch_and_one_value(emu):
    dr.check_detections(emu, dr.STACKS[1], 1, dr.EMU_PLACES, layouts=("pitched",))
    dr.check_one_value(emu, dr.EMU_PLACES)


def test_closed_form(emu):
    dr.check_closed_form(emu, dr.EMU_PLACES)


def test_planted_beads(emu):
    dr.check_planted_beads(emu)


def test_offsets_beyond_the_bound(emu):
    dr.check_offsets_beyond_the_bound(emu, dr.EMU_PLACES)


def test_errors_leave_the_outputs_untouched(emu):
    dr.apart(dr.check_errors, emu)


def test_memory_figure(emu):
    dr.apart(dr.check_memory, emu)


def test_counters_and_timing(emu):
    dr.apart(dr.check_counters_and_timing, emu)
