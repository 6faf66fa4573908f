"""Bead PSFs on the host emulation (csrc/mvn_beads.hpp; the emulation runs the passes' own bodies): mvn_extract_psf bit
for bit against the numpy restatement of the definition - both element types, host memory and what the emulation calls
device memory, a row pitch, one value for every voxel, beads in the corners, at integers and a hair below them, windows
wider than the stack, bead counts on both sides of the group boundary -, the closed form of one bead, the scores, a
planted Gaussian PSF through the kernel derivation into a resampled call, the errors, the memory figure, the counters
and the timing utility.  The checks live in beads_reference.py; test_gpu_beads.py runs them on the device."""
import os
import subprocess

import pytest

from libmultiviewnative_amd import native
import beads_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")
NEW = ("mvn_extract_psf", "mvn_extract_memory", "mvn_extract_counters", "mvn_extract_time")


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
    assert "#define MVN_BEADS_GROUP %d" % native.BEADS_GROUP in hdr
    assert "MVN_BEADS_REMOVE_MIN = %d" % native.BEADS_REMOVE_MIN in hdr


def test_the_remarks_that_left_beads_to_the_caller_are_gone():
    for name in ("include/mvn_engine_api.h", "INTEGRATION.md", "DESIGN.md", "README.md"):
        txt = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "Out of scope: extracting PSFs from beads" not in txt, name
        assert "mvn_extract_psf" in txt, name


@pytest.mark.parametrize("r", br.PSFS, ids=str)
@pytest.mark.parametrize("m", br.STACKS, ids=str)
def test_bit_equality_with_the_restatement(emu, m, r):
    br.check_bits(emu, m, r, br.EMU_PLACES)


def test_closed_form(emu):
    br.check_closed_form(emu, br.EMU_PLACES)


def test_scores(emu):
    br.check_scores(emu, br.EMU_PLACES)


def test_planted_psf(emu):
    br.check_planted_psf(emu)


def test_errors_leave_the_outputs_untouched(emu):
    br.apart(br.check_errors, emu)


def test_memory_figure(emu):
    br.apart(br.check_memory, emu)


def test_counters_and_timing(emu):
    br.apart(br.check_counters_and_timing, emu)
