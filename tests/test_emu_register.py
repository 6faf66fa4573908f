"""Bead registration on the host emulation (csrc/mvn_register.hpp; the emulation runs the passes' own bodies):
mvn_register_neighbours, mvn_register_candidates and mvn_register_beads bit for bit against the numpy restatement of
the definition - five set sizes, four numbers of hypotheses, a prior -, planted pairs against numpy.linalg.lstsq, sets
without a model, exactly four candidates, the sample, the independence of the match from its chunks, the chain from two
raw stacks through mvn_detect_beads, the errors, the memory figure, the counters and the timing utility.  The checks
live in register_reference.py; test_gpu_register.py runs them on the device."""
import os
import subprocess

import pytest

from libmultiviewnative_amd import native
import register_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")
NEW = ("mvn_register_beads", "mvn_register_neighbours", "mvn_register_candidates", "mvn_register_sample",
       "mvn_register_memory", "mvn_register_counters", "mvn_register_time")


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
    assert "MVN_REGISTER_PRIOR = %d" % native.REGISTER_PRIOR in hdr
    assert "#define MVN_REGISTER_NEIGHBOURS %d" % native.REGISTER_NEIGHBOURS in hdr
    assert "#define MVN_REGISTER_REFITS %d" % native.REGISTER_REFITS in hdr
    assert "#define MVN_REGISTER_MAX_BEADS %d" % native.REGISTER_MAX_BEADS in hdr
    assert native.REGISTER_MAX_HYPOTHESES == 1 << 24 and "#define MVN_REGISTER_MAX_HYPOTHESES (1 << 24)" in hdr


def test_the_documents_describe_the_call():
    for name in ("include/mvn_engine_api.h", "INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "mvn_register_beads" in open(os.path.join(ROOT, name)).read(), name


@pytest.mark.parametrize("size", rr.SIZES, ids=str)
def test_neighbours_bit_for_bit(emu, size):
    rr.check_neighbours(emu, size)


@pytest.mark.parametrize("size", rr.SIZES, ids=str)
def test_candidates_bit_for_bit(emu, size):
    rr.check_candidates(emu, size)


@pytest.mark.parametrize("hyps", rr.HYPOTHESES)
@pytest.mark.parametrize("size", rr.SIZES, ids=str)
def test_registration_bit_for_bit(emu, size, hyps):
    rr.check_registration(emu, size, hyps)


def test_planted_truth(emu):
    rr.check_planted_truth(emu)


def test_prior(emu):
    rr.check_prior(emu)


def test_no_model_is_no_error(emu):
    rr.apart(rr.check_no_model, emu)


def test_exactly_four_candidates(emu):
    rr.check_four_candidates(emu)


def test_sample(emu):
    rr.apart(rr.check_sample, emu)


def test_chunk_independence(emu):
    rr.check_chunk_independence(emu)


def test_the_chain_from_raw_stacks(emu):
    rr.check_chain(emu)


def test_errors_leave_the_outputs_untouched(emu):
    rr.apart(rr.check_errors, emu)


def test_memory_figure(emu):
    rr.apart(rr.check_memory, emu)


def test_counters_and_timing(emu):
    rr.apart(rr.check_counters_and_timing, emu)
