"""Bead registration on the MI355X (csrc/mvn_register.hpp: k_reg_neighbours, k_reg_match, k_reg_match_fold,
k_reg_ransac): the cases of test_emu_register.py at the same small sizes on the real kernels - neighbours, candidates
and registrations bit for bit against the numpy restatement, planted pairs against numpy.linalg.lstsq, a prior, sets
without a model, exactly four candidates, the sample, the independence of the match from its chunks, the chain from two
raw stacks through mvn_detect_beads, the errors, the memory figure, counters and timing.  The checks live in
register_reference.py."""
import os

import pytest

import register_reference as rr

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


@pytest.mark.parametrize("size", rr.SIZES, ids=str)
def test_neighbours_bit_for_bit(gpu, size):
    rr.check_neighbours(gpu, size)


@pytest.mark.parametrize("size", rr.SIZES, ids=str)
def test_candidates_bit_for_bit(gpu, size):
    rr.check_candidates(gpu, size)


@pytest.mark.parametrize("hyps", rr.HYPOTHESES)
@pytest.mark.parametrize("size", rr.SIZES, ids=str)
def test_registration_bit_for_bit(gpu, size, hyps):
    rr.check_registration(gpu, size, hyps)


def test_planted_truth(gpu):
    rr.check_planted_truth(gpu)


def test_prior(gpu):
    rr.check_prior(gpu)


def test_no_model_is_no_error(gpu):
    rr.apart(rr.check_no_model, gpu)


def test_exactly_four_candidates(gpu):
    rr.check_four_candidates(gpu)


def test_sample(gpu):
    rr.apart(rr.check_sample, gpu)


def test_chunk_independence(gpu):
    rr.check_chunk_independence(gpu)


def test_the_chain_from_raw_stacks(gpu):
    rr.check_chain(gpu)


def test_errors_leave_the_outputs_untouched(gpu):
    rr.apart(rr.check_errors, gpu)


def test_memory_figure(gpu):
    rr.apart(rr.check_memory, gpu)


def test_counters_and_timing(gpu):
    rr.apart(rr.check_counters_and_timing, gpu)
