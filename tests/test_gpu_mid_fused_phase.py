"""The steady state of the fused middle pass's walk on the GPU (csrc/mvn_mid_fused.hpp, kf_mid<K>): the peeled mixed batch
and the loop unrolled over the window phase - against the oracle, and bit for bit against results recorded from the build
in front of the change that made the phase a compile-time constant (tools/mid_fused_phase_golden.py)."""
import os

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from nonfinite_util import nonfinite_cases
import mid_fused_phase_util as mu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):  # fresh checkout on the GPU box: compile, never fall back
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()  # raises if the HIP library is missing: no fallback
    assert b.backend_name() == "hip-gfx950"
    return b


@pytest.fixture(scope="module")
def orc():
    from oracle import binding
    return binding


@pytest.fixture
def fused(gpu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")  # the fused pass on shallow volumes too
    gpu.check(gpu.l.mvn_release_cached_engines())
    yield gpu
    gpu.check(gpu.l.mvn_release_cached_engines())


@pytest.fixture(scope="module")
def golden():
    return mu.load_golden("gpu")


@pytest.mark.parametrize("k0,d0", mu.CASES)
def test_every_phase_and_loop_exit_vs_oracle_and_recorded_results(fused, orc, golden, k0, d0):
    got, h, psi0 = mu.run_case(fused, k0, d0)
    mu.check_case(got, orc.cpu_deconvolve(psi0, h, -1), golden, k0, d0)


def test_unrolled_loop_in_the_slab_form(fused, monkeypatch):
    # MVN_DEVICES: every slab walks from its lower halo to its upper one without wrapping (zcount > 0), 31 taps, four
    # window phases; bit-equal to the one-device call
    views, k1, k2, w, psi0 = mu.case_inputs(31, 64)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 1)
    single = fused.gpu_deconvolve(psi0, h)
    monkeypatch.setenv("MVN_DEVICES", "0,0")
    try:
        before, c0 = fused.l.mvn_multi_device_calls(), fused.l.mvn_mid_fused_launch_count()
        multi = fused.gpu_deconvolve(psi0, h)
        assert fused.l.mvn_multi_device_calls() == before + 1
        assert fused.l.mvn_mid_fused_launch_count() - c0 == 1 * 2 * 2 * 2
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
    assert np.array_equal(multi, single)


@pytest.mark.parametrize("pos", mu.NONFINITE_POS)
def test_nonfinite_voxel_is_tracked_in_every_window_phase(fused, pos):
    # (the planes of mu.NONFINITE_POS are the newest input of an output step in the phases 0, 1, 2, 3: the flood must come)
    c0 = fused.l.mvn_mid_fused_launch_count()
    nonfinite_cases(fused, mu.NONFINITE_SHAPE, mu.NONFINITE_PSF, pos, its_list=(1,))
    assert fused.l.mvn_mid_fused_launch_count() > c0
