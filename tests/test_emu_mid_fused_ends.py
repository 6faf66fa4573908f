"""The ends of the fused middle pass's walk on the host emulation (csrc/mvn_mid_fused.hpp): the prologue that fills the
window, the mixed batch, the tail - against the oracle, and bit for bit against results recorded from the build in front
of the change that gave the walk its own prologue and tail (tools/mid_fused_ends_golden.py)."""
import os
import subprocess

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from nonfinite_util import nonfinite_cases
import mid_fused_ends_util as mu

CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    return native.Binding(native.EMU_SO)


@pytest.fixture
def fused(emu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")  # the fused pass on shallow volumes too
    emu.l.mvn_release_cached_engines()
    yield emu
    emu.l.mvn_release_cached_engines()


@pytest.fixture(scope="module")
def golden():
    return mu.load_golden("emu")


@pytest.mark.parametrize("k0,d0", mu.CASES)
def test_ends_of_the_walk_vs_oracle_and_recorded_results(fused, golden, k0, d0):
    got, h, psi0 = mu.run_case(fused, k0, d0)
    ref = orc.cpu_deconvolve(psi0, h, 8)
    err, mx = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("K %d d0 %d: max |got - ref| %.3g, max |ref| %.3g" % (k0, d0, err, mx))
    assert err <= 1e-5 * mx, (k0, d0, err, mx)
    if (k0, d0) in mu.PINNED:
        key = mu.golden_key(k0, d0)
        assert np.array_equal(golden[key + "_idx"], mu.sample_index(k0, d0))
        assert np.array_equal(got.reshape(-1)[golden[key + "_idx"]], golden[key + "_val"]), (k0, d0)


def test_ends_of_the_walk_in_the_slab_form(fused, monkeypatch):
    # MVN_DEVICES: every slab walks from its lower halo to its upper one without wrapping (zcount > 0), 13 taps: one whole
    # fill batch, a mixed batch of four fill lines; bit-equal to the one-device call
    views, k1, k2, w, psi0 = mu.case_inputs(13, 40)
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
    ref = orc.cpu_deconvolve(psi0, h, 8)
    assert np.abs(single - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("pos", [(11, 100, 7), (1, 100, 7), (22, 300, 500)])
def test_nonfinite_voxel_in_the_first_and_the_last_planes(fused, pos):
    # 5 taps, h = 2: a whole column's walk starts at plane 22, so planes 22, 23, 0, 1 are read once as fill lines
    # (which track nothing) and once, at the walk's end, as the newest input of an output step (which does): the
    # flood must come.  Plane 11: the interior.
    c0 = fused.l.mvn_mid_fused_launch_count()
    nonfinite_cases(fused, (24, 512, 512), (5, 3, 3), pos, its_list=(1,))
    assert fused.l.mvn_mid_fused_launch_count() > c0
