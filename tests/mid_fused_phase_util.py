"""The steady state of the fused middle pass's walk (csrc/mvn_mid_fused.hpp: the mixed batch and the loop unrolled over the
window phase): cases shared by the emulation test, the -m gpu test and tools/mid_fused_phase_golden.py."""
import os

import numpy as np

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import realistic_views

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (taps K, planes d0) on (d0, 512, 512) volumes with (K, 3, 3) PSFs.  A walk is d0 + K - 1 steps in batches of 8.  With
# NU = ceil(K / 8) window phases and P = (K - 1) // 8 whole fill batches (P + 1 == NU), batch P is the mixed batch and the
# L = ceil((d0 + K - 1) / 8) - (P + 1) batches behind it run in the loop that is unrolled over the NU phases: L takes
# every remainder mod NU, and the loop is left in its first turn, at the end of it and in a later one.
CASES = [
    (9, 16), (9, 24), (9, 32), (9, 40),      # NU = 2: L = 1, 2, 3, 4
    (17, 24), (17, 32), (17, 40), (17, 48),  # NU = 3: L = 2, 3, 4, 5
    (31, 48), (31, 56), (31, 64), (31, 72),  # NU = 4: L = 6, 7, 8, 9
    (25, 40),                                # a mixed batch without fill lines ((K - 1) % 8 == 0), L = 4
]
# the emulation runs the smaller half
EMU_CASES = [(9, 16), (9, 24), (17, 24), (17, 32), (31, 48), (31, 56), (25, 40)]
SAMPLE = 4096


def loop_batches(k0, d0):
    return -(-(d0 + k0 - 1) // 8) - ((k0 - 1) // 8 + 1)


def case_inputs(k0, d0):
    """2 views of (d0, 512, 512), PSFs (k0, 3, 3), an asymmetric second kernel of the same depth."""
    shape = (d0, 512, 512)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (k0, 3, 3), seed=4100 + 53 * k0 + d0)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    return views, k1, k2, w, psi0


def case_lambda(k0, d0):
    """lambda 0 and 0.006 alternate over the cases (both forms of the update's epilogue)."""
    return 0.0 if CASES.index((k0, d0)) % 2 else 0.006


def run_case(binding, k0, d0, inputs=None, iterations=2):
    """Two iterations of the sequential sweep through the blocking ABI call; the fused launches are counted.  The caller
    sets MVN_PAD_MODE=none and MVN_MID_FUSED=2 (the fused pass on shallow volumes too) and drops the cached engines."""
    views, k1, k2, w, psi0 = inputs if inputs is not None else case_inputs(k0, d0)
    h = WorkspaceHolder(views, k1, k2, w, case_lambda(k0, d0), 1e-4, iterations)
    c0 = binding.l.mvn_mid_fused_launch_count()
    got = binding.gpu_deconvolve(psi0, h)
    assert binding.l.mvn_mid_fused_launch_count() - c0 == iterations * 2 * 2  # iterations x views x convolutions
    return got, h, psi0


def sample_index(k0, d0):
    """SAMPLE voxels of the result, seeded."""
    rng = np.random.default_rng(31000 + 100 * k0 + d0)
    return np.sort(rng.choice(d0 * 512 * 512, SAMPLE, replace=False))


def golden_key(k0, d0):
    return "k%d_d%d" % (k0, d0)


def load_golden(tag):
    """tag: 'emu' | 'gpu'.  {key + '_idx': indices, key + '_val': float32 values} per case."""
    return np.load(os.path.join(GOLDEN_DIR, "mid_fused_phase_%s.npz" % tag))


def check_case(got, ref, golden, k0, d0):
    """Against the oracle at the project's 1e-5 max, and bit for bit against the recorded values."""
    err, mx = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("K %d d0 %d (%d loop batches): max |got - ref| %.3g, max |ref| %.3g" % (k0, d0, loop_batches(k0, d0), err, mx))
    assert err <= 1e-5 * mx, (k0, d0, err, mx)
    key = golden_key(k0, d0)
    assert np.array_equal(golden[key + "_idx"], sample_index(k0, d0))
    assert np.array_equal(got.reshape(-1)[golden[key + "_idx"]], golden[key + "_val"]), (k0, d0)


# non-finite voxels, 31 taps (h = 15) on 48 planes: a whole column's walk reads plane p as the newest input of output
# step n = p + 15 (p >= 15), in batch n // 8 - planes 20, 28, 36, 44 are tracked in batches 4, 5, 6, 7, i.e. in the
# window phases 0, 1, 2, 3 of the unrolled loop
NONFINITE_SHAPE, NONFINITE_PSF = (48, 512, 512), (31, 3, 3)
NONFINITE_POS = [(20, 100, 7), (28, 300, 500), (36, 0, 0), (44, 511, 257)]
