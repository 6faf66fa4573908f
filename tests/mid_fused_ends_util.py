"""The ends of the fused middle pass's walk (csrc/mvn_mid_fused.hpp: prologue, mixed batch, tail): cases shared by the
emulation test, the -m gpu test and tools/mid_fused_ends_golden.py."""
import os

import numpy as np

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import realistic_views

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (taps K, planes d0) on (d0, 512, 512) volumes with (K, 3, 3) PSFs.  A walk is d0 + K - 1 steps in batches of 8; the
# first K - 1 steps fill the window: P = (K - 1) // 8 whole batches in the prologue, the rest in the mixed batch.
CASES = [
    (1, 8),    # no fill, a walk of exactly one batch
    (1, 9),    # ... and one batch + 1
    (3, 16),   # fill shorter than a batch: P = 0
    (7, 16),
    (9, 16),   # fill is exactly one batch: no mixed batch
    (17, 24),  # two whole fill batches
    (25, 32),  # three
    (31, 35),  # d0 + 30 = 1 mod 8: a last batch of one line
    (31, 41),  # ... of seven
    (31, 42),  # ... a full one
    (15, 26),  # 40 steps, 5 batches: the line buffers' parity carried from the prologue into the loop
]
# the cases whose results are pinned bit for bit to the build in front of the change (tests/golden/mid_fused_ends_*.npz)
PINNED = [(1, 9), (9, 16), (31, 35), (31, 42)]
SAMPLE = 4096


def case_inputs(k0, d0):
    """2 views of (d0, 512, 512), PSFs (k0, 3, 3), an asymmetric second kernel of the same depth."""
    shape = (d0, 512, 512)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (k0, 3, 3), seed=700 + 37 * k0 + d0)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    return views, k1, k2, w, psi0


def case_lambda(k0, d0):
    """lambda 0 and 0.006 alternate over the cases (both forms of the update's epilogue)."""
    return 0.0 if CASES.index((k0, d0)) % 2 else 0.006


def run_case(binding, k0, d0, inputs=None):
    """Two iterations of the sequential sweep through the blocking ABI call; the fused launches are counted.  The caller
    sets MVN_PAD_MODE=none and MVN_MID_FUSED=2 (the fused pass on shallow volumes too) and drops the cached engines."""
    views, k1, k2, w, psi0 = inputs if inputs is not None else case_inputs(k0, d0)
    h = WorkspaceHolder(views, k1, k2, w, case_lambda(k0, d0), 1e-4, 2)
    c0 = binding.l.mvn_mid_fused_launch_count()
    got = binding.gpu_deconvolve(psi0, h)
    assert binding.l.mvn_mid_fused_launch_count() - c0 == 2 * 2 * 2  # iterations x views x convolutions
    return got, h, psi0


def sample_index(k0, d0):
    """SAMPLE voxels of the result: seeded, and every plane of the two ends of the walk is met."""
    rng = np.random.default_rng(9000 + 100 * k0 + d0)
    return np.sort(rng.choice(d0 * 512 * 512, SAMPLE, replace=False))


def golden_key(k0, d0):
    return "k%d_d%d" % (k0, d0)


def load_golden(tag):
    """tag: 'emu' | 'gpu'.  {key + '_idx': indices, key + '_val': float32 values} per pinned case."""
    return np.load(os.path.join(GOLDEN_DIR, "mid_fused_ends_%s.npz" % tag))
