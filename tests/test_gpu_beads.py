"""Bead PSFs on the MI355X (csrc/mvn_beads.hpp: k_beads_gather, k_beads_reduce, k_beads_min, k_beads_sub, k_beads_score,
k_beads_score_fold): the cases of test_emu_beads.py at the same small shapes on the real kernels - mvn_extract_psf bit
for bit against the numpy restatement, the closed form, the scores, the planted PSF through the kernel derivation into
a resampled call, the errors, the memory figure, counters and timing; and, in one child process that imports torch
first, raw stacks in device memory (dense, with a row pitch, one value) and a device pointer described as host memory.
The checks live in beads_reference.py."""
import os
import subprocess
import sys

import pytest

import beads_reference as br

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("r", br.PSFS, ids=str)
@pytest.mark.parametrize("m", br.STACKS, ids=str)
def test_bit_equality_with_the_restatement(gpu, m, r):
    br.check_bits(gpu, m, r, br.HOST)


def test_closed_form(gpu):
    br.check_closed_form(gpu)


def test_scores(gpu):
    br.check_scores(gpu)


def test_planted_psf(gpu):
    br.check_planted_psf(gpu)


def test_errors_leave_the_outputs_untouched(gpu):
    br.apart(br.check_errors, gpu)


def test_memory_figure(gpu):
    br.apart(br.check_memory, gpu)


def test_counters_and_timing(gpu):
    br.apart(br.check_counters_and_timing, gpu)


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_HOST
import beads_reference as br
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"

def dev(a):
    # (uint16 travels as int16 bits: every torch has that type)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

places = {"device": (dev, {"int16_is_uint16": True})}
for m in br.STACKS:
    for r in br.PSFS:
        br.check_bits(gpu, m, r, places)
br.check_closed_form(gpu, places)
br.check_scores(gpu, places)
m, r = br.STACKS[0], br.PSFS[0]
vals = br.values(m, np.float32)
t = dev(vals)
assert gpu.extract_memory(t, 33, r, True) == br.memory_model(33, r, True)
print("device stacks ok", flush=True)

# a device pointer described as host memory: refused before anything reads it, the outputs untouched
ptr, desc, shape, _ = native.describe_stack(t)
desc.location = MVN_HOST
psf, sc = np.full(r, -3, np.float32), np.full(4, -3.0)
before = gpu.extract_counters()
assert br.extract_raw(gpu, ptr, desc, shape, br.positions(m, 4), r, 0, psf, sc) < 0
assert "host memory" in gpu.l.mvn_last_error().decode()
assert np.all(psf == -3) and np.all(sc == -3) and gpu.extract_counters() == before
print("described as host ok", flush=True)
"""


def test_stacks_in_device_memory():
    # Time limit: importing torch and loading the library into a new process takes most of it, the calls little.
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    tail = (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    for line in ("device stacks ok", "described as host ok"):
        assert line in r.stdout, tail
