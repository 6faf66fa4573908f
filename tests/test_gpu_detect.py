"""Bead detection on the MI355X (csrc/mvn_detect.hpp: k_detect_rows, k_detect_lines, k_detect_extrema,
k_detect_refine): the cases of test_emu_detect.py at the same small shapes on the real kernels - mvn_detect_dog and
mvn_detect_beads bit for bit against the numpy restatement, the closed form of one impulse, planted beads through
mvn_extract_psf, fits that leave the voxel or have no determinant, the errors, the memory figure, counters and timing;
and, in one child process that imports torch first, raw stacks in device memory (dense, with a row pitch, one value)
and a device pointer described as host memory.  The checks live in detect_reference.py."""
import os
import subprocess
import sys

import pytest

import detect_reference as dr

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


def test_taps(gpu):
    dr.apart(dr.check_taps, gpu)


@pytest.mark.parametrize("sig", range(len(dr.SIGMAS)))
@pytest.mark.parametrize("m", dr.STACKS, ids=str)
def test_dog_bit_for_bit(gpu, m, sig):
    dr.check_dog(gpu, m, sig, dr.HOST)


@pytest.mark.parametrize("sig", range(len(dr.SIGMAS)))
@pytest.mark.parametrize("m", dr.STACKS, ids=str)
def test_detections_bit_for_bit(gpu, m, sig):
    dr.check_detections(gpu, m, sig, dr.HOST)


def test_a_row_pitch_and_one_value(gpu):
    dr.check_detections(gpu, dr.STACKS[1], 1, dr.HOST, layouts=("pitched",))
    dr.check_one_value(gpu, dr.HOST)


def test_closed_form(gpu):
    dr.check_closed_form(gpu)


def test_planted_beads(gpu):
    dr.check_planted_beads(gpu)


def test_offsets_beyond_the_bound(gpu):
    dr.check_offsets_beyond_the_bound(gpu)


def test_errors_leave_the_outputs_untouched(gpu):
    dr.apart(dr.check_errors, gpu)


def test_memory_figure(gpu):
    dr.apart(dr.check_memory, gpu)


def test_counters_and_timing(gpu):
    dr.apart(dr.check_counters_and_timing, gpu)


_CHILD = r"""
import ctypes as C
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_HOST, detect_params
import detect_reference as dr
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"

def dev(a):
    # (uint16 travels as int16 bits: every torch has that type)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

places = {"device": (dev, {"int16_is_uint16": True})}
for m in dr.STACKS[:2]:
    dr.check_dog(gpu, m, 0, places)
    dr.check_detections(gpu, m, 0, places, layouts=("dense", "pitched"))
dr.check_detections(gpu, dr.STACKS[2], 1, places)
dr.check_one_value(gpu, places)
dr.check_closed_form(gpu, places)
m = dr.STACKS[1]
vals = dr.values(m, np.float32)
t = dev(vals)
assert gpu.detect_memory(t, 100) == dr.memory_model(m, 100)
print("device stacks ok", flush=True)

# a device pointer described as host memory: refused before anything reads it, the outputs untouched
ptr, desc, shape, _ = native.describe_stack(t)
desc.location = MVN_HOST
n, pos, val, vox = C.c_int(-3), np.full((64, 3), -3.0), np.full(64, -3, np.float32), np.full((64, 3), -3, np.int32)
before = gpu.detect_counters()
prm = detect_params(*dr.SIGMAS[0], 2.0)
assert dr.detect_raw(gpu, ptr, desc, shape, prm, 64, n, pos, val, vox) < 0
assert "host memory" in gpu.l.mvn_last_error().decode()
assert n.value == -3 and np.all(pos == -3) and np.all(val == -3) and np.all(vox == -3)
assert gpu.detect_counters() == before
print("described as host ok", flush=True)
"""


def test_stacks_in_device_memory():
    # Time limit: importing torch and loading the library into a new process takes most of it, the calls little.
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    tail = (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    for line in ("device stacks ok", "described as host ok"):
        assert line in r.stdout, tail
