"""Padding policy "reflect" on the MI355X (csrc/mvn_reflect.hpp, k_reflect3d): the cases of test_emu_reflect.py at the
same small shapes on the real kernels - the call against the library's own "none" call on hand-mirrored stacks bit for
bit and against the CPU oracle, every placement route (one child process, torch imported first, hands over stacks in
device memory), cached engines, the loop's switches together, the public surface and the border band.  The checks
live in reflect_reference.py."""
import os
import subprocess
import sys

import pytest

from oracle import binding as orc
import reflect_reference as rr

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
    return b


# the suite's pin of the direct dim0 leg (tests/conftest.py) and the product's defaults: see tests/test_gpu_parity.py
@pytest.fixture(params=["suite pin", "product defaults"])
def leg(request, gpu, monkeypatch):
    if request.param == "product defaults":
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    gpu.check(gpu.l.mvn_release_cached_engines())
    yield request.param
    gpu.check(gpu.l.mvn_release_cached_engines())


@pytest.mark.parametrize("name", sorted(rr.PARITY_CASES))
def test_parity_with_hand_mirrored_stacks(gpu, leg, name):
    rr.check_parity(gpu, orc, name)


@pytest.mark.parametrize("name", sorted(rr.ROUTE_CASES))
def test_every_placement_route(gpu, name):
    rr.check_routes(gpu, name)


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import reflect_reference as rr
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
for name in sorted(rr.ROUTE_CASES):
    st = rr.make_stacks(name, integer_views=True)
    views, k1, k2, w, psi0 = st
    want = rr.reflect_call(gpu, st)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    psi = dev(psi0)
    c0 = gpu.reflect_counters()
    rr.described(gpu, st, [dev(v) for v in views], [dev(x) for x in w], psi=psi)
    assert gpu.reflect_counters()[1] - c0[1] == 5
    assert np.array_equal(psi.cpu().numpy(), want), name
    # device views next to host weights and a host psi
    assert np.array_equal(rr.described(gpu, st, [dev(v) for v in views], w), want), name
print("device stacks ok", flush=True)
"""


def test_stacks_in_device_memory():
    # float32 stacks in device memory take the ingest pass on the compute stream; the fill follows it there.
    # Time limit: importing torch and loading the library into a new process takes most of it, the calls little.
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device stacks ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("mem", [None, "stream:1"])
def test_cached_engines_between_zero_and_reflect(gpu, mem):
    rr.check_cached_engines(gpu, mem)


def test_composition_with_acceleration_tv_background_and_statistics(gpu):
    rr.check_composition(gpu)


def test_surface(gpu, monkeypatch):
    rr.check_surface(gpu, monkeypatch)


def test_border_band_of_a_block_cut_out_of_a_larger_specimen(gpu):
    rr.check_border_quality(gpu)


def test_fill_time_utility(gpu):
    before = gpu.reflect_counters()
    for u16 in (False, True):
        ms = gpu.reflect_time((6, 10, 15), (12, 12, 20), (3, 1, 2), u16=u16, reps=2)
        assert ms[0] > 0 and ms[1] > 0
    after = gpu.reflect_counters()
    assert after[1] - before[1] == 2 * 3 and after[0] - before[0] == 2 * 3 * 3
