"""Resampled views on the MI355X (csrc/mvn_resample.hpp: k_resample3d, k_weights_normalize): the cases of
test_emu_resample.py at the same small shapes on the real kernels - the pass alone against the numpy restatement (the
image bit for bit, the weights by their rule) for every case, element type and layout; the call against the plain call
on the library's own resampled stacks under all four padding policies and against the CPU oracle; computed weights;
block after block; the loop's switches together; the surface; and, in one child process that imports torch first, raw
stacks in device memory.  The checks live in resample_reference.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import binding as orc
import resample_reference as rs

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


@pytest.mark.parametrize("layout", rs.LAYOUTS)
@pytest.mark.parametrize("dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("name", sorted(rs.CASES))
def test_pass_against_numpy(gpu, name, dtype, layout):
    rs.check_stack(gpu, name, dtype, layout)


@pytest.mark.parametrize("mode", rs.PAD_MODES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call_image_route(gpu, key, mode):
    rs.check_image_route(gpu, key, mode, orc if mode == "none" else None)


@pytest.mark.parametrize("mode", ["zero", "reflect"])
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_call_weights_route(gpu, key, mode):
    rs.check_weights_route(gpu, key, mode)


def test_reflect_fill_runs_behind_the_normalisation(gpu):
    _, want = rs.check_weights_route(gpu, "even block", "reflect")
    _, zero = rs.check_weights_route(gpu, "even block", "zero")
    assert not np.array_equal(want, zero)


def test_block_after_block_from_host_raw_stacks(gpu):
    rs.check_block_after_block(gpu)


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import resample_reference as rs
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"

def dev(a):
    # (uint16 travels as int16 bits: every torch has that type)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

def laid_out(raw, layout):
    if layout == "dense":
        return dev(raw)
    if layout == "row-strided":
        big = dev(np.full(tuple(s + 3 for s in raw.shape), 7, raw.dtype))
        win = big[1:1 + raw.shape[0], 2:2 + raw.shape[1], 1:1 + raw.shape[2]]
        win.copy_(dev(raw))
        return win
    return dev(raw[:1, :1, :1]).expand(*raw.shape)

# the pass alone on raw stacks in device memory: every case, both element types, dense, row-strided and broadcast
for name in sorted(rs.CASES):
    for dtype in rs.DTYPES:
        for layout in rs.LAYOUTS:
            raw = rs.raw_stack(name, dtype)
            t = laid_out(raw, layout)
            if layout != "dense":
                assert not t.is_contiguous()
            host = np.ascontiguousarray(rs.laid_out(raw, layout))
            got_i, got_w = gpu.resample_stack(t, rs.geometry(name), rs.CASES[name][0], int16_is_uint16=True)
            block, _, M, border, rng = rs.CASES[name]
            want_i, want_w, zero, one = rs.resample_numpy(host, M, block, border, rng)
            assert np.array_equal(got_i, want_i), (name, dtype, layout)
            rs.check_weights(name, got_w, want_w, zero, one)
print("pass on device stacks ok", flush=True)

# the call from resident raw stacks: computed weights under "zero" and "reflect", psi in device memory too
for key in sorted(rs.CALL_VIEWS):
    for mode in ("zero", "reflect"):
        c = rs.make_call(key)
        images, ws = rs.library_stacks(gpu, c)
        gpu.check(gpu.l.mvn_release_cached_engines())
        want = rs.plain_call(gpu, c, images, rs.normalize_numpy(ws), mode)
        raws = [dev(r) for r in c["raws"]]
        psi = dev(c["psi0"])
        call = gpu.resample_call(psi, raws, c["geoms"], c["k1"], c["k2"], 0.006, rs.MINV, 3, int16_is_uint16=True)
        rs.with_pad_mode(gpu, mode, call.run)
        assert np.array_equal(psi.cpu().numpy(), want), (key, mode)
        h = rs.WorkspaceHolder(images, c["k1"], c["k2"], ws, 0.006, rs.MINV, 3)
        assert call.memory() == gpu.deconvolve_memory(h, 0)  # (nothing is uploaded: the figure of the plain call)
print("call on device stacks ok", flush=True)

# block after block: the raw stacks stay where they are, only the matrix offset changes
key = "even block"
c = rs.make_call(key)
raws = [dev(r) for r in c["raws"]]
gpu.check(gpu.l.mvn_release_cached_engines())
for shift in ((0, 0, 0), (1, 2, 3)):
    geoms = []
    for n in c["names"]:
        block, raw, M, border, rng = rs.CASES[n]
        M = np.asarray(M, np.float64).copy()
        M[:, 3] = M[:, 3] + M[:, :3] @ np.asarray(shift, np.float64)
        geoms.append(rs.view_geometry(raw, M, border, rng))
    cb = dict(c, geoms=geoms)
    images, ws = rs.library_stacks(gpu, cb)
    want = rs.plain_call(gpu, cb, images, rs.normalize_numpy(ws), "zero")
    psi = c["psi0"].copy()
    call = gpu.resample_call(psi, raws, geoms, c["k1"], c["k2"], 0.006, rs.MINV, 3, int16_is_uint16=True)
    rs.with_pad_mode(gpu, "zero", call.run)
    assert np.array_equal(psi, want), shift
print("block after block ok", flush=True)
"""


def test_raw_stacks_in_device_memory():
    # Time limit: importing torch and loading the library into a new process takes most of it, the calls little.
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    tail = (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    for line in ("pass on device stacks ok", "call on device stacks ok", "block after block ok"):
        assert line in r.stdout, tail


def test_composition_with_acceleration_tv_background_and_statistics(gpu):
    rs.check_composition(gpu)


def test_errors_leave_psi_untouched(gpu):
    rs.check_errors_leave_psi_untouched(gpu)


def test_memory_figure(gpu):
    rs.check_memory_figure(gpu)


def test_halo_engine_refuses(gpu):
    rs.check_halo_engine_refuses(gpu)


def test_engine_api(gpu):
    rs.check_engine_api(gpu)


def test_image_storage_mode_1_leaves_resampled_images_float32(gpu):
    rs.check_image_storage_stays_float32(gpu)


def test_time_utility(gpu):
    before = gpu.resample_counters()
    for u16 in (False, True):
        ms = gpu.resample_time(rs.geometry("anisotropic scale"), (10, 14, 70), u16=u16, reps=2)
        assert ms[0] > 0 and ms[1] > 0
    assert gpu.resample_counters()[0] - before[0] == 2 * 3
