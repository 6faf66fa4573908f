"""Fusion on the MI355X (csrc/mvn_fuse.hpp: k_fuse_resampled, k_fuse_volumes): the checks of test_emu_fuse.py at the
same small shapes on the real kernels - mvn_fuse_resampled bit for bit against the numpy restatement applied to what the
library's resample pass returns and against pure numpy with hard edges; the uint16 rule; psi start under all four padding
policies and both weights modes, block after block and with the loop's switches; the engine API; errors, the memory
figure, counters and timing; and, in one child process that imports torch first, raw stacks and outputs in device
memory.  The checks live in fuse_reference.py."""
import os
import subprocess
import sys

import pytest

import fuse_reference as fr
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


@pytest.mark.parametrize("out_dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("group", sorted(fr.GROUPS))
def test_against_the_resample_pass(gpu, group, out_dtype):
    assert fr.check_against_resample_pass(gpu, group, out_dtype) == 3 * 3 * 2 * 2


@pytest.mark.parametrize("out_dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("group", sorted(fr.GROUPS))
def test_against_pure_numpy_with_hard_edges(gpu, group, out_dtype):
    fr.check_against_numpy(gpu, group, out_dtype)


def test_uint16_rule(gpu):
    fr.check_uint16_rule(gpu)


@pytest.mark.parametrize("weights_mode", [0, 1], ids=["caller's weights", "computed weights"])
@pytest.mark.parametrize("mode", rs.PAD_MODES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_psi_start(gpu, key, mode, weights_mode):
    fr.check_psi_start(gpu, key, mode, weights_mode)


def test_psi_start_block_after_block(gpu):
    fr.check_psi_start_block_after_block(gpu)


def test_psi_start_with_acceleration_tv_background_and_statistics(gpu):
    fr.check_psi_start_composition(gpu)


def test_engine_api(gpu):
    fr.check_engine_api(gpu)


def test_engine_refusals(gpu):
    fr.check_engine_refusals(gpu)


def test_errors(gpu):
    fr.check_errors(gpu)


def test_memory_figure(gpu):
    fr.check_memory(gpu)


def test_counters_and_timing(gpu):
    fr.check_counters_and_timing(gpu)


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import fuse_reference as fr
import resample_reference as rs
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"

def dev(a):
    # (uint16 travels as int16 bits: every torch has that type)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

def host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype is np.uint16 else a

def raw_on_device(raw, layout):
    if layout == "dense":
        return dev(raw)
    big = dev(np.full(tuple(s + 3 for s in raw.shape), 7, raw.dtype))
    win = big[1:1 + raw.shape[0], 2:2 + raw.shape[1], 1:1 + raw.shape[2]]
    win.copy_(dev(raw))
    assert not win.is_contiguous()
    return win

def out_on_device(block, dtype, layout):
    # dense; a window with contiguous rows of a larger tensor; elements of a row two apart, planes the fastest but one
    if layout == "dense":
        big = dev(np.full(block, 9, dtype))
        return big, big, None
    if layout == "window":
        big = dev(np.full(tuple(s + 3 for s in block), 9, dtype))
        return big[1:1 + block[0], 2:2 + block[1], 1:1 + block[2]], big, (slice(1, 1 + block[0]), slice(2, 2 + block[1]), slice(1, 1 + block[2]))
    big = dev(np.full((block[2] * 2, block[0], block[1]), 9, dtype))
    return big[::2].permute(1, 2, 0), big, None

# raw stacks and output as tensors on the device, dense and non-contiguous, for every group and both output types
for group in sorted(fr.GROUPS):
    block = fr.block_of(group)
    for raw_layout in ("dense", "row-strided"):
        raws, geoms = fr.group_views(group, fr.MIXED, "dense")
        images, ws = fr.library_stacks(gpu, group, fr.MIXED, "dense")
        traws = [raw_on_device(r, raw_layout) for r in raws]
        for dtype in rs.DTYPES:
            for fill in fr.FILLS:
                want = fr.as_output(fr.fuse_numpy(images, ws, fill), dtype)
                for out_layout in ("dense", "window", "permuted"):
                    out, big, window = out_on_device(block, dtype, out_layout)
                    assert tuple(out.shape) == block and (out_layout == "dense") == out.is_contiguous()
                    gpu.fuse_resampled(out, traws, geoms, fill, int16_is_uint16=True)
                    got = host(out, dtype)
                    assert np.array_equal(got, want), (group, raw_layout, dtype, fill, out_layout)
                    whole = host(big, dtype)
                    if out_layout == "window":
                        ref = np.full(whole.shape, 9, dtype)
                        ref[window] = want
                        assert np.array_equal(whole, ref), (group, out_layout, "outside the window")
                    elif out_layout == "permuted":
                        assert (whole[1::2] == 9).all(), (group, out_layout, "between the elements")
    # host raw stacks into a device output, and device raw stacks into a host output
    out, big, _ = out_on_device(block, np.float32, "dense")
    gpu.fuse_resampled(out, raws, geoms, 123.5)
    assert np.array_equal(host(out, np.float32), fr.fuse_numpy(images, ws, 123.5)), group
    win, bigh = fr.new_output(block, np.uint16, "window")
    gpu.fuse_resampled(win, traws, geoms, 123.5, int16_is_uint16=True)
    fr.assert_output(win, bigh, fr.to_uint16(fr.fuse_numpy(images, ws, 123.5)), group)
    assert gpu.fuse_memory(out, traws, geoms, int16_is_uint16=True) == fr.RECORD_BYTES * len(raws)
print("fusion on device stacks ok", flush=True)

# psi start with resident raw stacks and a resident psi
for key in sorted(rs.CALL_VIEWS):
    for mode in ("zero", "reflect"):
        c = rs.make_call(key)
        psi0 = fr.fused_start(gpu, c, None)
        gpu.check(gpu.l.mvn_release_cached_engines())
        want = rs.resampled_call(gpu, dict(c, psi0=psi0), mode)
        raws = [dev(r) for r in c["raws"]]
        psi = dev(fr.garbage(c["block"]))
        call = gpu.resample_call(psi, raws, c["geoms"], c["k1"], c["k2"], 0.006, rs.MINV, 3, int16_is_uint16=True)
        before = gpu.fuse_counters()
        fr.with_psi_start(gpu, 1, fr.PSI_FILL, lambda: rs.with_pad_mode(gpu, mode, call.run))
        after = gpu.fuse_counters()
        assert (after[0] - before[0], after[1] - before[1]) == (0, 1)
        assert np.array_equal(psi.cpu().numpy(), want), (key, mode)
print("psi start on device stacks ok", flush=True)
"""


def test_stacks_in_device_memory():
    # Time limit: importing torch and loading the library into a new process takes most of it, the calls little.
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    tail = (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    for line in ("fusion on device stacks ok", "psi start on device stacks ok"):
        assert line in r.stdout, tail
