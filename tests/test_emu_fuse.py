"""Fusion on the host emulation (csrc/mvn_fuse.hpp; the emulation runs the passes' own bodies): mvn_fuse_resampled bit
for bit against the numpy restatement applied to what the library's resample pass returns - every group, output type,
fill, combination of element types, raw layout and output layout - and against pure numpy with weights of exactly 0 or
1; the uint16 rule; psi start under all four padding policies and both weights modes, block after block and with the
loop's switches; the engine API; errors, the memory figure, counters and the timing utility.  The checks live in
fuse_reference.py; test_gpu_fuse.py runs them on the device."""
import os
import subprocess

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_DEVICE
import fuse_reference as fr
import resample_reference as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")
SYMBOLS = ("mvn_fuse_resampled", "mvn_fuse_memory_resampled", "mvn_fuse_time", "mvn_fuse_counters", "mvn_set_psi_start",
           "mvn_get_psi_start", "mvn_engine_fuse_psi")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    b = native.Binding(native.EMU_SO)
    yield b
    b.l.mvn_release_cached_engines()


def test_symbols_declared_exported_bound(emu):
    hdr = open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read()
    exports = open(os.path.join(CSRC, "mvn_exports.map")).read()
    for n in SYMBOLS:
        assert n in native.ENGINE_ABI_SYMBOLS
        assert "MVN_API int %s(" % n in hdr, n
        assert "%s;" % n in exports, n
        assert hasattr(emu.l, n)


@pytest.mark.parametrize("out_dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("group", sorted(fr.GROUPS))
def test_against_the_resample_pass(emu, group, out_dtype):
    assert fr.check_against_resample_pass(emu, group, out_dtype) == 3 * 3 * 2 * 2


@pytest.mark.parametrize("out_dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("group", ["(3, 5, 7)", "(10, 14, 70) x 3"])
def test_stacks_and_output_described_as_device_memory(emu, group, out_dtype):
    # (any pointer of the emulation may be called device memory: raw stacks are then read and the output is written
    #  where they lie, strides and all)
    def fuse(out, raws, geoms, fill):
        assert fr.fuse_direct(emu, out, raws, geoms, fill, MVN_DEVICE, MVN_DEVICE) == 0, emu.l.mvn_last_error()
    fr.check_against_resample_pass(emu, group, out_dtype, fuse)


def test_output_in_device_memory_with_any_strides(emu):
    group = "(4, 6, 10)"
    raws, geoms = fr.group_views(group)
    images, ws = fr.library_stacks(emu, group, fr.MIXED)
    for dtype in rs.DTYPES:
        want = fr.as_output(fr.fuse_numpy(images, ws, 123.5), dtype)
        block = fr.block_of(group)
        big = np.full((block[2] * 2, block[0], block[1]), 9, dtype)
        out = big[::2].transpose(1, 2, 0)  # elements of a row two apart, planes the fastest but one
        assert out.shape == block and out.strides[2] != out.itemsize
        assert fr.fuse_direct(emu, out, raws, geoms, 123.5, MVN_DEVICE, MVN_DEVICE) == 0
        assert np.array_equal(out, want) and (big[1::2] == 9).all()


@pytest.mark.parametrize("out_dtype", rs.DTYPES, ids=["uint16", "float32"])
@pytest.mark.parametrize("group", sorted(fr.GROUPS))
def test_against_pure_numpy_with_hard_edges(emu, group, out_dtype):
    fr.check_against_numpy(emu, group, out_dtype)


def test_uint16_rule(emu):
    fr.check_uint16_rule(emu)


@pytest.mark.parametrize("weights_mode", [0, 1], ids=["caller's weights", "computed weights"])
@pytest.mark.parametrize("mode", rs.PAD_MODES)
@pytest.mark.parametrize("key", sorted(rs.CALL_VIEWS))
def test_psi_start(emu, key, mode, weights_mode):
    fr.check_psi_start(emu, key, mode, weights_mode)


@pytest.mark.parametrize("location", [None, MVN_DEVICE], ids=["host raw stacks", "resident raw stacks"])
def test_psi_start_block_after_block(emu, location):
    fr.check_psi_start_block_after_block(emu, location)


def test_psi_start_with_acceleration_tv_background_and_statistics(emu):
    fr.check_psi_start_composition(emu)


def test_engine_api(emu):
    fr.check_engine_api(emu)


def test_engine_refusals(emu):
    fr.check_engine_refusals(emu)


def test_errors(emu):
    fr.check_errors(emu)


def test_memory_figure(emu):
    fr.check_memory(emu)


def test_counters_and_timing(emu):
    fr.check_counters_and_timing(emu)


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.asan
def test_stand_alone_program_under_sanitizers():
    """tools/fuse_standalone.cpp: a C++ main on the emulation, both under AddressSanitizer + UBSan (csrc/Makefile,
    target fuse-asan).  Nothing is preloaded and nothing is loaded into Python."""
    if not (_runtime("libasan.so") and _runtime("libubsan.so")):
        pytest.skip("no libasan / libubsan next to gcc")
    subprocess.check_call(["make", "-C", CSRC, "fuse-asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "libmultiviewnative_amd", "lib", "fuse_standalone")
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), tail
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
    assert r.stdout.count("fused") == 2, tail
