"""Padding policy "reflect" on the host emulation (csrc/mvn_reflect.hpp; the emulation runs the fill's own bodies): the
call against the library's own "none" call on hand-mirrored stacks bit for bit and against the CPU oracle, every
placement route, cached engines, the loop's switches together, the public surface, and what the policy is for - the
border band of a block cut out of a larger specimen.  The checks live in reflect_reference.py; test_gpu_reflect.py runs
them on the device."""
import os
import subprocess

import numpy as np
import pytest

from libmultiviewnative_amd import native
from oracle import binding as orc
import reflect_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    return native.Binding(native.EMU_SO)


# the suite's pin of the direct dim0 leg (tests/conftest.py) and the product's defaults: see tests/test_gpu_parity.py
@pytest.fixture(params=["suite pin", "product defaults"])
def leg(request, emu, monkeypatch):
    if request.param == "product defaults":
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
        monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    emu.l.mvn_release_cached_engines()
    yield request.param
    emu.l.mvn_release_cached_engines()


def test_the_index_rule_is_numpys_symmetric_extension():
    # the helper the other tests lean on, against np.pad - margins wider than the stack and an extent of 1 included
    rng = np.random.default_rng(3)
    for shape, ext, off in (((3, 5, 2), (12, 7, 8), (4, 1, 3)), ((1, 4, 6), (1, 9, 6), (0, 2, 0)), ((4, 3, 5), (15, 14, 17), (9, 0, 5))):
        a = rng.standard_normal(shape).astype(np.float32)
        pw = [(o, e - n - o) for o, e, n in zip(off, ext, shape)]
        assert np.array_equal(rr.mirror_pad(a, ext, off), np.pad(a, pw, mode="symmetric"))


def test_symbols_declared_exported_bound(emu):
    hdr = open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read()
    exports = open(os.path.join(CSRC, "mvn_exports.map")).read()
    for n in ("mvn_reflect_counters", "mvn_reflect_time"):
        assert n in native.ENGINE_ABI_SYMBOLS
        assert "MVN_API int %s(" % n in hdr, n
        assert "%s;" % n in exports, n
        assert hasattr(emu.l, n)


@pytest.mark.parametrize("name", sorted(rr.PARITY_CASES))
def test_parity_with_hand_mirrored_stacks(emu, leg, name):
    rr.check_parity(emu, orc, name)


@pytest.mark.parametrize("name", sorted(rr.ROUTE_CASES))
def test_every_placement_route(emu, name):
    rr.check_routes(emu, name)


@pytest.mark.parametrize("mem", [None, "stream:1"])
def test_cached_engines_between_zero_and_reflect(emu, mem):
    rr.check_cached_engines(emu, mem)


def test_composition_with_acceleration_tv_background_and_statistics(emu):
    rr.check_composition(emu)


def test_surface(emu, monkeypatch):
    rr.check_surface(emu, monkeypatch)


def test_border_band_of_a_block_cut_out_of_a_larger_specimen(emu):
    rr.check_border_quality(emu)


def test_fill_time_utility(emu):
    # the bench utility runs the fill itself: both element types, and a window it refuses
    before = emu.reflect_counters()
    for u16 in (False, True):
        ms = emu.reflect_time((6, 10, 15), (12, 12, 20), (3, 1, 2), u16=u16, reps=2)
        assert ms[0] >= 0 and ms[1] >= 0
    after = emu.reflect_counters()
    assert after[1] - before[1] == 2 * 3 and after[0] - before[0] == 2 * 3 * 3
    with pytest.raises(native.MvnError):
        emu.reflect_time((6, 10, 15), (12, 12, 16), (3, 1, 2))


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.asan
def test_stand_alone_program_under_sanitizers():
    """tools/reflect_standalone.cpp: a C++ main on the emulation, both under AddressSanitizer + UBSan (csrc/Makefile,
    target reflect-asan).  Nothing is preloaded and nothing is loaded into Python."""
    if not (_runtime("libasan.so") and _runtime("libubsan.so")):
        pytest.skip("no libasan / libubsan next to gcc")
    subprocess.check_call(["make", "-C", CSRC, "reflect-asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "libmultiviewnative_amd", "lib", "reflect_standalone")
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), tail
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
    assert r.stdout.count("filled") == 6, tail
