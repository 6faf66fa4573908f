"""The host code's owning handles (csrc/mvn_backend.hpp: DeviceBuffer, Stream, Event) on the host emulation: an error
path frees what it took.  The emulation counts live device bytes per fake device and refuses an allocation beyond
MVN_EMU_TOTAL_MB (read at every allocation).  For every test and legacy utility of the ABI that allocates scratch: run
it at a small shape S and keep the result; cap the device at what that call needs, rounded up to the MB; run it eight
times at a shape B of about twice the volume, whose first allocation fits and a later one does not - each call must
fail, naming exhausted device memory; then the call at S again under the same cap - it must succeed and give the kept
result bit for bit.  One leaked buffer of one failed call and it cannot.  The same recipe for the engines' resident
state, held in the same owners (csrc/mvn_engine.hpp): an engine and a slab engine that cannot be built, set_view on a
live engine, a streamed call.

Each case runs in a process of its own, so that the count starts at zero: no plan, engine or garbage of another test.
tools/scoped_standalone.cpp runs the same error paths, the group constructor's among them, under AddressSanitizer with
leak detection on."""
import os
import subprocess
import sys

import pytest

from libmultiviewnative_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")

_CHILD = r"""
import ctypes as C, os, sys
import numpy as np
root, name = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import view_geometry
emu = native.Binding(native.EMU_SO)
MB = 1 << 20
S, B = (64, 64, 64), (126, 64, 64)  # even d2: a volume is d0 d1 d2 floats (1 MB, 2016 KB), its Nyquist plane d0 d1 bins
K = (3, 3, 3)
vol = lambda s: 4 * s[0] * s[1] * s[2]
nyq = lambda s: 8 * s[0] * s[1]
rng = np.random.default_rng(5)
data = {s: rng.uniform(1, 2, s).astype(np.float32) for s in (S, B)}
kernel = rng.uniform(0.1, 1, K).astype(np.float32)
kernel /= kernel.sum()
RAW = (8, 8, 8)
raw = rng.uniform(100, 200, RAW).astype(np.float32)
geom = view_geometry(RAW, [[0.1, 0, 0, 0], [0, 0.1, 0, 0], [0, 0, 0.1, 0]], (0, 0, 0), (2, 2, 2))

def void_call(where, f):
    # a void entry point reports through mvn_last_error, which a success leaves alone: first put a message of another
    # call's there
    assert emu.l.mvn_set_pad_mode(b"no such mode") < 0
    out = f()
    err = emu.l.mvn_last_error().decode()
    if not err.startswith("mvn_set_pad_mode"):
        assert err.startswith(where + ":"), err
        raise native.MvnError(err)
    return out

# ---- the engines' resident state (csrc/mvn_engine.hpp): every buffer, stream and event a member that owns it ----
def engine_create(s):  # Engine::Engine: psi, the work volume, its Nyquist plane, the poison words
    e = emu.engine(s, 0)
    try:
        e.set_psi(data[s])
        return e.get_psi()
    finally:
        e.close()

def with_engine_uncapped(s, views):
    cap = os.environ.pop("MVN_EMU_TOTAL_MB", None)
    try:
        return emu.engine(s, views)
    finally:
        if cap is not None:
            os.environ["MVN_EMU_TOTAL_MB"] = cap

def live_set_view(s):
    # the engine itself is built with no cap; the views are then set under it: alloc_view (image, weights), and per
    # kernel prepare_psfs' device copy and prepare_psf's 3-D spectrum with its Nyquist plane (the suite's pin of the
    # direct dim0 leg, tests/conftest.py, holds in this process: no taps at these sizes, no second work volume)
    e = with_engine_uncapped(s, 2)
    try:
        for v in range(2):
            e.set_view(v, data[s] + v, np.full(s, 0.5, np.float32), kernel, kernel)
        e.set_psi(data[s])
        e.iterate(1, 0.006, 1e-4)
        return e.get_psi()
    finally:
        e.close()

def streamed_ring(s):
    # inplace_gpu_deconvolve, 2 views of which 1 streams through a ring of 2 slots, cyclic policy (the engine has the
    # extents of the stacks)
    from libmultiviewnative_amd.abi import WorkspaceHolder
    h = WorkspaceHolder([data[s], data[s] + 1], [kernel] * 2, [kernel] * 2, [np.full(s, 0.5, np.float32)] * 2, 0.006, 1e-4, 2)
    emu.set_pad_mode("none")
    emu.set_memory_mode("stream:1")
    before = emu.stream_counters()
    try:
        out = void_call("inplace_gpu_deconvolve", lambda: emu.gpu_deconvolve(data[s], h, pad_mode=False))
        assert [b - a for a, b in zip(before, emu.stream_counters())][:2] == [1, 2], "the call streamed no view"
        return out
    finally:
        emu.set_memory_mode(None)

def slab_create(s):  # SlabEngine::SlabEngine, rank 0 of 2: psi, work, own_a_, own_b_, then the three Nyquist planes
    e = emu.slab_engine(s, 2, 0, 1)
    try:
        e.set_psi(data[s][:s[0] // 2])
        return e.get_psi()
    finally:
        e.close()

half = lambda s: (s[0] // 2, s[1], s[2])
ENGINE = lambda s: [vol(s), vol(s), nyq(s), 256]
VIEW = lambda s: [vol(s), vol(s)] + [kernel.nbytes, vol(s), nyq(s)] * 2
# stream:1 of 2 views: the engine, the ring's two weights volumes (set_residency) and two image volumes
# (alloc_ring_images), the resident view's pair and the second work volume (reserve_views), then per kernel its device
# copy and 3-D spectrum, and the staging thread's re-tiling scratch
RING = lambda s: ENGINE(s) + [vol(s)] * 2 + [vol(s)] * 2 + [vol(s)] * 2 + [vol(s), nyq(s)] + \
    [kernel.nbytes, vol(s), nyq(s)] * 4 + [vol(s)]

# name -> (the call at a shape, the device allocations of that call in order, timed: the result is a time, plans: the
# call goes through the plan store[, fits: this many leading allocations at B fit under the cap and the next one does
# not[, the refusal's words]])
CASES = {
    "mvn_tv_factor": (lambda s: emu.tv_factor(data[s], 0.005, 0.01), lambda s: [vol(s)] * 2, False, False),
    "mvn_tv_time": (lambda s: emu.tv_time(s, reps=1), lambda s: [vol(s)] * 2, True, False),
    "mvn_reflect_time": (lambda s: emu.reflect_time((s[0] - 4, 60, 60), s, (2, 2, 2), reps=1), lambda s: [vol(s)] * 2, True, False),
    "mvn_resample_stack": (lambda s: np.stack(emu.resample_stack(raw, geom, s, device=0)),
                           lambda s: [vol(s)] * 2 + [raw.nbytes], False, False),
    "mvn_resample_time": (lambda s: emu.resample_time(geom, s, u16=False, reps=1), lambda s: [vol(s)] * 2 + [raw.nbytes], True, False),
    "inplace_gpu_convolution": (lambda s: void_call("inplace_gpu_convolution", lambda: emu.gpu_convolution(data[s], kernel)),
                                lambda s: [vol(s)] * 2 + [nyq(s)] * 2 + [kernel.nbytes], False, True),
    "iterate_fft_plain": (lambda s: void_call("iterate_fft_plain", lambda: emu.iterate_fft(data[s], kernel)),
                          lambda s: [vol(s)] * 3 + [kernel.nbytes, vol(s)] + [nyq(s)] * 2, False, True),
    "compute_quotient": (lambda s: void_call("compute_quotient", lambda: emu.compute_quotient(data[s], data[s] + 1)),
                         lambda s: [vol(s)] * 2, False, False),
    "compute_final_values": (lambda s: void_call("compute_final_values", lambda: emu.compute_final_values(
                                 data[s], data[s] + 1, data[s] * 0.5, 1e-4, 0.006)), lambda s: [vol(s)] * 3, False, False),
    "mvn_fft3_r2c": (lambda s: emu.rfft3(data[s]), lambda s: [vol(s), nyq(s)], False, True),
    "mvn_fft3_many_r2c": (lambda s: emu.rfft3_many(np.stack([data[s], data[s] * 2, data[s] + 1])),
                          lambda s: [vol(s), nyq(s)] * 3, False, True),
    "mvn_fft3_many_time": (lambda s: emu.fft3_many_time(s, 3, reps=1), lambda s: [vol(s), nyq(s)] * 3, True, True),
    # psi fits, the work volume does not
    "mvn_engine_create": (engine_create, ENGINE, False, True, 1),
    # view 0 gets its image, weights and first spectrum; the second spectrum's main array does not fit
    "mvn_engine_set_view": (live_set_view, lambda s: ENGINE(s) + VIEW(s) * 2, False, True, 10),
    # The planner (plan_engine, csrc/mvn_abi.cpp) prices the call by Engine::memory_need against the same total before
    # anything is allocated, and that model is exact (tests/test_emu_streamed_views.py): under ANY cap a streamed call
    # either fits whole or is refused there, in the reference's words - no cap makes alloc_ring_images, or any other
    # allocation of the call, fail.  What the case does check: the engine the call at S left in the cache - ring slots,
    # their events, the upload stream - is dropped by the refused calls, and everything it held is free again.
    "streamed_ring": (streamed_ring, RING, False, True, None, "memory constraints"),
    # own_a_ fits, own_b_ does not
    "mvn_slab_create": (slab_create, lambda s: [vol(half(s))] * 4 + [nyq(half(s))] * 3, False, True, 3),
}
call, allocations, timed, plans = CASES[name][:4]
fits = CASES[name][4] if len(CASES[name]) > 4 else None
refusal = CASES[name][5] if len(CASES[name]) > 5 else "device memory exhausted"
emu.check(emu.l.mvn_release_cached_engines())
kept = call(S)  # (uncapped; the plan's small device tables stay in the store and are counted from here on)
cap = -(-sum(allocations(S)) // MB)
# the tables of the plans of S and B (a few KB each) must fit beside the call at S, and beside the first allocation at B
TABLES = 24 << 10 if plans else 0
assert sum(allocations(S)) + TABLES <= cap * MB and allocations(B)[0] + TABLES <= cap * MB < sum(allocations(B)), name
if fits:
    assert sum(allocations(B)[:fits]) + TABLES <= cap * MB < sum(allocations(B)[:fits + 1]), name
os.environ["MVN_EMU_TOTAL_MB"] = str(cap)
for i in range(8):
    try:
        call(B)
    except native.MvnError as e:
        assert refusal in str(e), (name, i, str(e))
    else:
        raise AssertionError("%s: call %d at %r succeeded under a cap of %d MB" % (name, i, B, cap))
again = call(S)
if timed:
    assert all(np.isfinite(t) and t >= 0 for t in np.atleast_1d(again)) and np.shape(again) == np.shape(kept), (again, kept)
else:
    assert np.asarray(again).tobytes() == np.asarray(kept).tobytes(), name
print("ok")
"""

CASES = ["mvn_tv_factor", "mvn_tv_time", "mvn_reflect_time", "mvn_resample_stack", "mvn_resample_time",
         "inplace_gpu_convolution", "iterate_fft_plain", "compute_quotient", "compute_final_values", "mvn_fft3_r2c",
         "mvn_fft3_many_r2c", "mvn_fft3_many_time", "mvn_engine_create", "mvn_engine_set_view", "streamed_ring",
         "mvn_slab_create"]


@pytest.fixture(scope="module")
def emu_built():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])


@pytest.mark.parametrize("name", CASES)
def test_error_paths_free_what_they_took(emu_built, name):
    """(a timing utility's result is a time: the last call must succeed with finite times, not repeat them)"""
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("MVN_EMU_TOTAL_MB", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.asan
def test_stand_alone_program_under_sanitizers_with_leak_detection():
    """tools/scoped_standalone.cpp: a C++ main on the emulation, both under AddressSanitizer + UBSan (csrc/Makefile,
    target scoped-asan), leak detection ON.  Nothing is preloaded and nothing is loaded into Python."""
    if not (_runtime("libasan.so") and _runtime("libubsan.so")):
        pytest.skip("no libasan / libubsan next to gcc")
    subprocess.check_call(["make", "-C", CSRC, "scoped-asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "libmultiviewnative_amd", "lib", "scoped_standalone")
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1",
               MVN_EMU_DEVICES="2")
    env.pop("LD_PRELOAD", None)
    env.pop("MVN_EMU_TOTAL_MB", None)
    # the product's defaults, not the suite's pin of the direct dim0 leg (tests/conftest.py): a group needs that leg
    env.pop("MVN_DIM0_DIRECT_MIN_ITEMS", None)
    env.pop("MVN_DIM0_DIRECT_MIN_PLANE", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), tail
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
