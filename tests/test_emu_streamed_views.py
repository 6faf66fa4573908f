"""Out-of-core views of inplace_gpu_deconvolve (memory modes auto / stream / stream:N, csrc/mvn_abi.cpp) on the
host emulation: the exact memory model (Engine::memory_need) against the emulation's device-memory total (an
allocation beyond it fails), and streamed calls bit for bit against resident ones.  The emulation's copies are synchronous and its stream waits are
no-ops, so these tests check the bookkeeping and the arithmetic; tests/test_gpu_streamed_views.py checks the ordering
of the uploads against the compute on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")
MB = 1 << 20

_CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views
emu = native.Binding(native.EMU_SO)
what, pad, V, s_arg, kernels = sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5], sys.argv[6]
MB = 1 << 20
# kernels "exact*": d1 + 4 = 128, a multiple of 16, so that the zero policy may keep dim0 exact: 34 + 4 = 38 planes
# when every PSF is held in the direct form, else good_extent(38) = 40
shape = (34, 124, 126) if kernels.startswith("exact") else (32, 128, 126)
_, views, k1, k2, w, psi0 = realistic_views(shape, V, (21 if kernels == "mixed" else 5, 5, 5), seed=11)
k2 = [np.ascontiguousarray(k[k.shape[0] // 2 - 1:k.shape[0] // 2 + 2]) for k in k2]  # (3 planes: another tap plan)
if kernels == "mixed":  # PSF depths 21, 17, 15 across the views: under MVN_DIM0_DIRECT_MAX=17 one 3-D spectrum and
    # direct forms of two tap depths (32, 16) in one call
    k1 = [np.ascontiguousarray(k[(21 - d) // 2:(21 - d) // 2 + d]) for d, k in zip([21, 17, 15] * V, k1)]
h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
emu.set_pad_mode(pad)

def fresh():  # nothing of an earlier call stays allocated: no cached engine, no plans
    emu.check(emu.l.mvn_plan_store_clear())

def call(mode):
    emu.set_memory_mode(mode)
    before = emu.stream_counters()
    try:
        got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    finally:
        emu.set_memory_mode(None)
    return got, [b - a for a, b in zip(before, emu.stream_counters())]

if what == "exact":
    # the call runs in exactly the memory the model names (rounded up to the MB): an undercount fails an allocation
    s = V if s_arg == "V" else int(s_arg)
    need = emu.deconvolve_memory(h, s)
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need // MB))
    got, d = call("auto" if s == 0 else "stream:%d" % s)
    assert d == ([0, 0, 0] if s == 0 else [1, 2 * s, d[2]]), d
    assert np.isfinite(got).all() and not np.array_equal(got, psi0), "the call did not run"
    err = emu.l.mvn_last_error().decode()
    assert not err, err
    if kernels.startswith("exact"):  # the extents the call ran on: dim0 exact (38) or padded (40), never both
        import ctypes
        def has(d0):
            return any(emu.l.mvn_plan_store_has_key(0, (ctypes.c_int * 3)(d0, 128, e2)) == 1 for e2 in range(130, 180))
        want = 38 if kernels == "exact" else 40
        assert has(want) and not has(78 - want), (has(38), has(40))
    # one MB less: auto streams more views, or refuses cleanly - never a failed allocation
    fresh()
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need // MB) - 1)
    less, d2 = call("auto")
    err = emu.l.mvn_last_error().decode()
    if "memory constraints" in err:
        assert np.array_equal(less, psi0)
    else:  # (a plan of s >= 1 views may give way to any other that fits; the resident one to streaming)
        assert not err, err
        assert d2[0] == 1 or s > 0, (d2, s)
        assert np.array_equal(less, got)
    print("ok")
elif what == "identical":
    # a call the resident mode refuses runs in auto mode with streamed views and gives the resident result
    ref, _ = call("resident")
    if pad == "none":
        o = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(ref - o).max() <= 1e-4 * np.abs(o).max()
    fresh()
    need0 = emu.deconvolve_memory(h, 0)
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need0 // MB) - 1)
    if os.environ.get("MVN_DIM0_DIRECT_MIN_ITEMS") == "0":
        # taps instead of 3-D spectra: the resident mode's estimate (4 volumes per view) asks for far more than the
        # call needs (with 3-D spectra it is close to the exact figure, and no larger)
        refused, _ = call("resident")
        assert np.array_equal(refused, psi0) and "memory constraints" in emu.l.mvn_last_error().decode()
    got, d = call("auto")
    assert d[0] == 1 and d[1] >= 2 and d[1] % 2 == 0, d
    s = d[1] // 2
    assert d[2] == d[1] * 2 * views[0].nbytes, d
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    print("ok", s)
elif what == "refuse":
    # not even every view streamed with one ring slot fits: refused, psi untouched, the next call works
    need_min = emu.deconvolve_memory(h, V) - (emu.deconvolve_memory(h, 1) - emu.deconvolve_memory(h, 0))
    os.environ["MVN_EMU_TOTAL_MB"] = str(need_min // MB - 1)
    for mode in ("auto", "stream"):
        got, d = call(mode)
        assert np.array_equal(got, psi0) and d == [0, 0, 0]
        assert "memory constraints" in emu.l.mvn_last_error().decode()
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need_min // MB))
    got, d = call("auto")
    assert d[0] == 1 and d[1] == 2 * V and np.isfinite(got).all(), d
    print("ok")
"""


def _child(what, pad, V, s, direct=False, env_extra=None, timeout=900, kernels="same"):
    env = dict(os.environ, OMP_NUM_THREADS="4", **(env_extra or {}))
    env.pop("MVN_EMU_TOTAL_MB", None)
    if direct:  # the direct dim0 leg (taps) at this size: the suite pins it to large volumes (tests/conftest.py)
        env["MVN_DIM0_DIRECT_MIN_ITEMS"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, what, pad, str(V), str(s), kernels], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ok" in r.stdout.split("\n")[-2], (r.stdout[-2000:], r.stderr[-4000:])
    assert "exhausted" not in r.stderr, r.stderr[-4000:]
    return r


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    return native.Binding(native.EMU_SO)


@pytest.mark.parametrize("pad, form, s, kernels", [
    pytest.param(pad, form, s, "same", id="%s-%s-%s" % (pad, form, s))
    for pad in ("none", "zero") for form in ("fft", "direct") for s in ("0", "1", "V")] + [
    # PSF depths differ across the views: one rule decides the form of every kernel (a 3-D spectrum, two tap depths)
    pytest.param("zero", "direct", "1", "mixed", id="zero-direct-1-mixed"),
    # dim0 kept at image + kernel - 1 by that rule, before the engine exists / padded when the rule refuses a PSF
    pytest.param("zero", "direct", "0", "exact", id="zero-direct-0-exact"),
    pytest.param("zero", "direct", "0", "exact-refused", id="zero-direct-0-exact-refused"),
])
def test_memory_model_is_exact(emu, pad, form, s, kernels):
    extra = {"mixed": {"MVN_DIM0_DIRECT_MAX": "17"}, "exact-refused": {"MVN_DIM0_DIRECT_MAX": "4"}}.get(kernels)
    _child("exact", pad, 3, s, direct=form == "direct", env_extra=extra, kernels=kernels)


@pytest.mark.parametrize("form", ["fft", "direct"])
@pytest.mark.parametrize("pad", ["none", "zero"])
def test_auto_streams_what_resident_refuses_bit_identically(emu, pad, form):
    _child("identical", pad, 4, 0, direct=form == "direct")


def test_refusal_when_nothing_fits(emu):
    _child("refuse", "none", 3, 0)


def test_model_prices_the_plan(emu):
    # one streamed view less resident = one image + weights pair; a ring slot = one pair
    _, views, k1, k2, w, psi0 = realistic_views((16, 20, 24), 4, (5, 5, 5), seed=1)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    before = emu.get_pad_mode()
    emu.set_pad_mode("none")
    try:
        need = [emu.deconvolve_memory(h, s) for s in range(5)]
    finally:
        emu.set_pad_mode(before)
    pair = need[1] - need[0]
    assert pair >= 2 * 16 * 20 * 24 * 4
    assert all(need[s] - need[s + 1] == pair for s in range(1, 4)), need
    with pytest.raises(native.MvnError):
        emu.deconvolve_memory(h, 5)


def test_memory_mode_switch(emu):
    assert emu.get_memory_mode() is None
    for m in ("resident", "auto", "stream", "stream:3"):
        emu.set_memory_mode(m)
        assert emu.get_memory_mode() == m
    with pytest.raises(native.MvnError):
        emu.set_memory_mode("streaming")
    emu.set_memory_mode(None)
    assert emu.get_memory_mode() is None


def _stream_case(shape, V, lam, seed):
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 3, 5), seed=seed)
    return WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3), psi0


def _run(emu, h, psi0, mode, pad="none"):
    emu.set_memory_mode(mode)
    try:
        before = emu.stream_counters()
        got = emu.gpu_deconvolve(psi0, h, pad_mode=pad)
        return got, [b - a for a, b in zip(before, emu.stream_counters())]
    finally:
        emu.set_memory_mode(None)


@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("V", [1, 2, 3, 4])
def test_stream_mode_is_bit_identical(emu, V, lam):
    # every view streamed, odd d2 (padded rows in the ring slots), the cached engine replaced between the modes
    h, psi0 = _stream_case((12, 18, 17), V, lam, 20 + V)
    ref, d0 = _run(emu, h, psi0, "resident")
    got, d = _run(emu, h, psi0, "stream")
    assert d0 == [0, 0, 0] and d[:2] == [1, 3 * V], d
    assert np.array_equal(got, ref)
    o = orc.cpu_deconvolve(psi0, h, 4)
    assert np.abs(got - o).max() <= 1e-4 * np.abs(o).max()
    # stream:N on a cached engine of another plan, and the default policy (embedded stacks in the ring)
    for n in range(V + 1):
        got, d = _run(emu, h, psi0, "stream:%d" % n)
        assert d[1] == 3 * n and np.array_equal(got, ref), n
    got, d = _run(emu, h, psi0, "resident")  # (the cached engine of the last plan streams: not re-used here)
    assert d == [0, 0, 0] and np.array_equal(got, ref)
    ref_z, _ = _run(emu, h, psi0, "resident", pad="zero")
    got_z, d = _run(emu, h, psi0, "stream", pad="zero")
    assert d[1] == 3 * V and np.array_equal(got_z, ref_z)
    emu.l.mvn_release_cached_engines()


def test_submit_wait_streamed_blocks_match_blocking_calls(emu):
    blocks = [_stream_case((12, 18, 16), 3, 0.006, 40 + b) for b in range(3)]
    refs = [_run(emu, h, psi0, "resident")[0] for h, psi0 in blocks]
    emu.set_pad_mode("none")
    emu.set_memory_mode("auto")
    emu.set_memory_budget(emu.deconvolve_memory(blocks[0][0], 0) - 1)  # resident does not fit: views stream
    try:
        before = emu.stream_counters()
        outs = [psi0.copy() for _, psi0 in blocks]
        tickets = [emu.deconvolve_submit(o, h) for o, (h, _) in zip(outs, blocks)]
        for t in tickets:
            emu.deconvolve_wait(t)
        d = [b - a for a, b in zip(before, emu.stream_counters())]
    finally:
        emu.set_memory_budget(None)
        emu.set_memory_mode(None)
        emu.set_pad_mode(None)
        emu.l.mvn_release_cached_engines()
    assert d[0] == 3 and d[1] >= 3 * 3 * 2, d
    for o, r in zip(outs, refs):
        assert np.array_equal(o, r)


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.asan
def test_streamed_call_under_asan():
    asan, ubsan = _runtime("libasan.so"), _runtime("libubsan.so")
    if not (asan and ubsan):
        pytest.skip("no libasan / libubsan next to gcc")
    subprocess.check_call(["make", "-C", CSRC, "emu-asan"], stdout=subprocess.DEVNULL)
    so = os.path.join(ROOT, "libmultiviewnative_amd", "lib", "libmvn_emu_asan.so")
    r = _child("identical", "zero", 3, 0, direct=True, timeout=1500,
               env_extra={"LD_PRELOAD": asan + ":" + ubsan, "MVN_EMU_SO": so,
                          "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
