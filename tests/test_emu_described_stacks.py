"""Described stacks (mvn_deconvolve_described, mvn_engine_*_described; include/mvn_engine_api.h) on the host emulation:
uint16, strided and "device"-located stacks give, bit for bit, what inplace_gpu_deconvolve gives on the same values as
dense float32 host arrays.  The emulation accepts any pointer as device memory, so the device path of the ingest /
extract passes (csrc/mvn_ingest.hpp) runs here on host arrays; tests/test_gpu_described_stacks.py runs it on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_DEVICE, MVN_HOST, CallDesc, StackDesc, WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")
MB = 1 << 20
SHAPES = [(32, 128, 126), (20, 36, 45)]
V, ITERS = 3, 2


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    return native.Binding(native.EMU_SO)


_CASES = {}


def case(shape):
    if shape not in _CASES:
        _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=11)
        _CASES[shape] = (views, k1, k2, w, psi0)
    return _CASES[shape]


def plain(b, shape, lam, pad, views=None):
    vs, k1, k2, w, psi0 = case(shape)
    h = WorkspaceHolder(vs if views is None else views, k1, k2, w, lam, 1e-4, ITERS)
    return b.gpu_deconvolve(psi0, h, pad_mode=pad), h


def relabeled(c, locations):
    """a prepared call (Binding.describe_call) with the locations of some of its stacks overwritten"""
    for key, loc in (locations or {}).items():
        if key == "psi":
            c.desc.psi.location = loc
        else:
            getattr(c, key[0])[key[1]].location = loc
    return c


def described(b, psi, views, weights, shape, lam, pad, locations=None):
    _, k1, k2, _, _ = case(shape)
    before = b.get_pad_mode()
    b.set_pad_mode(pad)
    try:
        return relabeled(b.describe_call(psi, views, weights, k1, k2, lam, 1e-4, ITERS), locations).run()
    finally:
        b.set_pad_mode(before)


def window(a, off=(3, 5, 7), fill=-7.0):
    """`a` as a window of a larger array of the same dtype"""
    big = np.full(tuple(s + 2 * o + 1 for s, o in zip(a.shape, off)), fill, a.dtype)
    win = big[off[0]:off[0] + a.shape[0], off[1]:off[1] + a.shape[1], off[2]:off[2] + a.shape[2]]
    win[...] = a
    return big, win


ALL_DEVICE = dict([("psi", MVN_DEVICE)] + [((k, v), MVN_DEVICE) for k in ("image", "weights") for v in range(V)])


@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dense_float32_through_descriptors(emu, shape, lam, pad):
    views, _, _, w, psi0 = case(shape)
    ref, h = plain(emu, shape, lam, pad)
    got = described(emu, psi0.copy(), views, w, shape, lam, pad)
    assert np.array_equal(got, ref)
    # the same stacks said to be in device memory: the ingest pass reads them where they lie
    got = described(emu, psi0.copy(), views, w, shape, lam, pad, locations=ALL_DEVICE)
    assert np.array_equal(got, ref)
    if pad == "none":  # the anchor outside the code under test
        o = orc.cpu_deconvolve(psi0, h, 4)
        assert np.abs(got - o).max() <= 1e-4 * np.abs(o).max()


@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_uint16_images(emu, shape, lam, pad):
    views, _, _, w, psi0 = case(shape)
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    assert all(0 < int(u.min()) and int(u.max()) < 65535 for u in u16)
    ref, _ = plain(emu, shape, lam, pad, views=[u.astype(np.float32) for u in u16])
    assert np.array_equal(described(emu, psi0.copy(), u16, w, shape, lam, pad), ref)
    loc = {("image", v): MVN_DEVICE for v in range(V)}
    assert np.array_equal(described(emu, psi0.copy(), u16, w, shape, lam, pad, locations=loc), ref)


@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_strided_stacks(emu, shape, lam, pad):
    views, _, _, w, psi0 = case(shape)
    ref, _ = plain(emu, shape, lam, pad)
    wins = [window(v)[1] for v in views]
    wins[1] = np.ascontiguousarray(views[1].transpose(2, 1, 0)).transpose(2, 1, 0)  # stride[2] != 1: "device" memory
    assert wins[1].strides[2] != 4 and np.array_equal(wins[1], views[1])
    consts = [np.broadcast_to(np.float32(1.0 / V), shape) for _ in range(V)]
    assert consts[0].strides == (0, 0, 0) and all(np.array_equal(c, x) for c, x in zip(consts, w))
    big, psi = window(psi0)
    frame = big.copy()
    got = described(emu, psi, wins, consts, shape, lam, pad, locations={("image", 1): MVN_DEVICE})
    assert got is psi and np.array_equal(psi, ref)
    inside = np.zeros(big.shape, bool)
    inside[3:3 + shape[0], 5:5 + shape[1], 7:7 + shape[2]] = True
    assert np.array_equal(big[~inside], frame[~inside]), "the call wrote outside psi's window"
    # the same with every stack in "device" memory (broadcast weights and the window of psi included)
    big2, psi2 = window(psi0)
    described(emu, psi2, wins, consts, shape, lam, pad, locations=ALL_DEVICE)
    assert np.array_equal(psi2, ref) and np.array_equal(big2[~inside], frame[~inside])


_CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder, MVN_DEVICE
from ref_fixtures import realistic_views
emu = native.Binding(native.EMU_SO)
def relabeled(c, locations):
    for key, loc in (locations or {}).items():
        if key == "psi":
            c.desc.psi.location = loc
        else:
            getattr(c, key[0])[key[1]].location = loc
    return c
what, pad = sys.argv[2], sys.argv[3]
MB = 1 << 20
V = 3
shape = (32, 128, 126)
_, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=11)
h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
emu.set_pad_mode(pad)
ref = emu.gpu_deconvolve(psi0, h, pad_mode=False)
emu.check(emu.l.mvn_release_cached_engines())
emu.check(emu.l.mvn_plan_store_clear())
need = emu.deconvolve_memory(h, 0)
u16 = [np.rint(v).astype(np.uint16) for v in views]
ref16 = emu.gpu_deconvolve(psi0, WorkspaceHolder([u.astype(np.float32) for u in u16], k1, k2, w, 0.006, 1e-4, 2), pad_mode=False)
emu.check(emu.l.mvn_release_cached_engines())
emu.check(emu.l.mvn_plan_store_clear())
if what == "host":
    # host-located described stacks: the model's figure is what the call allocates ("auto": the exact planner)
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need // MB))
    emu.set_memory_mode("auto")
    before = emu.stream_counters()
    got = emu.deconvolve_described(psi0.copy(), u16, w, k1, k2, 0.006, 1e-4, 2)
    assert emu.stream_counters() == before, "the call streamed views"
    assert np.array_equal(got, ref16)
else:
    # every stack in "device" memory: resident whatever the mode, and without the embedding scratch
    scratch = 4 * shape[0] * shape[1] * shape[2] if pad != "none" else 0
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-(need - scratch) // MB))
    emu.set_memory_mode("stream")
    loc = dict([("psi", MVN_DEVICE)] + [((k, v), MVN_DEVICE) for k in ("image", "weights") for v in range(V)])
    before = emu.stream_counters()
    got = relabeled(emu.describe_call(psi0.copy(), views, w, k1, k2, 0.006, 1e-4, 2), loc).run()
    assert emu.stream_counters() == before, "the call streamed views"
    assert np.array_equal(got, ref)
    # ... and refused cleanly, psi untouched, when even that does not fit
    emu.check(emu.l.mvn_release_cached_engines())
    emu.check(emu.l.mvn_plan_store_clear())
    os.environ["MVN_EMU_TOTAL_MB"] = str((need - scratch) // MB - 2)
    psi = psi0.copy()
    try:
        relabeled(emu.describe_call(psi, views, w, k1, k2, 0.006, 1e-4, 2), loc).run()
        raise SystemExit("not refused")
    except native.MvnError as e:
        assert "memory constraints" in str(e), e
    assert np.array_equal(psi, psi0)
assert not emu.l.mvn_last_error().decode() or what != "host"
print("ok")
"""


def _child(what, pad, env_extra=None, timeout=900):
    env = dict(os.environ, OMP_NUM_THREADS="4", **(env_extra or {}))
    env.pop("MVN_EMU_TOTAL_MB", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, what, pad], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0 and "ok" in r.stdout.split("\n")[-2], (r.stdout[-2000:], r.stderr[-4000:])
    assert "exhausted" not in r.stderr, r.stderr[-4000:]
    return r


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("pad", ["none", "zero"])
def test_memory_model_holds_for_described_calls(emu, pad, where):
    _child(where, pad)


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_streamed_uint16_views_stream_uint16(emu, pad):
    shape = SHAPES[1]
    views, _, _, w, psi0 = case(shape)
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    ref = described(emu, psi0.copy(), u16, w, shape, 0.006, pad)
    emu.set_memory_mode("stream:%d" % V)
    try:
        before = emu.stream_counters()
        got = described(emu, psi0.copy(), u16, w, shape, 0.006, pad)
        d = [b - a for a, b in zip(before, emu.stream_counters())]
    finally:
        emu.set_memory_mode(None)
        emu.l.mvn_release_cached_engines()
    assert np.array_equal(got, ref)
    assert d[0] == 1 and d[1] == V * ITERS, d
    assert d[2] == V * ITERS * (u16[0].nbytes + w[0].nbytes), d


def _raw_call(emu, shape, psi, psi_desc, image_descs=None, weights_descs=None):
    import ctypes as C
    views, k1, k2, w, _ = case(shape)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, ITERS)
    call = CallDesc()
    call.psi = psi_desc
    keep = []
    for name, descs in (("image", image_descs), ("weights", weights_descs)):
        if descs is not None:
            arr = (StackDesc * V)(*descs)
            keep.append(arr)
            setattr(call, name, C.cast(arr, C.POINTER(StackDesc)))
    return emu.l.mvn_deconvolve_described(C.c_void_p(psi.ctypes.data), h.ws, C.byref(call), 0)


def _desc(shape, dtype=0, location=MVN_HOST, stride=None):
    d = StackDesc()
    d.dtype, d.location = dtype, location
    for k, s in enumerate(stride or (shape[1] * shape[2], shape[2], 1)):
        d.stride[k] = s
    return d


def test_errors_leave_psi_untouched(emu):
    shape = SHAPES[1]
    psi0 = case(shape)[4]
    dense = (shape[1] * shape[2], shape[2], 1)
    bad = {
        "uint16 weights": dict(weights_descs=[_desc(shape, dtype=1)] * V),
        "psi with a zero stride": dict(psi_desc=_desc(shape, stride=(dense[0], 0, 1))),
        "negative stride": dict(image_descs=[_desc(shape, stride=(dense[0], -dense[1], 1))] * V),
        "negative psi stride": dict(psi_desc=_desc(shape, stride=(-dense[0], dense[1], 1))),
        "dtype 7": dict(image_descs=[_desc(shape, dtype=7)] * V),
        "location 5": dict(image_descs=[_desc(shape, location=5)] * V),
        "host stack with stride[2] != 1": dict(image_descs=[_desc(shape, stride=(dense[0] * 2, dense[1] * 2, 2))] * V),
    }
    emu.set_pad_mode("none")
    try:
        for what, kw in bad.items():
            psi = psi0.copy()
            kw.setdefault("psi_desc", _desc(shape))
            rc = _raw_call(emu, shape, psi, **kw)
            assert rc < 0, what
            assert emu.l.mvn_last_error().decode().startswith("mvn_deconvolve_described"), what
            assert np.array_equal(psi, psi0), what
        # no descriptor arrays (dense float32 in host memory) with psi in "device" memory: fine
        psi = psi0.copy()
        assert _raw_call(emu, shape, psi, _desc(shape, location=MVN_DEVICE)) == 0
        assert np.array_equal(psi, plain(emu, shape, 0.006, "none")[0])
    finally:
        emu.set_pad_mode(None)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_resident_engine_takes_described_stacks(emu, shape):
    views, k1, k2, w, psi0 = case(shape)
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    a = emu.engine(shape, V)
    b = emu.engine(shape, V)
    try:
        for v in range(V):
            # (layouts the described symbols refuse in host memory are copied, as before: Fortran order, reversed)
            a.set_view(v, np.asfortranarray(u16[v].astype(np.float32)), w[v][::-1], k1[v], k2[v])
            img = window(u16[v], off=(1, 2, 3), fill=9)[1] if v else u16[v]
            b.set_view(v, img, np.broadcast_to(np.float32(1.0 / V), shape) if v == 1 else window(w[v])[1], k1[v], k2[v])
        a.set_psi(psi0)
        b.set_psi(window(psi0)[1])
        a.iterate(ITERS, 0.006, 1e-4)
        b.iterate(ITERS, 0.006, 1e-4)
        ref = a.get_psi()
        assert np.array_equal(b.get_psi(), ref)
        big, out = window(np.zeros(shape, np.float32))
        assert b.get_psi(out) is out and np.array_equal(out, ref)
        assert big[0, 0, 0] == -7.0 and big[-1, -1, -1] == -7.0
    finally:
        a.close()
        b.close()


def test_convergence_statistics_of_a_described_call(emu):
    shape = SHAPES[1]
    views, _, _, w, psi0 = case(shape)
    emu.set_convergence(0.0)
    try:
        for pad in ("none", "zero"):
            ref, _ = plain(emu, shape, 0.006, pad)
            run0, rows0 = emu.last_convergence()
            got = described(emu, window(psi0)[1], [window(v)[1] for v in views], w, shape, 0.006, pad)
            run1, rows1 = emu.last_convergence()
            assert np.array_equal(got, ref)
            assert run0 == run1 == ITERS and rows0.shape == (ITERS, 3) and np.array_equal(rows0, rows1)
    finally:
        emu.set_convergence(-1.0)


# ---- the blocking branch of the ABI call (MVN_NO_PIPELINE, read once per process: a child) ---------------------------
_BLOCKING_CHILD = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import test_emu_described_stacks as t
emu = native.Binding(native.EMU_SO)
for pad in t.BLOCKING_PADS:
    plain, desc = t.blocking_calls(emu, pad)
    np.save(os.path.join(out, "plain_%s.npy" % pad), plain)
    np.save(os.path.join(out, "described_%s.npy" % pad), desc)
assert not emu.l.mvn_last_error().decode(), emu.l.mvn_last_error().decode()
print("blocking child ok", flush=True)
"""

BLOCKING_PADS = ("none", "zero")


def blocking_calls(b, pad):
    """one plain call, and one described call with uint16 images in unaligned windows and psi in a window"""
    shape = SHAPES[1]  # odd last extent: rows are padded and the pitched copy runs; "zero" embeds the stacks
    views, _, _, w, psi0 = case(shape)
    u16 = [window(np.rint(v).astype(np.uint16), off=(1, 2, 3), fill=9)[1] for v in views]
    return plain(b, shape, 0.006, pad)[0], described(b, window(psi0)[1], u16, w, shape, 0.006, pad).copy()


def test_blocking_call_gives_what_the_pipelined_call_gives(emu, tmp_path):
    # the library against itself on another code path, bit for bit (the anchor outside it: the oracle comparison of
    # test_dense_float32_through_descriptors)
    env = dict(os.environ, OMP_NUM_THREADS="4", MVN_NO_PIPELINE="1", MVN_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _BLOCKING_CHILD, ROOT, str(tmp_path)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "blocking child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    # the child took the blocking branch: its calls were traced, and none of them started the uploader thread
    assert "[lmvn::inplace_gpu_deconvolve]" in r.stdout and "(uploader thread)" not in r.stdout, r.stdout[-4000:]
    for pad in BLOCKING_PADS:
        ref, ref16 = blocking_calls(emu, pad)
        assert not np.array_equal(ref, case(SHAPES[1])[4]) and not np.array_equal(ref16, ref)
        assert np.array_equal(np.load(str(tmp_path / ("plain_%s.npy" % pad))), ref), pad
        assert np.array_equal(np.load(str(tmp_path / ("described_%s.npy" % pad))), ref16), pad


_ASAN_CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder, MVN_DEVICE
from ref_fixtures import realistic_views
emu = native.Binding(native.EMU_SO)
def relabeled(c, locations):
    for key, loc in (locations or {}).items():
        if key == "psi":
            c.desc.psi.location = loc
        else:
            getattr(c, key[0])[key[1]].location = loc
    return c
V = 3
shape = (20, 36, 45)   # odd extents: head and tail groups of the 16-byte form in every row
_, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=11)
u16 = [np.rint(v).astype(np.uint16) for v in views]
def win(a, x):  # an unaligned window that ENDS where its array ends: an overread leaves the allocation
    big = np.zeros((a.shape[0], a.shape[1], a.shape[2] + x), a.dtype)
    big[..., x:] = a
    return big[..., x:x + a.shape[2]]
loc = dict([("psi", MVN_DEVICE)] + [((k, v), MVN_DEVICE) for k in ("image", "weights") for v in range(V)])
for pad in ("none", "zero"):
    emu.set_pad_mode(pad)
    ref = emu.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2), pad_mode=False)
    ref16 = emu.gpu_deconvolve(psi0, WorkspaceHolder([u.astype(np.float32) for u in u16], k1, k2, w, 0.006, 1e-4, 2),
                               pad_mode=False)
    for l in (None, loc):
        got = relabeled(emu.describe_call(win(psi0, 1).copy(), [win(v, 1) for v in views], w, k1, k2, 0.006, 1e-4, 2), l).run()
        assert np.array_equal(got, ref)
        got = relabeled(emu.describe_call(win(psi0, 1), [win(u, 3) for u in u16], [win(x, 1) for x in w], k1, k2, 0.006,
                                          1e-4, 2), l).run()
        assert np.array_equal(got, ref16)
print("ok")
"""


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.asan
def test_described_stacks_under_asan():
    asan, ubsan = _runtime("libasan.so"), _runtime("libubsan.so")
    if not (asan and ubsan):
        pytest.skip("no libasan / libubsan next to gcc")
    subprocess.check_call(["make", "-C", CSRC, "emu-asan"], stdout=subprocess.DEVNULL)
    so = os.path.join(ROOT, "libmultiviewnative_amd", "lib", "libmvn_emu_asan.so")
    env = dict(os.environ, OMP_NUM_THREADS="4", LD_PRELOAD=asan + ":" + ubsan, MVN_EMU_SO=so,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", _ASAN_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
