"""Described stacks on the MI355X (mvn_deconvolve_described, mvn_engine_*_described; csrc/mvn_ingest.hpp): uint16,
strided and device-resident stacks give, bit for bit, what inplace_gpu_deconvolve gives on the same values as dense
float32 host arrays.  The in-process cases use host memory only; one child process (torch imported first, as
INTEGRATION.md section 3 asks) hands over cuda tensors produced on a side stream without a host synchronise, so that
the library's event on that stream is what orders its reads."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd.abi import MVN_DEVICE, MVN_HOST, CallDesc, StackDesc, WorkspaceHolder
from ref_fixtures import realistic_views

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, V, ITERS = (64, 64, 128), 4, 3


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    return b


def make_stacks():
    _, views, k1, k2, w, psi0 = realistic_views(SHAPE, V, (7, 5, 5), seed=71)
    return views, k1, k2, w, psi0


@pytest.fixture(scope="module")
def stacks():
    return make_stacks()


def plain(gpu, stacks, lam, pad, views=None):
    vs, k1, k2, w, psi0 = stacks
    h = WorkspaceHolder(vs if views is None else views, k1, k2, w, lam, 1e-4, ITERS)
    got = gpu.gpu_deconvolve(psi0, h, pad_mode=pad)
    assert not np.array_equal(got, psi0), gpu.l.mvn_last_error().decode()
    return got


def described(gpu, stacks, psi, views, weights, lam, pad, iters=ITERS):
    _, k1, k2, _, _ = stacks
    before = gpu.get_pad_mode()
    gpu.set_pad_mode(pad)
    try:
        return gpu.deconvolve_described(psi, views, weights, k1, k2, lam, 1e-4, iters)
    finally:
        gpu.set_pad_mode(before)


def window(a, off=(3, 5, 7), fill=-7.0):
    big = np.full(tuple(s + 2 * o + 1 for s, o in zip(a.shape, off)), fill, a.dtype)
    win = big[off[0]:off[0] + a.shape[0], off[1]:off[1] + a.shape[1], off[2]:off[2] + a.shape[2]]
    win[...] = a
    return big, win


@pytest.mark.parametrize("pad", ["none", "zero", "zero_exact"])
@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_host_stacks_dense_uint16_strided(gpu, stacks, lam, pad):
    views, _, _, w, psi0 = stacks
    ref = plain(gpu, stacks, lam, pad)
    if pad == "none":  # the anchor outside the code under test
        from oracle import binding as orc
        o = orc.cpu_deconvolve(psi0, WorkspaceHolder(views, stacks[1], stacks[2], w, lam, 1e-4, ITERS), 4)
        assert np.abs(ref - o).max() <= 1e-4 * np.abs(o).max()
    # dense float32 through descriptors (every descriptor the default one: what the plain call builds for itself)
    assert np.array_equal(described(gpu, stacks, psi0.copy(), views, w, lam, pad), ref)
    # dense float32 views and weights next to a strided stack: psi in a window
    assert np.array_equal(described(gpu, stacks, window(psi0)[1], views, w, lam, pad), ref)
    # windows of larger arrays, constant weights as a broadcast scalar, psi into a window
    consts = [np.broadcast_to(np.float32(1.0 / V), SHAPE) for _ in range(V)]
    assert all(np.array_equal(c, x) for c, x in zip(consts, w))
    big, psi = window(psi0)
    frame = big.copy()
    described(gpu, stacks, psi, [window(v)[1] for v in views], consts, lam, pad)
    assert np.array_equal(psi, ref)
    inside = np.zeros(big.shape, bool)
    inside[3:3 + SHAPE[0], 5:5 + SHAPE[1], 7:7 + SHAPE[2]] = True
    assert np.array_equal(big[~inside], frame[~inside])
    # uint16 images, dense and as unaligned windows
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    assert all(0 < int(u.min()) and int(u.max()) < 65535 for u in u16)
    ref16 = plain(gpu, stacks, lam, pad, views=[u.astype(np.float32) for u in u16])
    assert np.array_equal(described(gpu, stacks, psi0.copy(), u16, w, lam, pad), ref16)
    wins = [window(u, off=(1, 2, 3), fill=9)[1] for u in u16]
    assert np.array_equal(described(gpu, stacks, psi0.copy(), wins, consts, lam, pad), ref16)


@pytest.mark.parametrize("pad", ["none", "zero"])
def test_streamed_uint16_views_stream_uint16(gpu, stacks, pad):
    views, _, _, w, psi0 = stacks
    u16 = [np.rint(v).astype(np.uint16) for v in views]
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        ref = described(gpu, stacks, psi0.copy(), u16, w, 0.006, pad)
        for n in (V, 2):
            gpu.set_memory_mode("stream:%d" % n)
            before = gpu.stream_counters()
            got = described(gpu, stacks, psi0.copy(), u16, w, 0.006, pad)
            d = [b - a for a, b in zip(before, gpu.stream_counters())]
            assert np.array_equal(got, ref), n
            assert d == [1, n * ITERS, n * ITERS * (u16[0].nbytes + w[0].nbytes)], (n, d)
    finally:
        gpu.set_memory_mode(None)
        gpu.check(gpu.l.mvn_release_cached_engines())


def test_fused_middle_pass_on_described_stacks(gpu):
    # 13-plane PSFs: the form rule takes the fused middle pass where the volume has three PSF depths of planes
    # (FormRule::lines_worth, 40 >= 3 x 13), so the product's own decision is what runs here - no switch is set
    shape, nv, iters = (40, 512, 512), 2, 2
    _, views, k1, k2, w, psi0 = realistic_views(shape, nv, (13, 7, 5), seed=61)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    st = (views, k1, k2, w, psi0)
    gpu.check(gpu.l.mvn_release_cached_engines())
    try:
        h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, iters)
        c0 = gpu.l.mvn_mid_fused_launch_count()
        ref = gpu.gpu_deconvolve(psi0, h, pad_mode="none")
        assert gpu.l.mvn_mid_fused_launch_count() - c0 == iters * nv * 2, "the plain call did not take the pass either"
        u16 = [np.rint(v).astype(np.uint16) for v in views]
        ref16 = gpu.gpu_deconvolve(psi0, WorkspaceHolder([u.astype(np.float32) for u in u16], k1, k2, w, 0.006, 1e-4, iters),
                                   pad_mode="none")
        c0 = gpu.l.mvn_mid_fused_launch_count()
        got = described(gpu, st, window(psi0)[1], [window(v)[1] for v in views], w, 0.006, "none", iters=iters)
        assert gpu.l.mvn_mid_fused_launch_count() - c0 == iters * nv * 2
        assert np.array_equal(got, ref)
        assert np.array_equal(described(gpu, st, psi0.copy(), u16, w, 0.006, "none", iters=iters), ref16)
    finally:
        gpu.check(gpu.l.mvn_release_cached_engines())


def _desc(dtype=0, location=MVN_HOST, stride=None):
    d = StackDesc()
    d.dtype, d.location = dtype, location
    for k, s in enumerate(stride or (SHAPE[1] * SHAPE[2], SHAPE[2], 1)):
        d.stride[k] = s
    return d


def test_errors_leave_psi_untouched(gpu, stacks):
    views, k1, k2, w, psi0 = stacks
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, ITERS)
    dense = (SHAPE[1] * SHAPE[2], SHAPE[2], 1)
    bad = {
        "uint16 weights": dict(weights=[_desc(dtype=1)] * V),
        "psi with a zero stride": dict(psi=_desc(stride=(dense[0], 0, 1))),
        "negative stride": dict(image=[_desc(stride=(dense[0], -dense[1], 1))] * V),
        "dtype 7": dict(image=[_desc(dtype=7)] * V),
        "host stack with stride[2] != 1": dict(image=[_desc(stride=(dense[0] * 2, dense[1] * 2, 2))] * V),
        # a host pointer said to be device memory: refused by the pointer attribute query, never read
        "host pointer as device memory": dict(image=[_desc(location=MVN_DEVICE)] * V),
        "host psi as device memory": dict(psi=_desc(location=MVN_DEVICE)),
    }
    gpu.set_pad_mode("none")
    try:
        for what, kw in bad.items():
            call = CallDesc()
            call.psi = kw.get("psi", _desc())
            keep = []
            for name in ("image", "weights"):
                if name in kw:
                    keep.append((StackDesc * V)(*kw[name]))
                    setattr(call, name, C.cast(keep[-1], C.POINTER(StackDesc)))
            psi = psi0.copy()
            rc = gpu.l.mvn_deconvolve_described(C.c_void_p(psi.ctypes.data), h.ws, C.byref(call), 0)
            assert rc < 0, what
            assert gpu.l.mvn_last_error().decode().startswith("mvn_deconvolve_described"), what
            assert np.array_equal(psi, psi0), what
    finally:
        gpu.set_pad_mode(None)


# ---- the blocking branch of the ABI call (MVN_NO_PIPELINE, read once per process: a child) ---------------------------
_BLOCKING_CHILD = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import test_gpu_described_stacks as t
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
stacks = t.make_stacks()
for pad in t.BLOCKING_PADS:
    plain, desc = t.blocking_calls(gpu, stacks, pad)
    np.save(os.path.join(out, "plain_%s.npy" % pad), plain)
    np.save(os.path.join(out, "described_%s.npy" % pad), desc)
print("blocking child ok", flush=True)
"""

BLOCKING_PADS = ("none", "zero")


def blocking_calls(b, stacks, pad):
    """one plain call, and one described call with uint16 images in unaligned windows and psi in a window"""
    views, _, _, w, psi0 = stacks
    u16 = [window(np.rint(v).astype(np.uint16), off=(1, 2, 3), fill=9)[1] for v in views]
    return plain(b, stacks, 0.006, pad), described(b, stacks, window(psi0)[1], u16, w, 0.006, pad).copy()


def test_blocking_call_gives_what_the_pipelined_call_gives(gpu, stacks, tmp_path):
    # the library against itself on another code path, bit for bit (the anchor outside it: the oracle comparison of
    # test_host_stacks_dense_uint16_strided).  The module's own library handle stays idle while the child works.
    # Time limit: loading the library into a new process and creating its plans takes seconds, the calls less.
    r = subprocess.run([sys.executable, "-c", _BLOCKING_CHILD, ROOT, str(tmp_path)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, MVN_NO_PIPELINE="1", MVN_TRACE="1"))
    assert r.returncode == 0 and "blocking child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    # the child took the blocking branch: its calls were traced, and none of them started the uploader thread
    assert "[lmvn::inplace_gpu_deconvolve]" in r.stdout and "(uploader thread)" not in r.stdout, r.stdout[-4000:]
    for pad in BLOCKING_PADS:
        ref, ref16 = blocking_calls(gpu, stacks, pad)
        assert not np.array_equal(ref16, ref)
        assert np.array_equal(np.load(str(tmp_path / ("plain_%s.npy" % pad))), ref), pad
        assert np.array_equal(np.load(str(tmp_path / ("described_%s.npy" % pad))), ref16), pad


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder, MVN_DEVICE, MVN_HOST
from ref_fixtures import realistic_views
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
dev = torch.device("cuda:0")
shape, V, iters = (64, 64, 128), 4, 3
_, views, k1, k2, w, psi0 = realistic_views(shape, V, (7, 5, 5), seed=71)
u16 = [np.rint(v).astype(np.uint16) for v in views]
have_u16 = hasattr(torch, "uint16")
print("torch.uint16:", have_u16)
as16 = dict(int16_is_uint16=not have_u16)

def pin(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()

# sources in pinned host memory: copies from them with non_blocking=True are only enqueued
P_views, P_w, P_psi = [pin(v) for v in views], [pin(x) for x in w], pin(psi0)
P_u16 = [pin(u if have_u16 else u.view(np.int16)) for u in u16]  # torch.uint16, else int16 holding the same bits
P_scalar = torch.tensor(1.0 / V, dtype=torch.float32).pin_memory()
Z32, Z16 = pin(np.zeros(shape, np.float32)), pin(np.zeros(shape, np.uint16 if have_u16 else np.int16))
# the device tensors the library is handed, allocated once
D_views, D_w, D_psi = [torch.empty(shape, device=dev) for _ in range(V)], [torch.empty(shape, device=dev) for _ in range(V)], torch.empty(shape, device=dev)
D_u16 = [torch.empty(shape, dtype=P_u16[0].dtype, device=dev) for _ in range(V)]
D_perm = torch.empty(shape[::-1], device=dev)
D_scalar = torch.empty((), device=dev)
big = torch.empty((shape[0] + 7, shape[1] + 11, shape[2] + 15), device=dev)
win = big[3:3 + shape[0], 5:5 + shape[1], 7:7 + shape[2]]
junk = torch.empty(1 << 28, device=dev)
side = torch.cuda.Stream(device=dev)

def stale():
    # what a library that did not wait for the side stream would read: zeros everywhere, and the device idle
    for t in D_views + D_w + [D_psi]:
        t.copy_(Z32)
    for t in D_u16:
        t.copy_(Z16)
    D_perm.zero_(); D_scalar.zero_(); big.zero_()
    torch.cuda.synchronize()

def produce():
    # current stream = side.  Nothing here makes the host wait: a queue of fills first, then copies out of pinned
    # memory and device-side ops behind it.  The inputs are right only once the side stream has run this far.
    for _ in range(80):
        junk.fill_(1.0)
    for d, p in zip(D_views + D_w + D_u16 + [D_psi, D_scalar], P_views + P_w + P_u16 + [P_psi, P_scalar]):
        d.copy_(p, non_blocking=True)
    D_perm.copy_(D_views[1].permute(2, 1, 0))
    big.fill_(-7.0)
    win.copy_(D_psi)

def call(psi, images, weights, **kw):
    pending = not side.query()  # asked right before the call, without waiting: the production is still in flight
    gpu.deconvolve_described(psi, images, weights, k1, k2, 0.006, 1e-4, iters, **kw)
    return pending

def relabeled(c, locations):
    for key, loc in locations.items():
        if key == "psi":
            c.desc.psi.location = loc
        else:
            getattr(c, key[0])[key[1]].location = loc
    return c

pendings = []
for pad in ("none", "zero"):
    gpu.set_pad_mode(pad)
    ref = gpu.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, iters), pad_mode=False)
    ref16 = gpu.gpu_deconvolve(psi0, WorkspaceHolder([u.astype(np.float32) for u in u16], k1, k2, w, 0.006, 1e-4, iters),
                               pad_mode=False)
    assert not np.array_equal(ref, psi0)
    with torch.cuda.stream(side):
        # dense float32
        stale(); produce()
        pendings.append(call(D_psi, D_views, D_w))
        assert torch.equal(D_psi.cpu(), torch.from_numpy(ref)), ("dense", pad)
        # uint16 images
        stale(); produce()
        pendings.append(call(D_psi, D_u16, D_w, **as16))
        assert torch.equal(D_psi.cpu(), torch.from_numpy(ref16)), ("uint16", pad)
        # a permuted tensor, an expanded scalar weight, psi as a window of a larger tensor, one view left on the host
        stale(); produce()
        mixed = list(D_views)
        mixed[1] = D_perm.permute(2, 1, 0)
        assert mixed[1].stride(2) != 1
        mixed[2] = views[2]
        tconst = [D_scalar.expand(shape) for _ in range(V)]
        tconst[2] = w[2]
        assert tconst[0].stride() == (0, 0, 0)
        pendings.append(call(win, mixed, tconst))
        assert torch.equal(win.cpu(), torch.from_numpy(ref)), ("strided", pad)
        inside = torch.zeros(big.shape, dtype=torch.bool, device=dev)
        inside[3:3 + shape[0], 5:5 + shape[1], 7:7 + shape[2]] = True
        assert bool((big[~inside] == -7.0).all()), "the call wrote outside psi's window"
        # a device pointer described as host memory, a host pointer described as device memory: refused by the pointer
        # attribute query, psi untouched
        torch.cuda.synchronize()
        for loc, stacks, text in (({("image", 0): MVN_HOST}, D_views, "described as host memory"),
                                  ({("image", 0): MVN_DEVICE}, views, "described as device memory"),
                                  ({"psi": MVN_HOST}, D_views, "described as host memory")):
            D_psi.copy_(P_psi)
            try:
                relabeled(gpu.describe_call(D_psi, stacks, D_w, k1, k2, 0.006, 1e-4, iters), loc).run()
                raise SystemExit("not refused: %r" % (loc,))
            except native.MvnError as e:
                assert text in str(e), e
            assert torch.equal(D_psi.cpu(), P_psi), loc
gpu.set_pad_mode(None)
# the resident engine takes the same objects, ordered behind the side stream in the same way
a, b = gpu.engine(shape, V), gpu.engine(shape, V)
for v in range(V):
    a.set_view(v, u16[v].astype(np.float32) if v % 2 else views[v], w[v], k1[v], k2[v])
a.set_psi(psi0)
a.iterate(iters, 0.006, 1e-4)
with torch.cuda.stream(side):
    stale(); produce()
    pendings.append(not side.query())
    for v in range(V):
        b.set_view(v, D_u16[v] if v % 2 and have_u16 else (D_views[v] if not v % 2 else u16[v]), D_scalar.expand(shape),
                   k1[v], k2[v])
    b.set_psi(win)
    b.iterate(iters, 0.006, 1e-4)
    out = torch.empty(shape, device=dev)
    b.get_psi(out)
    assert torch.equal(out.cpu(), torch.from_numpy(a.get_psi()))
a.close(); b.close()
torch.cuda.synchronize()
# the ordering was exercised: the side stream still had work queued when the library was entered
print("side stream pending at the calls:", pendings)
assert all(pendings), pendings
print("ok")
"""


def test_cuda_tensors_in_a_child_process(gpu):
    # (the module's own library handle stays idle meanwhile: one GPU process works at a time)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ))
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])
