"""Padding policy "reflect" (csrc/mvn_reflect.hpp): what the tests on the emulation (test_emu_reflect.py) and on the
device (test_gpu_reflect.py) share - the index rule restated with np.take, the extents a padded call picks, the stacks
of the cases, and the checks themselves, written once against a Binding.

    f(i, n):  m = i mod 2n (non-negative);  f = m < n ? m : 2n - 1 - m

Volume voxel (z, y, x) holds the stack's voxel (f(z - o0, n0), f(y - o1, n1), f(x - o2, n2)).
"""
import numpy as np

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import expected_good_extent, gaussian_psf

F = np.float32
MINV = 1e-4


# ---- the index rule -------------------------------------------------------------------------------------------------
def mirror_index(ext, n, off):
    """for every index of an axis of extent `ext`: the index of the stack (extent n, window at `off`) it holds"""
    m = np.mod(np.arange(ext) - off, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def mirror_pad(a, ext, off):
    """the stack `a` embedded at `off` in a volume of extents `ext`, the margins its mirror image"""
    for d in range(3):
        a = np.take(a, mirror_index(ext[d], a.shape[d], off[d]), axis=d)
    return np.ascontiguousarray(a)


def zero_pad(a, ext, off):
    out = np.zeros(ext, a.dtype)
    out[window(a.shape, off)] = a
    return out


def window(dims, off):
    return tuple(slice(o, o + n) for o, n in zip(off, dims))


def call_extents(lib, dims, kernels):
    """(ext, off) of a "zero" / "reflect" call (mvn_abi.cpp call_extents): image + kernel - 1 grown to the FFT-friendly
    extent, the window at (kernel - 1) / 2; dim0 stays exact where the rows of a plane keep whole tiles and every PSF
    of the call is held in the direct dim0 form."""
    kmax = [max(k.shape[d] for k in kernels) for d in range(3)]
    off = [(k - 1) // 2 for k in kmax]
    ext = [dims[d] + kmax[d] - 1 for d in range(3)]
    for d in (2, 1):
        ext[d] = expected_good_extent(lib, ext[d], d == 2)
    exact = False
    if ext[1] % 16 == 0:
        e = lib.engine(tuple(ext), 1)
        try:
            exact = all(e.would_be_direct(k.shape) for k in kernels)
        finally:
            e.close()
    if not exact:
        ext[0] = expected_good_extent(lib, ext[0], False)
    return tuple(ext), tuple(off)


def row_pitch(ext):
    return ext[2] + (ext[2] & 1)


# ---- stacks ---------------------------------------------------------------------------------------------------------
# name: (stack extents, kernel1 extents, kernel2 extents)
PARITY_CASES = {
    "block": ((20, 18, 22), (5, 5, 5), (3, 3, 3)),
    "odd last extent": ((6, 10, 15), (7, 3, 5), (7, 3, 5)),           # row padding
    "margins wider than the stack": ((3, 5, 2), (9, 3, 7), (9, 3, 7)),
    "an extent of 1": ((1, 12, 16), (1, 5, 5), (1, 5, 5)),
    "an axis without a kernel": ((12, 16, 20), (3, 3, 1), (3, 3, 1)),
}


# the cases of the placement routes, and whether a row of the volume is a whole number of 16-byte groups of uint16
ROUTE_CASES = {"block": False, "odd last extent": False, "rows of 16-byte groups": True}
EXTRA_CASES = {"rows of 16-byte groups": ((5, 9, 20), (3, 3, 5), (3, 3, 5))}


def make_stacks(name, integer_views=False, seed=11):
    """strictly positive stacks of a case: views, kernels1, kernels2, weights (sum over views <= 1), psi0"""
    shape, ks1, ks2 = PARITY_CASES.get(name) or EXTRA_CASES[name]
    rng = np.random.default_rng(seed)
    views, k1, k2, w = [], [], [], []
    for v in range(2):
        if integer_views:
            views.append(rng.integers(1, 4000, shape).astype(F))
        else:
            views.append(rng.uniform(1.0, 200.0, shape).astype(F))
        sig = [1.0, 1.0, 1.0]
        sig[v % 3] = 2.0
        psf = gaussian_psf(ks1, sig)
        k1.append(psf)
        if ks2 == ks1:
            k2.append(np.ascontiguousarray(psf[::-1, ::-1, ::-1]))
        else:
            k2.append(gaussian_psf(ks2, sig))
        w.append(rng.uniform(0.1, 0.5, shape).astype(F))
    psi0 = rng.uniform(20.0, 120.0, shape).astype(F)
    return views, k1, k2, w, psi0


def reflect_call(lib, st, lam=0.006, iters=3, mode="reflect"):
    views, k1, k2, w, psi0 = st
    got = lib.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, lam, MINV, iters), pad_mode=mode)
    assert not np.array_equal(got, psi0), lib.l.mvn_last_error().decode()
    return got


def mirrored_stacks(lib, st):
    """the stacks of a case mirrored by hand into the extents the padded call picks; also (ext, window)"""
    views, k1, k2, w, psi0 = st
    ext, off = call_extents(lib, psi0.shape, k1 + k2)
    pad = lambda a: mirror_pad(a, ext, off)
    return ([pad(v) for v in views], k1, k2, [pad(x) for x in w], pad(psi0)), ext, window(psi0.shape, off)


def none_call_on_mirrored(lib, st, lam=0.006, iters=3):
    big, ext, sl = mirrored_stacks(lib, st)
    views, k1, k2, w, psi0 = big
    got = lib.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, lam, MINV, iters), pad_mode="none")
    return got[sl], ext


# ---- 1. parity ------------------------------------------------------------------------------------------------------
def check_parity(lib, orc, name):
    st = make_stacks(name)
    assert all(float(a.min()) > 0 for a in st[0] + st[3] + [st[4]])
    got = reflect_call(lib, st)
    want, ext = none_call_on_mirrored(lib, st)
    differ = int((got != want).sum())
    print("%s: volume %r, %d voxels differ from the call on hand-mirrored stacks" % (name, ext, differ))
    assert np.array_equal(got, want), (name, ext, differ)
    big, ext, sl = mirrored_stacks(lib, st)
    views, k1, k2, w, psi0 = big
    ref = orc.cpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, 0.006, MINV, 3), 4)[sl]
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("%s: max error against the oracle %.3g of the maximum" % (name, err))
    assert err <= 1e-4, (name, err)
    # and mirrored margins are not zeros: the policy is not "zero" under another name
    assert not np.array_equal(got, reflect_call(lib, st, mode="zero"))
    return ext


# ---- 2. every placement route ---------------------------------------------------------------------------------------
def in_window(a, off=(1, 2, 3), fill=9):
    """a as a window with contiguous rows of a larger array"""
    big = np.full(tuple(s + 2 * o + 1 for s, o in zip(a.shape, off)), fill, a.dtype)
    win = big[window(a.shape, off)]
    win[...] = a
    return win


def described(lib, st, views, weights, psi=None):
    _, k1, k2, _, psi0 = st
    before = lib.get_pad_mode()
    lib.set_pad_mode("reflect")
    try:
        return lib.deconvolve_described(psi0.copy() if psi is None else psi, views, weights, k1, k2, 0.006, MINV, 3)
    finally:
        lib.set_pad_mode(before)


def check_routes(lib, name):
    st = make_stacks(name, integer_views=True)
    views, k1, k2, w, psi0 = st
    ext, _ = call_extents(lib, psi0.shape, k1 + k2)
    print("%s: volume %r, row pitch %d" % (name, ext, row_pitch(ext)))
    assert (row_pitch(ext) % 8 == 0) == ROUTE_CASES[name], ext
    lib.check(lib.l.mvn_release_cached_engines())
    want = reflect_call(lib, st)
    u16 = [v.astype(np.uint16) for v in views]
    assert all(np.array_equal(u.astype(F), v) for u, v in zip(u16, views))
    try:
        for mode in (0, 1):  # uint16 images in host memory, converted on entry / kept as uint16
            lib.set_image_storage(mode)
            before = lib.image_storage_counters()
            assert np.array_equal(described(lib, st, u16, w), want), ("uint16, storage mode", mode)
            assert np.array_equal(described(lib, st, [in_window(u) for u in u16], w), want), ("uint16 windows", mode)
            assert (lib.image_storage_counters()[1] > before[1]) == (mode == 1)
    finally:
        lib.set_image_storage(0)
    # strided host stacks: views, weights and psi as windows of larger arrays
    psi = in_window(psi0, off=(2, 1, 2), fill=-7.0)
    described(lib, st, [in_window(v, fill=-3.0) for v in views], [in_window(x, fill=0.25) for x in w], psi=psi)
    assert np.array_equal(psi, want)
    # {0, 0, 0} weights: that value everywhere, margins included
    consts = [np.broadcast_to(F(0.5), psi0.shape) for _ in views]
    st_c = (views, k1, k2, [np.ascontiguousarray(c) for c in consts], psi0)
    want_c = reflect_call(lib, st_c)
    assert not np.array_equal(want_c, want)
    assert np.array_equal(described(lib, st, views, consts), want_c)
    # submit / wait: the policy in force at submit
    out = psi0.copy()
    h = WorkspaceHolder(views, k1, k2, w, 0.006, MINV, 3)
    before = lib.get_pad_mode()
    lib.set_pad_mode("reflect")
    try:
        t = lib.deconvolve_submit(out, h)
    finally:
        lib.set_pad_mode(before)
    lib.deconvolve_wait(t)
    assert np.array_equal(out, want)
    # streamed views: one, and all of them - the fill follows every upload into a ring slot
    try:
        for mem, n in (("stream:1", 1), ("stream", 2)):
            lib.set_memory_mode(mem)
            before = lib.stream_counters()
            got = reflect_call(lib, st)
            d = [b - a for a, b in zip(before, lib.stream_counters())]
            assert d[0] == 1 and d[1] == n * 3, (mem, d)
            assert np.array_equal(got, want), mem
            lib.set_image_storage(1)
            assert np.array_equal(described(lib, st, u16, w), want), (mem, "uint16 kept")
            lib.set_image_storage(0)
    finally:
        lib.set_image_storage(0)
        lib.set_memory_mode(None)
        lib.check(lib.l.mvn_release_cached_engines())
    return want


# ---- 3. cached engines ----------------------------------------------------------------------------------------------
def check_cached_engines(lib, mem):
    st = make_stacks("block", seed=13)
    lib.check(lib.l.mvn_release_cached_engines())
    lib.set_memory_mode(mem)
    try:
        got = [reflect_call(lib, st, mode=m) for m in ("zero", "reflect", "zero", "reflect")]
        for i, m in ((0, "zero"), (1, "reflect")):
            lib.check(lib.l.mvn_release_cached_engines())
            fresh = reflect_call(lib, st, mode=m)
            assert np.array_equal(got[i], got[i + 2]), (m, "first against second")
            assert np.array_equal(got[i], fresh), (m, "first against a fresh engine")
            assert np.array_equal(got[i + 2], fresh), (m, "second against a fresh engine")
        assert not np.array_equal(got[0], got[1])
    finally:
        lib.set_memory_mode(None)
        lib.check(lib.l.mvn_release_cached_engines())


# ---- 4. composition -------------------------------------------------------------------------------------------------
def check_composition(lib):
    st = make_stacks("odd last extent", seed=17)
    views, k1, k2, w, psi0 = st
    one = (views[:1], k1[:1], k2[:1], w[:1], psi0)  # (one view: P_k of the last sweep is the sum of the returned psi)
    lam, iters = 0.01, 4
    lib.check(lib.l.mvn_release_cached_engines())
    lib.set_acceleration(1)
    lib.set_regularization(1, 1.0)
    lib.set_background([3.0])
    try:
        got = reflect_call(lib, st, lam=lam, iters=iters)
        want, ext = none_call_on_mirrored(lib, st, lam=lam, iters=iters)
        plain = reflect_call(lib, one, lam=lam, iters=iters)
        lib.set_convergence(0.0)
        single = reflect_call(lib, one, lam=lam, iters=iters)
        run, rows = lib.last_convergence()
    finally:
        lib.set_convergence(-1)
        lib.set_background(None)
        lib.set_regularization(0)
        lib.set_acceleration(0)
        lib.check(lib.l.mvn_release_cached_engines())
    assert np.array_equal(got, want), ext
    assert np.array_equal(single, plain)
    assert run == iters and rows.shape == (iters, 3)
    # the rows cover the window, the voxels handed back: with one view, P_k of the last sweep is the sum of the returned
    # psi.  Float-sum rounding: both sides sum the same float32 values in double, in different orders - 1e-9 of the
    # sum is generous for < 1e4 terms, and far below what the margins would add (the volume holds several times the
    # window's voxels, all of them positive)
    p_last = float(single.astype(np.float64).sum())
    off = call_extents(lib, psi0.shape, one[1] + one[2])[1]
    p_volume = float(mirror_pad(single, ext, off).astype(np.float64).sum())
    print("P_k %.12g, the sum of the returned psi %.12g, of the padded volume %.6g" % (rows[-1, 2], p_last, p_volume))
    assert p_volume > 2 * p_last
    assert abs(rows[-1, 2] - p_last) <= 1e-9 * p_last


# ---- 5. surface -----------------------------------------------------------------------------------------------------
def check_surface(lib, monkeypatch):
    before = lib.get_pad_mode()
    try:
        lib.set_pad_mode("reflect")
        assert lib.get_pad_mode() == "reflect"
        assert lib.l.mvn_set_pad_mode(b"mirror") < 0
        assert "reflect" in lib.l.mvn_last_error().decode() and "mirror" in lib.l.mvn_last_error().decode()
        assert lib.get_pad_mode() == "reflect"
    finally:
        lib.set_pad_mode(before)
    st = make_stacks("block")
    views, k1, k2, w, psi0 = st
    h = WorkspaceHolder(views, k1, k2, w, 0.006, MINV, 3)
    need = {}
    for mode in ("zero", "reflect"):
        lib.set_pad_mode(mode)
        try:
            need[mode] = [lib.deconvolve_memory(h, s) for s in (0, 1, 2)]
        finally:
            lib.set_pad_mode(before)
    assert need["zero"] == need["reflect"] and need["zero"][0] > 0
    # the counters: launches and volumes under "reflect" (psi, and image and weights of two views), none under "zero"
    lib.check(lib.l.mvn_release_cached_engines())
    c0 = lib.reflect_counters()
    reflect_call(lib, st, mode="zero")
    assert lib.reflect_counters() == c0
    want = reflect_call(lib, st)
    c1 = lib.reflect_counters()
    assert c1[1] - c0[1] == 5 and c1[0] - c0[0] == 15, (c0, c1)
    # the environment variable selects it as well
    monkeypatch.setenv("MVN_PAD_MODE", "reflect")
    assert lib.get_pad_mode() is None
    assert np.array_equal(reflect_call(lib, st, mode=False), want)
    monkeypatch.delenv("MVN_PAD_MODE")
    # MVN_DEVICES: a reflect call stays on one device (the slabs need the direct dim0 leg: the pins go)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    lib.check(lib.l.mvn_release_cached_engines())
    st = make_stacks("an axis without a kernel")
    one = reflect_call(lib, st)
    monkeypatch.setenv("MVN_DEVICES", "0,0")
    try:
        calls = lib.l.mvn_multi_device_calls()
        two = reflect_call(lib, st)
        assert lib.l.mvn_multi_device_calls() == calls
        assert np.array_equal(one, two)
        reflect_call(lib, st, mode="zero")
        assert lib.l.mvn_multi_device_calls() == calls + 1  # (the same call under "zero" does go to the slabs)
    finally:
        monkeypatch.delenv("MVN_DEVICES")
        lib.check(lib.l.mvn_release_cached_engines())


# ---- 6. the point of it ---------------------------------------------------------------------------------------------
def border_problem(seed=5, big=(44, 48, 52), shape=(24, 28, 32), kshape=(7, 7, 7), n_blobs=60):
    """The window of a larger specimen: truth is blobs on a background of 10 in `big`, two views are truth convolved
    LINEARLY (not cyclically) with realistic_views' Gaussians, the central `shape` window of each is what the loop gets.
    Returns the truth in the window and the stacks (views, kernels1, kernels2, weights, psi0)."""
    rng = np.random.default_rng(seed)
    o = tuple((b - s) // 2 for b, s in zip(big, shape))
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in big], indexing="ij")
    truth = np.full(big, 10.0)
    for _ in range(n_blobs):
        c = [rng.uniform(0, s) for s in big]
        sg = rng.uniform(1.0, 3.0)
        amp = rng.uniform(50, 500)
        truth += amp * np.exp(-((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) / (2 * sg * sg))
    win = window(shape, o)
    full = tuple(b + k - 1 for b, k in zip(big, kshape))
    same = tuple(slice((k - 1) // 2, (k - 1) // 2 + b) for b, k in zip(big, kshape))
    ft = np.fft.rfftn(truth, full, axes=(0, 1, 2))
    views, k1, k2, w = [], [], [], []
    for v in range(2):
        sig = [1.0, 1.0, 1.0]
        sig[v % 3] = 2.0
        psf = gaussian_psf(kshape, sig)
        blurred = np.fft.irfftn(ft * np.fft.rfftn(psf.astype(np.float64), full, axes=(0, 1, 2)), full, axes=(0, 1, 2))[same]  # zeros beyond `big`
        views.append(np.ascontiguousarray(blurred[win]).astype(F))
        k1.append(psf)
        k2.append(np.ascontiguousarray(psf[::-1, ::-1, ::-1]))
        w.append(np.full(shape, 0.5, F))
    psi0 = np.full(shape, F(np.mean(views)), F)
    return truth[win], (views, k1, k2, w, psi0)


def band_rms(a, truth, width=3):
    band = np.ones(truth.shape, bool)
    band[width:-width, width:-width, width:-width] = False
    return float(np.sqrt(np.mean((a[band].astype(np.float64) - truth[band]) ** 2)))


def check_border_quality(lib):
    truth, st = border_problem()
    lib.check(lib.l.mvn_release_cached_engines())
    try:
        err = {m: band_rms(reflect_call(lib, st, lam=0.0, iters=20, mode=m), truth) for m in ("zero", "reflect")}
    finally:
        lib.check(lib.l.mvn_release_cached_engines())
    blurred = band_rms(st[0][0], truth)
    print("RMS error in the border band after 20 sweeps: zero %.2f, reflect %.2f; the blurred view itself %.2f" % (
        err["zero"], err["reflect"], blurred))
    assert err["reflect"] < 0.5 * err["zero"], err
    assert err["reflect"] < blurred, (err, blurred)
