"""Resampled views (csrc/mvn_resample.hpp, mvn_view_geometry in include/mvn_engine_api.h): what the tests on the
emulation (test_emu_resample.py) and on the device (test_gpu_resample.py) share - a numpy restatement of the
definition, the cases, and the checks themselves, written once against a Binding.

For block voxel (z, y, x):   c_k = ((M[k][0] z + M[k][1] y) + M[k][2] x) + M[k][3]   in double,
inside iff 0 <= c_k <= m_k - 1;  i_k = floor(c_k), f_k = float32(c_k - i_k), j_k = min(i_k + 1, m_k - 1);
trilinear in float32 along raw axis 2, 1, 0 with lerp(p, q, f) = p + f * (q - p);  the blend weight is the product
(r_0 r_1) r_2 of cosine ramps of the distance to the nearer face.  numpy rounds every float32 / float64 array operation
once and contracts nothing, which is what the definition asks for.
"""
import ctypes as C
import math

import numpy as np

from libmultiviewnative_amd.abi import (MVN_DEVICE, MVN_F32, MVN_U16, StackDesc, WorkspaceHolder, fptr, view_geometry)
from ref_fixtures import gaussian_psf

F = np.float32
MINV = 1e-4
TILE = (8, 8, 64)  # MVN_RS_TZ, MVN_RS_TY, MVN_RS_TX of csrc/mvn_resample.hpp


# ---- the definition -------------------------------------------------------------------------------------------------
def coordinates(M, out_shape):
    M = np.asarray(M, np.float64).reshape(3, 4)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing="ij")
    return [((M[k, 0] * z + M[k, 1] * y) + M[k, 2] * x) + M[k, 3] for k in range(3)]


def inside_mask(c, m):
    ok = np.ones(c[0].shape, bool)
    for k in range(3):
        ok &= (c[k] >= 0.0) & (c[k] <= float(m[k] - 1))
    return ok


def ramps(c, m, border, rng, inside, dtype=np.float32):
    """per axis (r_k, zero mask, one mask) with the formula evaluated in `dtype`"""
    out = []
    for k in range(3):
        ck = np.where(inside, c[k], 0.0)
        d = np.minimum(ck, float(m[k] - 1) - ck)
        dk = d.astype(np.float32).astype(dtype)
        b, w = dtype(F(border[k])), dtype(F(rng[k]))  # (border, range and pi_f are float32 values in either evaluation)
        zero = dk < b
        one = ~zero & ((w == 0) | (dk >= b + w))
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (dk - b) / w
            r = dtype(0.5) * (dtype(1.0) - np.cos(dtype(F(3.14159265358979323846)) * u))
        r = np.where(zero, dtype(0), np.where(one, dtype(1), r)).astype(dtype)
        out.append((r, zero, one))
    return out


def resample_numpy(raw, M, out_shape, border=(0, 0, 0), rng=(0, 0, 0)):
    """image, unnormalised weights (float32 formula), and the masks where the weight must be exactly 0 / exactly 1"""
    m = raw.shape
    c = coordinates(M, out_shape)
    inside = inside_mask(c, m)
    S = np.asarray(raw).astype(F)
    i, j, f = [], [], []
    for k in range(3):
        ck = np.where(inside, c[k], 0.0)
        ik = np.floor(ck)
        f.append((ck - ik).astype(F))
        ik = ik.astype(np.int64)
        i.append(ik)
        j.append(np.minimum(ik + 1, m[k] - 1))
    lerp = lambda p, q, t: p + t * (q - p)
    b = []
    for p in (i[0], j[0]):
        a = [lerp(S[p, q, i[2]], S[p, q, j[2]], f[2]) for q in (i[1], j[1])]
        b.append(lerp(a[0], a[1], f[1]))
    image = np.where(inside, lerp(b[0], b[1], f[0]), F(0)).astype(F)
    r = ramps(c, m, border, rng, inside)
    w = ((r[0][0] * r[1][0]) * r[2][0]).astype(F)
    w = np.where(inside, w, F(0)).astype(F)
    zero = ~inside | r[0][1] | r[1][1] | r[2][1]
    one = inside & r[0][2] & r[1][2] & r[2][2]
    return image, w, zero, one


def weights_float64(raw_shape, M, out_shape, border, rng):
    """the same definition with the ramp formula in float64"""
    c = coordinates(M, out_shape)
    inside = inside_mask(c, raw_shape)
    r = ramps(c, raw_shape, border, rng, inside, np.float64)
    return np.where(inside, (r[0][0] * r[1][0]) * r[2][0], 0.0)


def normalize_numpy(ws):
    """W = ((w_0 + w_1) + ...) in view order, w_v <- W > 0 ? w_v / W : 0, in float32"""
    W = ws[0].copy()
    for w in ws[1:]:
        W = W + w
    with np.errstate(divide="ignore", invalid="ignore"):
        return [np.where(W > 0, w / W, F(0)).astype(F) for w in ws]


# ---- the cases ------------------------------------------------------------------------------------------------------
_C30, _S30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
# name: (block extents, raw extents, matrix (3 x 4), blend border, blend range)
CASES = {
    # (3, 5, 7): odd last extent, row pitch 2 mod 4; c_2 reaches m_2 - 1 = 6 exactly
    "identity": ((3, 5, 7), (5, 6, 7), [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], (0, 1, 0.5), (1, 2, 1.5)),
    # plane z = 0 lies outside the raw stack; c_2 reaches m_2 - 1 = 10 exactly
    "integer shift": ((4, 6, 10), (3, 9, 11), [[1, 0, 0, -1], [0, 1, 0, 2], [0, 0, 1, 1]], (0, 0, 1), (1, 3, 0)),
    # (2, 3, 20): row pitch a multiple of 4; half of every row lies outside
    "fractional shift": ((2, 3, 20), (3, 9, 11), [[1, 0, 0, 0.25], [0, 1, 0, 1.5], [0, 0, 1, -2.6]],
                         (0, 0.5, 0), (0.75, 2, 3)),
    # a raw z-step of 3 block voxels; the block is larger than the kernel's tile on every axis by a non-multiple
    "anisotropic scale": ((10, 14, 70), (5, 6, 7), [[1 / 3, 0, 0, 0], [0, 0.35, 0, 0], [0, 0, 0.08, 0]],
                          (0.5, 0, 0.25), (1, 1.5, 2)),
    # 90 degrees about axis 1 with that scale: raw axis 0 follows the block's x, raw axis 2 runs against its z
    "rotation by 90 degrees with scale": ((4, 6, 10), (5, 6, 7), [[0, 0, 1 / 3, 0], [0, 1, 0, 0], [-1.5, 0, 0, 6]],
                                          (0, 0, 0), (1.25, 1, 2)),
    "rotation by 30 degrees": ((3, 5, 7), (5, 6, 7),
                               [[_C30, 0, _S30, 2 - _C30 * 1 - _S30 * 3], [0, 1, 0, 0.5],
                                [-_S30, 0, _C30, 3 + _S30 * 1 - _C30 * 3]], (0, 0.25, 0), (1, 1, 1.5)),
    "rotation by 30 degrees across tiles": ((10, 14, 70), (5, 6, 7),
                                            [[0.3 * _C30, 0, 0.05 * _S30, 2 - 0.3 * _C30 * 4.5 - 0.05 * _S30 * 34.5],
                                             [0, 0.38, 0, 0],
                                             [-0.3 * _S30, 0, 0.05 * _C30, 3 + 0.3 * _S30 * 4.5 - 0.05 * _C30 * 34.5]],
                                            (0, 0, 0), (0.5, 1, 1)),
    "one raw plane": ((2, 3, 20), (1, 6, 7), [[0, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0.3, 0]], (0, 0, 0.5), (0, 1, 1)),
}
DTYPES = (np.uint16, np.float32)
LAYOUTS = ("dense", "row-strided", "broadcast")
# the views of the calls: two blocks, each seen by two raw stacks
CALL_VIEWS = {
    "odd block": ("identity", "rotation by 30 degrees"),
    "even block": ("integer shift", "rotation by 90 degrees with scale"),
}
PAD_MODES = ("none", "zero", "zero_exact", "reflect")


def raw_stack(name, dtype, seed=3):
    shape = CASES[name][1]
    rng = np.random.default_rng(seed + sum(shape))
    if dtype is np.uint16:
        return rng.integers(100, 4000, shape).astype(np.uint16)
    return rng.uniform(100.0, 4000.0, shape).astype(F)


def laid_out(raw, layout):
    """the raw stack as a window with contiguous rows of a larger array, or one value for every voxel"""
    if layout == "dense":
        return raw
    if layout == "row-strided":
        big = np.full(tuple(s + 3 for s in raw.shape), 7, raw.dtype)
        win = big[1:1 + raw.shape[0], 2:2 + raw.shape[1], 1:1 + raw.shape[2]]
        win[...] = raw
        return win
    return np.broadcast_to(raw.dtype.type(raw[0, 0, 0]), raw.shape)


def geometry(name):
    block, raw, M, border, rng = CASES[name]
    return view_geometry(raw, M, border, rng)


def _check_case_table():
    outside = on_face = False
    for name, (block, raw, M, border, rng) in CASES.items():
        c = coordinates(M, block)
        inside = inside_mask(c, raw)
        share = float(inside.mean())
        assert share >= 0.4, (name, share)
        outside = outside or not inside.all()
        on_face = on_face or any(bool((c[k][inside] == raw[k] - 1).any()) for k in range(3) if raw[k] > 1)
    assert outside and on_face
    assert any(CASES[n][1][0] == 1 for n in CASES)
    big = CASES["anisotropic scale"][0]
    assert all(b > t and b % t for b, t in zip(big, TILE)), (big, TILE)  # tile seams on all three axes
    for names in CALL_VIEWS.values():
        assert len({CASES[n][0] for n in names}) == 1


_check_case_table()

_TOL = {}


def weight_tolerance():
    """Ten times the largest deviation of the float32 formula (numpy) from a float64 evaluation of the same definition,
    over the ramp voxels of the cases: cosf of the host and device libraries differs from numpy's by a few units in the
    last place, which is what the factor is for."""
    if not _TOL:
        worst = 0.0
        for name, (block, raw, M, border, rng) in CASES.items():
            _, w32, _, _ = resample_numpy(np.zeros(raw, F), M, block, border, rng)
            w64 = weights_float64(raw, M, block, border, rng)
            worst = max(worst, float(np.abs(w32.astype(np.float64) - w64).max()))
        assert worst > 0
        _TOL["measured"], _TOL["allowed"] = worst, 10 * worst
    return _TOL["allowed"]


# ---- 1. the pass alone: mvn_resample_stack ---------------------------------------------------------------------------
def resample_direct(lib, arr, geom, out_shape, location=None):
    """mvn_resample_stack through ctypes, the descriptor made by hand (location: what it claims)"""
    d = StackDesc()
    d.dtype = MVN_U16 if arr.dtype == np.uint16 else MVN_F32
    d.location = 0 if location is None else location
    for k in range(3):
        d.stride[k] = arr.strides[k] // arr.itemsize
    image, weights = np.full(out_shape, -1, F), np.full(out_shape, -1, F)
    lib.check(lib.l.mvn_resample_stack(0, C.c_void_p(arr.ctypes.data), C.byref(d), C.byref(geom),
                                       (C.c_int * 3)(*out_shape), fptr(image), fptr(weights)))
    return image, weights


def check_weights(name, got, want, zero, one):
    tol = weight_tolerance()
    assert np.all(got[zero] == 0), name
    assert np.all(got[one] == 1), name
    dev = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: weights deviate from numpy's float32 by at most %.3g (allowed %.3g, measured float32 against float64 "
          "%.3g); %d ramp voxels" % (name, dev, tol, _TOL["measured"], int((~zero & ~one).sum())))
    assert dev <= tol, (name, dev, tol)
    return dev


def check_stack(lib, name, dtype, layout, resample=None):
    """the image bit for bit and the weights by their rule; `resample`: how the raw array reaches the library (default:
    Binding.resample_stack on the host array)"""
    block, raw_shape, M, border, rng = CASES[name]
    raw = laid_out(raw_stack(name, dtype), layout)
    want_i, want_w, zero, one = resample_numpy(np.ascontiguousarray(raw), M, block, border, rng)
    got_i, got_w = (resample or (lambda a, g, s: lib.resample_stack(a, g, s)))(raw, geometry(name), block)
    differ = int((got_i != want_i).sum())
    assert got_i.dtype == F and np.array_equal(got_i, want_i), (name, dtype, layout, differ)
    assert not zero.all() and float(got_i.max()) > 0
    return check_weights(name, got_w, want_w, zero, one)


# ---- 2. the call -----------------------------------------------------------------------------------------------------
def make_call(key, seed=21, dtypes=(np.uint16, np.float32)):
    """raw stacks and geometries of two views, kernels, caller's weights and psi0 of a block"""
    names = CALL_VIEWS[key]
    block = CASES[names[0]][0]
    rng = np.random.default_rng(seed)
    raws = [raw_stack(n, dt, seed) for n, dt in zip(names, dtypes)]
    geoms = [geometry(n) for n in names]
    k1, k2 = [], []
    for v in range(len(names)):
        sig = [1.0, 1.0, 1.0]
        sig[v % 3] = 2.0
        psf = gaussian_psf((3, 3, 3), sig)
        k1.append(psf)
        k2.append(np.ascontiguousarray(psf[::-1, ::-1, ::-1]))
    w = [rng.uniform(0.1, 0.5, block).astype(F) for _ in names]
    psi0 = rng.uniform(200.0, 1200.0, block).astype(F)
    return dict(names=names, block=block, raws=raws, geoms=geoms, k1=k1, k2=k2, w=w, psi0=psi0)


def with_pad_mode(lib, mode, fn):
    before = lib.get_pad_mode()
    lib.set_pad_mode(mode)
    try:
        return fn()
    finally:
        lib.set_pad_mode(before)


def plain_call(lib, c, images, weights, mode, lam=0.006, iters=3):
    h = WorkspaceHolder(images, c["k1"], c["k2"], weights, lam, MINV, iters)
    got = lib.gpu_deconvolve(c["psi0"], h, pad_mode=mode)
    assert not np.array_equal(got, c["psi0"]), lib.l.mvn_last_error().decode()
    return got


def resampled_call(lib, c, mode, weights=None, lam=0.006, iters=3, raws=None, location=None, psi=None):
    call = lib.resample_call(c["psi0"].copy() if psi is None else psi, raws or c["raws"], c["geoms"], c["k1"], c["k2"],
                             lam, MINV, iters, weights=weights)
    if location is not None:  # (the emulation: any pointer may be called device memory)
        for v in range(len(c["raws"])):
            call.image[v].location = location
    return with_pad_mode(lib, mode, call.run)


def library_stacks(lib, c):
    """what mvn_resample_stack makes of the views of a call: images and unnormalised weights"""
    out = [lib.resample_stack(r, g, c["block"]) for r, g in zip(c["raws"], c["geoms"])]
    return [o[0] for o in out], [o[1] for o in out]


def check_image_route(lib, key, mode, orc=None):
    c = make_call(key)
    images, _ = library_stacks(lib, c)
    lib.check(lib.l.mvn_release_cached_engines())
    want = plain_call(lib, c, images, c["w"], mode)
    got = resampled_call(lib, c, mode, weights=c["w"])
    assert np.array_equal(got, want), (key, mode, int((got != want).sum()))
    if orc is not None:
        views = [resample_numpy(r, CASES[n][2], c["block"])[0] for r, n in zip(c["raws"], c["names"])]
        ref = orc.cpu_deconvolve(c["psi0"], WorkspaceHolder(views, c["k1"], c["k2"], c["w"], 0.006, MINV, 3), 4)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("%s: max error against the oracle on numpy-resampled stacks %.3g of the maximum" % (key, err))
        assert err <= 1e-4, (key, err)


def check_weights_route(lib, key, mode):
    c = make_call(key)
    images, ws = library_stacks(lib, c)
    wn = normalize_numpy(ws)
    assert float(np.max(wn[0] + wn[1])) <= 1.0 + 1e-6 and float(np.max(wn[0])) > 0
    lib.check(lib.l.mvn_release_cached_engines())
    want = plain_call(lib, c, images, wn, mode)
    c0 = lib.resample_counters()
    got = resampled_call(lib, c, mode)
    c1 = lib.resample_counters()
    assert np.array_equal(got, want), (key, mode, int((got != want).sum()))
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (len(c["raws"]), 1), (c0, c1)
    # raw stacks as windows of larger arrays, and called device memory where the backend lets any pointer be
    strided = [laid_out(r, "row-strided") for r in c["raws"]]
    assert np.array_equal(resampled_call(lib, c, mode, raws=strided), want), (key, mode, "row-strided")
    return c, want


# ---- 3. block after block ---------------------------------------------------------------------------------------------
def check_block_after_block(lib, location=None, to_device=None):
    """two blocks cut from one raw stack per view: the same pointers, only the matrix offset changes; a cached engine"""
    key = "even block"
    c = make_call(key)
    raws = [to_device(r) for r in c["raws"]] if to_device else c["raws"]
    lib.check(lib.l.mvn_release_cached_engines())
    results = []
    for shift in ((0, 0, 0), (1, 2, 3)):
        geoms = []
        for n in c["names"]:
            block, raw, M, border, rng = CASES[n]
            M = np.asarray(M, np.float64).copy()
            M[:, 3] = M[:, 3] + M[:, :3] @ np.asarray(shift, np.float64)  # block voxel (z, y, x) + shift
            geoms.append(view_geometry(raw, M, border, rng))
        cb = dict(c, geoms=geoms)
        got = resampled_call(lib, cb, "zero", raws=raws, location=location)
        images, ws = library_stacks(lib, cb)
        want = plain_call(lib, cb, images, normalize_numpy(ws), "zero")
        assert np.array_equal(got, want), shift
        results.append(got)
    assert not np.array_equal(results[0], results[1])
    lib.check(lib.l.mvn_release_cached_engines())


# ---- 4. composition ---------------------------------------------------------------------------------------------------
def check_composition(lib):
    c = make_call("odd block", seed=17)
    images, ws = library_stacks(lib, c)
    wn = normalize_numpy(ws)
    lam, iters = 0.01, 4
    lib.check(lib.l.mvn_release_cached_engines())
    lib.set_acceleration(1)
    lib.set_regularization(1, 1.0)
    lib.set_background([3.0, 2.0])
    lib.set_convergence(0.0)
    try:
        want = plain_call(lib, c, images, wn, "zero", lam=lam, iters=iters)
        run_w, rows_w = lib.last_convergence()
        got = resampled_call(lib, c, "zero", lam=lam, iters=iters)
        run_g, rows_g = lib.last_convergence()
    finally:
        lib.set_convergence(-1)
        lib.set_background(None)
        lib.set_regularization(0)
        lib.set_acceleration(0)
        lib.check(lib.l.mvn_release_cached_engines())
    assert np.array_equal(got, want)
    assert run_g == run_w == iters and np.array_equal(rows_g, rows_w)
    assert not np.array_equal(got, plain_call(lib, c, images, wn, "zero", lam=lam, iters=iters))  # the switches act


# ---- 5. surface -------------------------------------------------------------------------------------------------------
def check_errors_leave_psi_untouched(lib):
    c = make_call("even block")
    good = CASES[c["names"][0]]

    def bad_geometry(**kw):
        block, raw, M, border, rng = good
        M = np.asarray(M, np.float64).copy()
        if "matrix" in kw:
            M[1, 2] = kw["matrix"]
        g = view_geometry(kw.get("src", raw), M, kw.get("border", border), kw.get("range", rng))
        return g

    cases = {
        "a NaN matrix entry": bad_geometry(matrix=float("nan")),
        "an infinite matrix entry": bad_geometry(matrix=float("inf")),
        "a negative border": bad_geometry(border=(0, -1, 0)),
        "a NaN border": bad_geometry(border=(float("nan"), 0, 0)),
        "a negative range": bad_geometry(range=(0, 0, -0.5)),
        "an infinite range": bad_geometry(range=(float("inf"), 0, 0)),
    }
    for what, g in cases.items():
        psi = c["psi0"].copy()
        call = lib.resample_call(psi, c["raws"], [g, c["geoms"][1]], c["k1"], c["k2"], 0.006, MINV, 3)
        rc = lib.l.mvn_deconvolve_resampled(C.c_void_p(call.psi_ptr), call.ws, C.byref(call.desc), call.geom, 1, 0)
        assert rc < 0 and lib.l.mvn_last_error().decode(), what
        assert np.array_equal(psi, c["psi0"]), what
    psi = c["psi0"].copy()
    call = lib.resample_call(psi, c["raws"], c["geoms"], c["k1"], c["k2"], 0.006, MINV, 3)
    call.geom[1].src_dims[0] = 0
    assert lib.l.mvn_deconvolve_resampled(C.c_void_p(call.psi_ptr), call.ws, C.byref(call.desc), call.geom, 1, 0) < 0
    assert "src_dims" in lib.l.mvn_last_error().decode()
    call.geom[1].src_dims[0] = c["raws"][1].shape[0]
    assert lib.l.mvn_deconvolve_resampled(C.c_void_p(call.psi_ptr), call.ws, C.byref(call.desc), None, 1, 0) < 0
    assert "geom" in lib.l.mvn_last_error().decode()
    assert lib.l.mvn_deconvolve_resampled(C.c_void_p(call.psi_ptr), call.ws, C.byref(call.desc), call.geom, 2, 0) < 0
    assert np.array_equal(psi, c["psi0"])


def check_memory_figure(lib):
    c = make_call("even block")
    call = lib.resample_call(c["psi0"].copy(), c["raws"], c["geoms"], c["k1"], c["k2"], 0.006, MINV, 3)
    before = lib.get_pad_mode()
    lib.set_pad_mode("zero")
    try:
        h = WorkspaceHolder([np.zeros(c["block"], F)] * 2, c["k1"], c["k2"], c["w"], 0.006, MINV, 3)
        described = lib.deconvolve_memory(h, 0)
        host = call.memory()
        for v in range(2):
            call.image[v].location = MVN_DEVICE
        device = call.memory()
    finally:
        lib.set_pad_mode(before)
    assert device == described, (device, described)
    assert host - described == max(r.nbytes for r in c["raws"]), (host, described)


def check_halo_engine_refuses(lib):
    c = make_call("even block")
    e = lib.engine(c["block"], 2)
    try:
        e.set_halo_hook(lambda spectrum, view, conv: None)
        try:
            e.set_view_resampled(0, c["raws"][0], c["geoms"][0], c["k1"][0], c["k2"][0])
        except Exception as err:
            assert "halo" in str(err)
        else:
            raise AssertionError("an engine with a halo hook took a resampled view")
    finally:
        e.close()


def check_engine_api(lib):
    """set_view_resampled + normalize_weights on a resident engine equal the plain engine on the library's stacks"""
    c = make_call("even block")
    images, ws = library_stacks(lib, c)
    wn = normalize_numpy(ws)
    res = []
    for resampled in (False, True):
        e = lib.engine(c["block"], 2)
        try:
            for v in range(2):
                if resampled:
                    e.set_view_resampled(v, c["raws"][v], c["geoms"][v], c["k1"][v], c["k2"][v])
                else:
                    e.set_view(v, images[v], wn[v], c["k1"][v], c["k2"][v])
            if resampled:
                e.normalize_weights()
            e.set_psi(c["psi0"])
            e.iterate(3, 0.006, MINV)
            res.append(e.get_psi())
        finally:
            e.close()
    assert np.array_equal(res[0], res[1])
    assert not np.array_equal(res[0], c["psi0"])


def check_image_storage_stays_float32(lib):
    c = make_call("even block", dtypes=(np.uint16, np.uint16))
    lib.check(lib.l.mvn_release_cached_engines())
    want = resampled_call(lib, c, "zero")
    lib.set_image_storage(1)
    try:
        before = lib.image_storage_counters()
        got = resampled_call(lib, c, "zero")
        assert lib.image_storage_counters() == before  # no divide pass on a uint16 image, no uint16 ingest
    finally:
        lib.set_image_storage(0)
        lib.check(lib.l.mvn_release_cached_engines())
    assert np.array_equal(got, want)
