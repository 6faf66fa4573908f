"""Derived kernels (csrc/mvn_psf.hpp, mvn_derive_kernels in include/mvn_engine_api.h): what the tests on the emulation
(test_emu_psf.py) and on the device (test_gpu_psf.py) share - a numpy restatement of the definition, the cases, and the
checks themselves, written once against a Binding.

The restatement holds every sum in float64, walks the taps of a correlation in raster order (t_0 outermost, ascending)
and is vectorised over the outputs only, so each output's sum sees its terms in the definition's order; numpy rounds
every array operation once and contracts nothing.

Allowance of the comparisons with the restatement: 1 unit in the last place of float32 per element.  The only order the
definition leaves free is that of S = sum q, a float64 sum of at most 1e5 float32 values: its relative spread over
summation orders is below 1e-11, the spacing of float32 is 6e-8, so a quotient q / S can change only where it sits on a
rounding tie.  Everything else (the correlations, the float32 products, the flips) is fixed to the bit.
"""
import ctypes as C
import math

import numpy as np

from libmultiviewnative_amd.abi import view_geometry
import resample_reference as rs

F = np.float32
TYPES = (0, 1, 2, 3)  # independent, efficient Bayesian, optimization I, optimization II
TYPE_NAMES = ("independent", "efficient_bayesian", "optimization_1", "optimization_2")
_C30, _S30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
IDENTITY = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
ROT30 = [[_C30, 0, _S30], [0, 1, 0], [-_S30, 0, _C30]]
Z4 = [[0.25, 0, 0], [0, 1, 0], [0, 0, 1]]
# matrix, raw extents, K: the table of the header's rule
EXTENTS_TABLE = [
    (IDENTITY, (5, 7, 9), (5, 7, 9)),
    (Z4, (9, 5, 7), (33, 5, 7)),
    ([[1 / 3, 0, 0], [0, 1, 0], [0, 0, 1]], (9, 5, 7), (25, 5, 7)),
    ([[0, 0, 1 / 3], [0, 1, 0], [-1.5, 0, 0]], (5, 7, 7), (5, 7, 13)),
    (ROT30, (5, 7, 9), (9, 7, 11)),
]
# name: (views as (linear part or None, raw extents), K given or None, K expected)
GROUPS = {
    # unequal axes, views smaller than K, an autocorrelation of (65, 13, 21): rows that cross a 64-lane wave
    "three views": ([(IDENTITY, (5, 7, 9)), (ROT30, (5, 7, 9)), (Z4, (9, 5, 7))], None, (33, 7, 11)),
    "one plane": ([(IDENTITY, (1, 3, 5)), (IDENTITY, (1, 3, 3)), (IDENTITY, (1, 1, 5))], None, (1, 3, 5)),
    "one view": ([(ROT30, (5, 7, 9))], None, (9, 7, 11)),
    "no geometry": ([(None, (3, 5, 7)), (None, (5, 3, 7))], None, (5, 5, 7)),
    "given extents": ([(IDENTITY, (5, 7, 9)), (ROT30, (5, 7, 9))], (7, 5, 9), (7, 5, 9)),
}


def geom_of(A, r):
    return view_geometry(r, [list(A[k]) + [0.0] for k in range(3)], (0, 0, 0), (0, 0, 0))


def raw_psf(shape, seed, zeros=False):
    """random positives raised to the sixth power: a peaked shape with tiny tails; zeros: some exact zeros"""
    rng = np.random.default_rng(seed + 31 * sum(shape))
    p = rng.random(shape, dtype=F) ** 6
    if zeros:
        p[rng.random(shape) < 0.3] = 0
    return np.ascontiguousarray(p, F)


def group(name, zeros=False):
    views, given, K = GROUPS[name]
    raws = [raw_psf(r, 5 + v, zeros) for v, (A, r) in enumerate(views)]
    geoms = None if views[0][0] is None else [geom_of(A, r) for A, r in views]
    return raws, geoms, given, K


# ---- the definition -------------------------------------------------------------------------------------------------
def extents_numpy(views):
    """K by the rule: h_k = ceil(s_k - 1e-6), s = |A^-1| cr"""
    best = np.zeros(3, int)
    for A, r in views:
        cr = (np.array(r) - 1) // 2
        if A is None:
            best = np.maximum(best, np.array(r))
            continue
        B = np.abs(np.linalg.inv(np.array(A, np.float64)))
        s = (B[:, 0] * cr[0] + B[:, 1] * cr[1]) + B[:, 2] * cr[2]
        best = np.maximum(best, 2 * np.ceil(s - 1e-6).astype(int) + 1)
    return tuple(int(k) for k in best)


def transform_geometry(A, r, K):
    """[A | t] with t_k = cr_k - ((A[k][0] h_0 + A[k][1] h_1) + A[k][2] h_2) in float64, every operation rounded once"""
    A = np.array(A, np.float64)
    h = [np.float64((k - 1) // 2) for k in K]
    M = np.zeros((3, 4))
    M[:, :3] = A
    for k in range(3):
        M[k, 3] = np.float64((r[k] - 1) // 2) - ((A[k, 0] * h[0] + A[k, 1] * h[1]) + A[k, 2] * h[2])
    return view_geometry(r, M, (0, 0, 0), (0, 0, 0))


def centred_copy(p, K):
    q = np.zeros(K, F)
    src, dst = [], []
    for k in range(3):
        r, cr, h = p.shape[k], (p.shape[k] - 1) // 2, (K[k] - 1) // 2
        if K[k] >= r:
            src.append(slice(0, r)), dst.append(slice(h - cr, h - cr + r))
        else:
            src.append(slice(cr - h, cr - h + K[k])), dst.append(slice(0, K[k]))
    q[tuple(dst)] = p[tuple(src)]
    return q


def normalise(q):
    S = float(np.sum(q.astype(np.float64)))
    assert S > 0 and math.isfinite(S)
    return (q.astype(np.float64) / S).astype(F)


def flip(a):
    return np.ascontiguousarray(a[::-1, ::-1, ::-1])


def corr(a, b, Eo):
    """corr(a, b)(d) = sum over t of a(-t) b(d - t): t in raster order, float64 sums from +0.0, one rounding to float32"""
    ca, cb, co = [(np.array(e) - 1) // 2 for e in (a.shape, b.shape, Eo)]
    out = np.zeros(Eo, np.float64)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for t0 in range(-ca[0], ca[0] + 1):
        for t1 in range(-ca[1], ca[1] + 1):
            for t2 in range(-ca[2], ca[2] + 1):
                t = np.array([t0, t1, t2])
                lo, hi = np.maximum(-co, t - cb), np.minimum(co, t + cb)  # the d whose d - t lies inside b
                if (lo > hi).any():
                    continue
                so = tuple(slice(lo[k] + co[k], hi[k] + co[k] + 1) for k in range(3))
                sb = tuple(slice(lo[k] - t[k] + cb[k], hi[k] - t[k] + cb[k] + 1) for k in range(3))
                out[so] = out[so] + a64[ca[0] - t0, ca[1] - t1, ca[2] - t2] * b64[sb]
    return out.astype(F)


def kernel2_numpy(P, type_):
    V, K = len(P), P[0].shape
    if type_ == 0:
        return [flip(p) for p in P]
    if type_ == 1:
        auto = [corr(flip(p), flip(p), [2 * k - 1 for k in K]) for p in P]
    out = []
    for v in range(V):
        T = flip(P[v])
        if type_ in (1, 2):
            for w in range(V):
                if w != v:
                    T = (T * corr(P[v], auto[w] if type_ == 1 else P[w], K)).astype(F)
        else:
            f = flip(P[v])
            for _ in range(V - 1):
                T = (T * f).astype(F)
        out.append(normalise(T))
    return out


def ulps(a, b):
    """distance in units in the last place between two arrays of non-negative float32"""
    assert a.dtype == F and b.dtype == F and a.shape == b.shape
    assert np.all(a >= 0) and np.all(b >= 0) and not np.isnan(a).any()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- 1. extents -----------------------------------------------------------------------------------------------------
def check_extents(lib):
    for A, r, K in EXTENTS_TABLE:
        assert lib.psf_extents([r], [geom_of(A, r)]) == K, (A, r)
        assert extents_numpy([(A, r)]) == K
    for name, (views, given, K) in GROUPS.items():
        if given is None:
            geoms = None if views[0][0] is None else [geom_of(A, r) for A, r in views]
            assert lib.psf_extents([r for _, r in views], geoms) == K == extents_numpy(views), name


# ---- 2. the kernels ---------------------------------------------------------------------------------------------------
_SEEN = {}


def derived(lib, name, type_, zeros=False):
    """the library's kernels of a group, once per (library, group, type)"""
    key = (lib.path, name, type_, zeros)
    if key not in _SEEN:
        raws, geoms, given, K = group(name, zeros)
        k1, k2 = lib.derive_kernels(raws, geoms, type_, out_dims=given)
        assert all(k.shape == K and k.dtype == F for k in k1 + k2)
        _SEEN[key] = (k1, k2)
    return _SEEN[key]


def check_kernel1(lib, name, zeros=False):
    """steps 1 and 2: q is mvn_resample_stack's image on the stated geometry (or the centred copy) bit for bit, so
    kernel1 is its quotient by S within the allowance, and exactly 0 where q is"""
    raws, geoms, given, K = group(name, zeros)
    k1, _ = derived(lib, name, 0, zeros)
    worst = 0
    for v, (A, r) in enumerate(GROUPS[name][0]):
        if A is None:
            q = centred_copy(raws[v], K)
        else:
            q, _ = lib.resample_stack(raws[v], transform_geometry(A, r, K), K)
        want = normalise(q)
        assert np.array_equal(k1[v] == 0, q == 0), (name, v)
        d = ulps(k1[v], want)
        worst = max(worst, int(d.max()))
        assert abs(float(k1[v].astype(np.float64).sum()) - 1) <= 1e-6 and k1[v].min() >= 0
        assert float(q.max()) > 0
    print("%s: kernel1 within %d units of the restatement" % (name, worst))
    assert worst <= 1, (name, worst)


def check_kernel2(lib, name, type_, zeros=False):
    """step 3, from the library's own kernel1"""
    k1, k2 = derived(lib, name, type_, zeros)
    want = kernel2_numpy(k1, type_)
    worst = 0
    for v in range(len(k1)):
        if type_ == 0:
            assert np.array_equal(k2[v], flip(k1[v])), (name, v)
            continue
        worst = max(worst, int(ulps(k2[v], want[v]).max()))
        assert abs(float(k2[v].astype(np.float64).sum()) - 1) <= 1e-6 and k2[v].min() >= 0, (name, type_, v)
    print("%s, %s: kernel2 within %d units of the restatement" % (name, TYPE_NAMES[type_], worst))
    assert worst <= 1, (name, type_, worst)
    if type_ in (1, 2) and len(k1) > 1:  # the types differ, and differ from the flipped kernel
        assert not np.array_equal(k2[0], flip(k1[0]))


def check_identical_symmetric_views(lib):
    z, y, x = np.meshgrid(*[np.arange(-(n // 2), n // 2 + 1, dtype=np.float64) for n in (5, 7, 9)], indexing="ij")
    p = np.exp(-(z * z / 2.0 + y * y / 4.5 + x * x / 8.0)).astype(F)
    assert np.array_equal(p, flip(p))
    k1, k2 = lib.derive_kernels([p, p], None, 1)
    assert np.array_equal(k1[0], k1[1]) and np.array_equal(k2[0], k2[1])
    assert int(ulps(k2[0], flip(k2[0])).max()) <= 1
    assert not np.array_equal(k2[0], k1[0])


# ---- 3. the surface of mvn_derive_kernels -----------------------------------------------------------------------------
def derive_raw(lib, raws, dims, geoms, type_, out_dims, k1, k2):
    n = len(raws)
    tab = lambda arrs: (C.POINTER(C.c_float) * n)(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
    garr = (type(geoms[0]) * n)(*geoms) if geoms else None
    return lib.l.mvn_derive_kernels(0, n, tab(raws), (C.c_int * (3 * n))(*[x for d in dims for x in d]), garr, type_,
                                    (C.c_int * 3)(*out_dims) if out_dims else None, tab(k1), tab(k2))


def check_derive_errors(lib):
    raws, geoms, _, K = group("three views")
    dims = [p.shape for p in raws]
    k1 = [np.full(K, -3, F) for _ in raws]
    k2 = [np.full(K, -3, F) for _ in raws]
    singular = [geoms[0], geom_of([[1, 0, 0], [2, 0, 0], [0, 0, 1]], dims[1]), geoms[2]]
    nan_lin = [geoms[0], geom_of([[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]], dims[1]), geoms[2]]
    bad_value = [raws[0], raws[1].copy(), raws[2]]
    bad_value[1][1, 2, 3] = np.inf
    massless = [raws[0], np.zeros_like(raws[1]), raws[2]]
    negative = [raws[0], -raws[1], raws[2]]
    cases = {
        "even raw extents": (raws, [(4, 7, 9)] + dims[1:], geoms, 1, None),
        "raw extents < 1": (raws, [(0, 7, 9)] + dims[1:], geoms, 1, None),
        "a non-finite PSF value": (bad_value, dims, geoms, 1, None),
        "a singular linear part": (raws, dims, singular, 1, None),
        "a non-finite linear part": (raws, dims, nan_lin, 1, None),
        "a bad type": (raws, dims, geoms, 4, None),
        "a negative type": (raws, dims, geoms, -1, None),
        "even out_dims": (raws, dims, geoms, 1, (33, 8, 11)),
        "out_dims above 257": (raws, dims, geoms, 1, (259, 7, 11)),
        "a kernel without mass": (massless, dims, geoms, 1, None),
        "a kernel of negative mass": (negative, dims, geoms, 1, None),
    }
    for what, (r, d, g, t, od) in cases.items():
        rc = derive_raw(lib, r, d, g, t, od, k1, k2)
        assert rc < 0 and lib.l.mvn_last_error().decode(), what
        assert all(np.all(k == -3) for k in k1 + k2), what
    assert lib.l.mvn_derive_kernels(0, 0, None, None, None, 1, None, None, None) < 0
    assert derive_raw(lib, raws, dims, geoms, 1, None, k1, k2) == 0 and not np.any(k1[0] == -3)


# ---- 4. the call ------------------------------------------------------------------------------------------------------
CALL_PSFS = ((5, 5, 5), (3, 5, 7))
# Under padding "none" the library refuses a kernel with an extent above the image's, and the kernels derived from
# CALL_PSFS exceed the blocks of rs.CALL_VIEWS ((3, 5, 7) and (4, 6, 10)): there both routes must be refused alike.
# These smaller PSFs derive to (3, 3, 3) for either block, so that "none" is also compared on calls that run.
SMALL_PSFS = ((3, 3, 3), (1, 3, 3))


def call_psfs(shapes=CALL_PSFS):
    return [raw_psf(r, 40 + v) for v, r in enumerate(shapes)]


def with_derivation(lib, type_, fn):
    before = lib.get_kernel_derivation()
    lib.set_kernel_derivation(1, type_)
    try:
        return fn()
    finally:
        lib.set_kernel_derivation(*before)


def derived_call(lib, c, psfs, mode, type_, geoms=None, iters=3):
    """mvn_deconvolve_resampled with derivation on: kernel1_ the raw PSFs, kernel2_ NULL; returns (status, psi)"""
    psi = c["psi0"].copy()
    call = lib.resample_call(psi, c["raws"], geoms or c["geoms"], psfs, None, 0.006, rs.MINV, iters)

    def run():
        return lib.l.mvn_deconvolve_resampled(C.c_void_p(call.psi_ptr), call.ws, C.byref(call.desc), call.geom, 1, 0)

    rc = with_derivation(lib, type_, lambda: rs.with_pad_mode(lib, mode, run))
    return rc, psi, call


def check_call(lib, key, mode, type_, shapes=CALL_PSFS):
    """derivation on == derivation off with mvn_derive_kernels' arrays handed in, bit for bit; the memory figures agree.
    Where the library refuses the derived kernels for the block (see SMALL_PSFS) both routes are refused with the same
    message and leave psi as it was."""
    c = rs.make_call(key)
    psfs = call_psfs(shapes)
    k1, k2 = lib.derive_kernels(psfs, c["geoms"], type_)
    lib.check(lib.l.mvn_release_cached_engines())
    want = c["psi0"].copy()
    plain = lib.resample_call(want, c["raws"], c["geoms"], k1, k2, 0.006, rs.MINV, 3)
    rc_plain = rs.with_pad_mode(lib, mode, lambda: lib.l.mvn_deconvolve_resampled(
        C.c_void_p(plain.psi_ptr), plain.ws, C.byref(plain.desc), plain.geom, 1, 0))
    why_plain = lib.l.mvn_last_error().decode() if rc_plain < 0 else ""
    rc, got, call = derived_call(lib, c, psfs, mode, type_)
    if rc_plain < 0:
        fits = all(k <= b for k, b in zip(k1[0].shape, c["block"]))
        assert mode == "none" and not fits, (key, mode, why_plain)
        assert rc < 0 and lib.l.mvn_last_error().decode() == why_plain, (key, mode, why_plain)
        assert np.array_equal(got, c["psi0"]) and np.array_equal(want, c["psi0"])
        return None
    assert rc == 0, lib.l.mvn_last_error().decode()
    assert not np.array_equal(want, c["psi0"])
    assert np.array_equal(got, want), (key, mode, type_, int((got != want).sum()))
    need = rs.with_pad_mode(lib, mode, plain.memory)
    assert with_derivation(lib, type_, lambda: rs.with_pad_mode(lib, mode, call.memory)) == need
    return got


def check_types_differ(lib):
    res = [check_call(lib, "even block", "zero", t) for t in TYPES]
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(res[i], res[j]), (i, j)


def shifted_geoms(c, shift):
    geoms = []
    for n in c["names"]:
        block, raw, M, border, rng = rs.CASES[n]
        M = np.asarray(M, np.float64).copy()
        M[:, 3] = M[:, 3] + M[:, :3] @ np.asarray(shift, np.float64)
        geoms.append(view_geometry(raw, M, border, rng))
    return geoms


def check_block_after_block(lib):
    """another fourth column and the same PSFs: the derivation is re-used, nothing is correlated, the spectra are kept"""
    c = rs.make_call("even block")
    psfs = call_psfs()
    lib.check(lib.l.mvn_release_cached_engines())
    lib.derive_kernels([raw_psf((3, 3, 3), 1)], None, 0)  # (whatever the cache holds is none of this test's)
    steps = []
    for shift, ps, type_ in (((0, 0, 0), psfs, 1), ((1, 2, 3), psfs, 1), ((1, 2, 3), [psfs[0], psfs[1] * F(1.5)], 1),
                             ((1, 2, 3), [psfs[0], psfs[1] * F(1.5)], 2)):
        d0, p0 = lib.derive_counters(), lib.psf_cache_counters()
        rc, got, _ = derived_call(lib, c, ps, "zero", type_, geoms=shifted_geoms(c, shift))
        assert rc == 0 and not np.array_equal(got, c["psi0"])
        d1, p1 = lib.derive_counters(), lib.psf_cache_counters()
        steps.append((tuple(a - b for a, b in zip(d1, d0)), p1[0] - p0[0], got))
    first, second, changed_bytes, changed_type = steps
    assert first[0][1:] == (1, 0) and first[0][0] == 2  # autocorrelations and cropped correlations: one launch each
    assert second[0] == (0, 0, 1) and second[1] > 0 and first[1] == 0
    assert not np.array_equal(first[2], second[2])
    assert changed_bytes[0] == (2, 1, 0) and changed_type[0] == (1, 1, 0)
    # mode 0 moves no counter
    d0 = lib.derive_counters()
    rs.resampled_call(lib, c, "zero")
    assert lib.derive_counters() == d0
    lib.check(lib.l.mvn_release_cached_engines())


def check_call_errors_leave_psi_untouched(lib):
    c = rs.make_call("even block")
    psfs = call_psfs()
    nan_psf = psfs[1].copy()
    nan_psf[0, 0, 0] = np.nan
    singular = [c["geoms"][0], view_geometry(rs.CASES[c["names"][1]][1], [[0, 0, 1, 0], [0, 0, 2, 0], [1, 0, 0, 0]],
                                             (0, 0, 0), (0, 0, 0))]
    cases = {
        "even raw extents": ([psfs[0], np.ones((3, 4, 7), F)], None),
        "a non-finite PSF value": ([psfs[0], nan_psf], None),
        "a kernel without mass": ([psfs[0], np.zeros((3, 5, 7), F)], None),
        "a singular linear part": (psfs, singular),
    }
    for what, (ps, geoms) in cases.items():
        d0 = lib.derive_counters()
        rc, psi, _ = derived_call(lib, c, ps, "zero", 1, geoms=geoms)
        assert rc < 0 and lib.l.mvn_last_error().decode(), what
        assert np.array_equal(psi, c["psi0"]), what
        assert lib.derive_counters()[1:] == d0[1:], what
    for mode, type_ in ((2, 0), (-1, 0), (1, 4), (1, -1)):
        assert lib.l.mvn_set_kernel_derivation(mode, type_) < 0
    assert lib.get_kernel_derivation() == (0, 0)
