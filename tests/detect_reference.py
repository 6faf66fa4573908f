"""Bead detection (csrc/mvn_detect.hpp, mvn_detect_beads in include/mvn_engine_api.h): what the tests on the emulation
(test_emu_detect.py) and on the device (test_gpu_detect.py) share - a numpy restatement of the definition, the cases,
and the checks themselves, written once against a Binding.

The restatement: float32 arrays for the blurs (numpy rounds every array operation once and contracts nothing) - the
mirrored volume is gathered once per axis, then the products are added tap by tap in ascending order from the first
product -, a boolean mask for the 26 strict comparisons, numpy's argwhere for the raster order, and Python floats
(IEEE doubles, one rounding per operation) for the fit, cofactor by cofactor as the header writes it.  The taps are the
library's (mvn_detect_taps), as the header prescribes for the bit-for-bit checks; check_taps compares them with numpy's
formula.

Allowances.  D, the candidates, their values and positions: zero - every order of operations is fixed.  The taps: one
float32 ulp against numpy's exp (two correctly rounded libraries may differ in the last bit of a double, which the
rounding to float32 can carry over a tie).  Planted beads: 0.1 voxel in the max norm, the figure of the issue; the
restatement's own error is printed first (0.036 voxel at these settings, on the emulation and on the device).

One case differs from its statement in the issue, which cannot be built: a stack of (24, 30, 70) does not hold 16
centres that are 13 apart AND 7 from every face - along axis 0 only the planes 7..16 qualify, two centres that share
(y, x) closer than 13 would have to be 13 planes apart, and the 16 x 56 positions of a plane hold at most 2 x 5 centres
13 apart.  The centres here form the 2 x 2 x 4 grid that does fit: planes 5 and 18 (5 from the faces of axis 0),
rows 8 and 21, columns 9, 26, 43, 60 - 13 apart or more, and 7 or more from the faces of the other two axes.
"""
import ctypes as C
import math

import numpy as np

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_F32, MVN_HOST, StackDesc, describe_stack, detect_params
from beads_reference import HOST, EMU_PLACES, apart, mir, stack  # noqa: F401  (the places and layouts are shared)

F = np.float32
DTYPES = (np.uint16, np.float32)
# (5, 6, 40): narrower than the radius, several reflections.  No extent of (34, 37, 300) is a multiple of a tile
# (rows: 4 x 256; lines: 64 x 64; extrema: 64 x 16 x 32 planes), and it has more than one workgroup in every pass
STACKS = ((5, 6, 40), (9, 11, 70), (34, 37, 300))
Q = 2.0 ** 0.25
SIGMAS = (
    ((1.5, 1.5, 1.5), (1.5 * Q, 1.5 * Q, 1.5 * Q)),
    ((1.0, 2.0, 2.0), (1.3, 2.4, 2.4)),
    ((0.0, 1.5, 1.5), (0.0, 1.8, 1.8)),
    ((2.5, 2.5, 2.5), (3.0, 3.0, 3.0)),
)
CAPACITY = 8192
THRESHOLD = {np.uint16: 8.0, np.float32: 2.0}  # about the deviation of D on the random values of `values`


# ---- the definition -------------------------------------------------------------------------------------------------
def taps_numpy(sigma):
    """the header's formula with numpy's exp"""
    R = int(math.ceil(3.0 * sigma))
    if R == 0:
        return np.ones(1, F)
    i = np.arange(-R, R + 1)
    g = np.exp(-(i * i).astype(np.float64) / ((2.0 * sigma) * sigma))
    S = g[0]
    for v in g[1:]:
        S = S + v
    return (g / S).astype(F)


def blur(u, w, k):
    """u blurred along axis k with the taps w: ascending taps, the sum started from the first product, float32"""
    assert u.dtype == F and w.dtype == F
    R, n = (len(w) - 1) // 2, u.shape[k]
    pad = np.take(u, mir(np.arange(-R, n + R), n), axis=k)
    cut = lambda j: pad[tuple(slice(j, j + n) if a == k else slice(None) for a in range(3))]
    acc = w[0] * cut(0)
    for j in range(1, 2 * R + 1):
        acc = acc + w[j] * cut(j)
    assert acc.dtype == F
    return acc


def dog_numpy(lib, raw, sigma1, sigma2):
    L = []
    for sigma in (sigma1, sigma2):
        v = np.asarray(raw).astype(F)
        for k in (2, 1, 0):
            v = blur(v, lib.detect_taps(sigma[k]), k)
        L.append(v)
    return L[0] - L[1]


def fit(E):
    """(o, the unrestricted o or None) from the 27 values of E around a candidate"""
    e = [[[float(E[a, b, c]) for c in range(3)] for b in range(3)] for a in range(3)]
    c = e[1][1][1]
    g0 = (e[2][1][1] - e[0][1][1]) / 2.0
    g1 = (e[1][2][1] - e[1][0][1]) / 2.0
    g2 = (e[1][1][2] - e[1][1][0]) / 2.0
    h00 = (e[2][1][1] + e[0][1][1]) - 2.0 * c
    h11 = (e[1][2][1] + e[1][0][1]) - 2.0 * c
    h22 = (e[1][1][2] + e[1][1][0]) - 2.0 * c
    h01 = ((e[2][2][1] - e[2][0][1]) - (e[0][2][1] - e[0][0][1])) / 4.0
    h02 = ((e[2][1][2] - e[2][1][0]) - (e[0][1][2] - e[0][1][0])) / 4.0
    h12 = ((e[1][2][2] - e[1][2][0]) - (e[1][0][2] - e[1][0][0])) / 4.0
    c00 = h11 * h22 - h12 * h12
    c01 = h02 * h12 - h01 * h22
    c02 = h01 * h12 - h02 * h11
    c11 = h00 * h22 - h02 * h02
    c12 = h01 * h02 - h00 * h12
    c22 = h00 * h11 - h01 * h01
    det = (h00 * c00 + h01 * c01) + h02 * c02
    n = [(c00 * g0 + c01 * g1) + c02 * g2, (c01 * g0 + c11 * g1) + c12 * g2, (c02 * g0 + c12 * g1) + c22 * g2]
    if det == 0.0 or not math.isfinite(det):
        return [0.0, 0.0, 0.0], None
    o = [-x / det for x in n]
    if not all(math.isfinite(x) and abs(x) <= 1.0 for x in o):
        return [0.0, 0.0, 0.0], o
    return o, o


def detect_numpy(D, threshold, minima=False):
    """(positions, values, voxels) of the candidates of D in raster order"""
    E = -D if minima else D
    m = E.shape
    if min(m) < 3:
        return np.zeros((0, 3)), np.zeros(0, F), np.zeros((0, 3), np.int32)
    core = E[1:-1, 1:-1, 1:-1]
    with np.errstate(invalid="ignore"):
        mask = core > F(threshold)
        for d0 in range(3):
            for d1 in range(3):
                for d2 in range(3):
                    if (d0, d1, d2) != (1, 1, 1):
                        mask &= core > E[d0:d0 + m[0] - 2, d1:d1 + m[1] - 2, d2:d2 + m[2] - 2]
    vox = (np.argwhere(mask) + 1).astype(np.int32)  # C order: ascending raster index
    pos = np.zeros((len(vox), 3))
    for i, c in enumerate(vox):
        o, _ = fit(E[c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2, c[2] - 1:c[2] + 2])
        pos[i] = [float(c[k]) + o[k] for k in range(3)]
    return pos, E[tuple(vox.T)].astype(F), vox


# ---- the cases ------------------------------------------------------------------------------------------------------
def values(m, dtype, seed=0):
    """random values plus planted blobs of sigma 1.5, some of them next to the faces"""
    rng = np.random.default_rng(seed + 7 * sum(m))
    vals = rng.random(m) * (3910.0 if dtype is np.uint16 else 900.0) + (90.0 if dtype is np.uint16 else 100.0)
    grid = [np.arange(n, dtype=np.float64) for n in m]
    for _ in range(max(4, int(np.prod(m)) // 2500)):
        p = rng.random(3) * (np.array(m) - 1)
        g = [np.exp(-((grid[k] - p[k]) ** 2) / 4.5) for k in range(3)]
        vals += 3000.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    return np.rint(vals).astype(np.uint16) if dtype is np.uint16 else vals.astype(F)


_SHARED = {}


def reference(lib, m, dtype, sig):
    """(values, D of the restatement), computed once per case and left unchanged"""
    key = (m, dtype, sig)
    if key not in _SHARED:
        vals = values(m, dtype)
        D = dog_numpy(lib, vals, *SIGMAS[sig])
        vals.setflags(write=False), D.setflags(write=False)
        _SHARED[key] = (vals, D)
    return _SHARED[key]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 0. the taps ------------------------------------------------------------------------------------------------------
def check_taps(lib):
    for sigma in sorted({s for pair in SIGMAS for trio in pair for s in trio} | {0.3, 1.0 / 3.0, 10.0}):
        got, want = lib.detect_taps(sigma), taps_numpy(sigma)
        assert got.dtype == F and len(got) == 2 * int(math.ceil(3 * sigma)) + 1 == len(want), sigma
        assert np.all(np.abs(got - want) <= np.spacing(np.maximum(got, want))), sigma  # one float32 ulp
        assert np.array_equal(got, got[::-1]) and abs(float(got.astype(np.float64).sum()) - 1) < 1e-6, sigma
    assert np.array_equal(lib.detect_taps(0.0), np.ones(1, F))
    assert len(lib.detect_taps(10.0)) == 2 * native.DETECT_MAX_RADIUS + 1
    taps, r = np.full(8, -3, F), C.c_int(-3)
    for sigma, cap in ((-0.5, 8), (float("nan"), 8), (float("inf"), 8), (10.5, 8), (1.5, 10)):
        assert lib.l.mvn_detect_taps(sigma, taps.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(r)) < 0, sigma
        assert np.all(taps == -3) and r.value == -3, sigma


# ---- 1. D, bit for bit ------------------------------------------------------------------------------------------------
def check_dog(lib, m, sig, places):
    s1, s2 = SIGMAS[sig]
    for dtype in DTYPES:
        vals, want = reference(lib, m, dtype, sig)
        for where, (place, kw) in sorted(places.items()):
            got = lib.detect_dog(stack(np.array(vals), "dense", place), s1, s2, **kw)
            assert got.dtype == F and same_bits(got, want), (m, sig, dtype, where)


# ---- 2. detections, bit for bit -----------------------------------------------------------------------------------------
def check_detections(lib, m, sig, places, layouts=("dense",)):
    s1, s2 = SIGMAS[sig]
    for dtype in DTYPES:
        vals, D = reference(lib, m, dtype, sig)
        for minima in (False, True):
            pos, val, vox = detect_numpy(D, THRESHOLD[dtype], minima)
            print("%s %s sigma set %d %s: %d candidates" % (m, dtype.__name__, sig, "minima" if minima else "maxima", len(vox)))
            if m == STACKS[2] and sig == 0:
                # several workgroups of the extremum pass append: the raster order is the sort's, not the schedule's
                tiles = {(int(c[0]) // 32, int(c[1]) // 16, int(c[2]) // 64) for c in vox}
                assert len(vox) > 256 and len(tiles) > 8, (len(vox), len(tiles))
            assert len(vox) <= CAPACITY
            for layout in layouts:
                for where, (place, kw) in sorted(places.items()):
                    held = np.array(vals)
                    first = None
                    for _ in range(3):
                        got = lib.detect_beads(stack(held, layout, place), s1, s2, THRESHOLD[dtype], minima=minima,
                                               capacity=CAPACITY, **kw)
                        first = first or got
                        assert all(same_bits(a, b) for a, b in zip(got, first)), (m, sig, dtype, where, "repeat")
                    what = (m, sig, dtype, minima, layout, where)
                    assert len(got[2]) == len(vox) and same_bits(got[2], vox), what
                    assert same_bits(got[1], val), what
                    assert same_bits(got[0], pos), what


def check_one_value(lib, places):
    """a stack of one value (strides {0, 0, 0}): D is a plateau, nothing is found, and D is the restatement's"""
    m = STACKS[1]
    s1, s2 = SIGMAS[0]
    for dtype in DTYPES:
        vals = values(m, dtype)
        flat = np.broadcast_to(vals[:1, :1, :1], m)
        want = dog_numpy(lib, flat, s1, s2)
        for where, (place, kw) in sorted(places.items()):
            assert same_bits(lib.detect_dog(stack(vals, "one value", place), s1, s2, **kw), want), (dtype, where)
            for minima in (False, True):
                got = lib.detect_beads(stack(vals, "one value", place), s1, s2, -1e30, minima=minima, **kw)
                assert len(got[0]) == 0 and len(detect_numpy(want, -1e30, minima)[2]) == 0, (dtype, where)


# ---- 3. closed form, independent of the restatement ---------------------------------------------------------------------
def check_closed_form(lib, places=HOST):
    m, c, A = (24, 26, 40), (11, 12, 20), F(1000.0)  # at least R + 1 = 10 from every face
    for sig in (0, 1, 2, 3):
        s1, s2 = SIGMAS[sig]
        want = np.zeros(m, F)
        for sign, sigma in ((1, s1), (-1, s2)):
            w = [lib.detect_taps(s) for s in sigma]
            R = [(len(x) - 1) // 2 for x in w]
            assert all(c[k] - R[k] >= 1 and c[k] + R[k] <= m[k] - 2 for k in range(3))
            t = (A * w[2]).astype(F)                                   # fl(A w2[d2])
            t = (t[None, :] * w[1][:, None]).astype(F)                 # fl(. w1[d1])
            t = (t[None, :, :] * w[0][:, None, None]).astype(F)        # fl(. w0[d0])
            box = np.zeros(m, F)
            box[tuple(slice(c[k] - R[k], c[k] + R[k] + 1) for k in range(3))] = t
            want = want + box if sign > 0 else want - box
        raw = np.zeros(m, F)
        raw[c] = A
        for where, (place, kw) in sorted(places.items()):
            held = stack(raw, "dense", place)
            assert same_bits(lib.detect_dog(held, s1, s2, **kw), want), (sig, where)
            pos, val, vox = lib.detect_beads(held, s1, s2, 0.5, **kw)
            assert len(vox) == 1 and tuple(vox[0]) == c, (sig, where, vox)
            assert tuple(pos[0]) == tuple(float(x) for x in c) and val[0] == want[c], (sig, where, pos)  # g is zero


# ---- 4. planted beads ---------------------------------------------------------------------------------------------------
BEAD_STACK, BEAD_SIGMA, BEAD_AMPLITUDE, BEAD_BASE = (24, 30, 70), 1.5, 3000.0, 100.0
BEAD_TOL = 0.1  # voxel, max norm: the issue's condition


def planted_beads(seed=5):
    rng = np.random.default_rng(seed)
    grid = np.array([(z, y, x) for z in (5, 18) for y in (8, 21) for x in (9, 26, 43, 60)], np.float64)
    d = np.abs(grid[:, None, :] - grid[None, :, :]).max(axis=2) + 99 * np.eye(len(grid))
    assert len(grid) == 16 and d.min() >= 13
    centres = grid + rng.random(grid.shape) - 0.5
    ax = [np.arange(n, dtype=np.float64) for n in BEAD_STACK]
    vals = np.full(BEAD_STACK, BEAD_BASE)
    for p in centres:
        g = [np.exp(-((ax[k] - p[k]) ** 2) / (2 * BEAD_SIGMA ** 2)) for k in range(3)]
        vals += BEAD_AMPLITUDE * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    noisy = np.minimum(rng.poisson(vals), 65535).astype(np.uint16)
    return centres, {"float32": vals.astype(F), "uint16": np.rint(vals).astype(np.uint16), "uint16 + Poisson": noisy}


def worst_miss(pos, centres):
    """the largest max-norm distance from a centre to its detection; inf unless every centre has a detection of its
    own (the raster order of the detections need not be the centres': two voxels of a grid row may swap)"""
    if len(pos) != len(centres):
        return float("inf")
    d = np.abs(pos[:, None, :] - centres[None, :, :]).max(axis=2)
    if sorted(d.argmin(axis=0)) != list(range(len(centres))):
        return float("inf")
    return float(d.min(axis=0).max())


def check_planted_beads(lib):
    centres, stacks = planted_beads()
    s1, s2 = (1.5,) * 3, (1.5 * Q,) * 3
    for name, vals in stacks.items():
        want = detect_numpy(dog_numpy(lib, vals, s1, s2), 20.0)
        print("planted beads, %s: the restatement finds %d, worst error %.4f voxel"
              % (name, len(want[0]), worst_miss(want[0], centres)))
        pos, val, vox = lib.detect_beads(vals, s1, s2, 20.0)
        assert len(pos) == 16 and all(same_bits(a, b) for a, b in zip((pos, val, vox), want)), name
        err = worst_miss(pos, centres)
        print("planted beads, %s: worst error of the library %.4f voxel" % (name, err))
        assert err <= BEAD_TOL, (name, err)
        psf = lib.extract_psf(vals, pos, (9, 9, 9))
        assert np.unravel_index(int(np.argmax(psf)), psf.shape) == (4, 4, 4), name


# ---- 5. offsets beyond the bound ------------------------------------------------------------------------------------------
def second_difference_stack(lib, P, c, m):
    """A float32 stack whose D is EXACTLY the 3 x 3 x 3 integer pattern P around c and zero elsewhere (the last plane
    aside).  sigma1 = 0 makes L_1 the stack itself; sigma2 = (s, 0, 0) with the taps {1/128, 1 - 1/64, 1/128} makes
    D = u - L_2 = -(u(z-1) - 2 u(z) + u(z+1)) / 128, exact for small multiples of 128: u is -128 P summed twice
    along axis 0."""
    s = math.sqrt(-1.0 / (2.0 * math.log((1.0 / 128) / (1 - 1.0 / 64))))
    assert np.array_equal(lib.detect_taps(s), np.array([1.0 / 128, 1 - 1.0 / 64, 1.0 / 128], F)), lib.detect_taps(s)
    want = np.zeros(m, np.float64)
    want[tuple(slice(c[k] - 1, c[k] + 2) for k in range(3))] = P
    u = np.zeros(m, np.float64)
    for z in range(1, m[0] - 1):
        u[z + 1] = 2 * u[z] - u[z - 1] - 128.0 * want[z]
    assert np.abs(u).max() < 2 ** 20
    return u.astype(F), (0.0, 0.0, 0.0), (s, 0.0, 0.0), want.astype(F)


def check_offsets_beyond_the_bound(lib, places=HOST):
    m, c = (7, 6, 8), (3, 3, 3)
    base = np.ones((3, 3, 3)) * 2.0
    base[1, 1, 1] = 20.0
    # |o| > 1: g = (1, -1, 0), H = [[-4, -3.5, 0], [-3.5, -4, 0], [0, 0, -4]]: o = (2, -2, 0)
    far = base.copy()
    far[2, 1, 1], far[0, 1, 1], far[1, 2, 1], far[1, 0, 1], far[1, 1, 2], far[1, 1, 0] = 19, 17, 17, 19, 18, 18
    far[2, 2, 1] = far[0, 0, 1] = 11
    far[2, 0, 1] = far[0, 2, 1] = 18
    # det H = 0: g = (1, 0, 0), H = [[-4, -4, 0], [-4, -4, 0], [0, 0, -4]]
    flat = base.copy()
    flat[2, 1, 1], flat[0, 1, 1], flat[1, 2, 1], flat[1, 0, 1], flat[1, 1, 2], flat[1, 1, 0] = 19, 17, 18, 18, 18, 18
    flat[2, 2, 1] = flat[0, 0, 1] = 10
    flat[2, 0, 1] = flat[0, 2, 1] = 18
    for name, P in (("|o| > 1", far), ("det H = 0", flat)):
        o, raw_o = fit(P)
        if name == "|o| > 1":
            assert raw_o == [2.0, -2.0, -0.0] or [abs(x) for x in raw_o] == [2.0, 2.0, 0.0], raw_o
        else:
            assert raw_o is None
        assert o == [0.0, 0.0, 0.0]
        for minima in (False, True):
            u, s1, s2, want = second_difference_stack(lib, -P if minima else P, c, m)
            for where, (place, kw) in sorted(places.items()):
                held = stack(u, "dense", place)
                D = lib.detect_dog(held, s1, s2, **kw)
                assert np.array_equal(D[:-1], want[:-1]), (name, where)  # the pattern, exactly
                pos, val, vox = lib.detect_beads(held, s1, s2, 0.5, minima=minima, **kw)
                assert len(vox) == 1 and tuple(vox[0]) == c and val[0] == 20.0, (name, where, vox)
                assert tuple(pos[0]) == (3.0, 3.0, 3.0), (name, where, pos)
                ref = detect_numpy(D, 0.5, minima)
                assert all(same_bits(a, b) for a, b in zip((pos, val, vox), ref)), (name, where)


# ---- 6. errors leave the outputs untouched --------------------------------------------------------------------------------
def detect_raw(lib, ptr, desc, m, prm, capacity, n, pos, val, vox):
    return lib.l.mvn_detect_beads(0, C.c_void_p(ptr), C.byref(desc) if desc is not None else None, (C.c_int * 3)(*m),
                                  C.byref(prm) if prm is not None else None, capacity,
                                  C.byref(n) if n is not None else None,
                                  pos.ctypes.data_as(C.POINTER(C.c_double)) if pos is not None else None,
                                  val.ctypes.data_as(C.POINTER(C.c_float)) if val is not None else None,
                                  vox.ctypes.data_as(C.POINTER(C.c_int)) if vox is not None else None, None)


def check_errors(lib):
    m = STACKS[1]
    vals = values(m, np.float32)
    s1, s2 = SIGMAS[0]
    thr = THRESHOLD[np.float32]
    found = len(detect_numpy(dog_numpy(lib, vals, s1, s2), thr)[2])
    assert found >= 3
    n, pos, val, vox = C.c_int(-3), np.full((64, 3), -3.0), np.full(64, -3, F), np.full((64, 3), -3, np.int32)
    untouched = lambda: np.all(pos == -3) and np.all(val == -3) and np.all(vox == -3)
    good = detect_params(s1, s2, thr)

    def prm(**kw):
        p = detect_params(kw.get("s1", s1), kw.get("s2", s2), kw.get("threshold", thr), kw.get("flags", 0))
        return p

    ptr, desc, shape, _ = describe_stack(vals)
    cases = {
        "a negative sigma": (prm(s1=(1.5, -0.1, 1.5)), 64),
        "a NaN sigma": (prm(s2=(1.5, 1.5, float("nan"))), 64),
        "an infinite sigma": (prm(s1=(float("inf"), 1.5, 1.5)), 64),
        "a sigma above 10": (prm(s2=(10.5, 1.5, 1.5)), 64),
        "a NaN threshold": (prm(threshold=float("nan")), 64),
        "an infinite threshold": (prm(threshold=float("inf")), 64),
        "an unknown flag": (prm(flags=2), 64),
        "a capacity of 0": (good, 0),
        "a negative capacity": (good, -1),
    }
    before = lib.detect_counters()
    for what, (p, cap) in cases.items():
        assert detect_raw(lib, ptr, desc, shape, p, cap, n, pos, val, vox) < 0, what
        assert lib.l.mvn_last_error().decode(), what
        assert n.value == -3 and untouched(), what
    for what, args in {
        "a null stack": (None, desc, shape, good, 64, n, pos, val, vox),
        "a null prm": (ptr, desc, shape, None, 64, n, pos, val, vox),
        "a null num_found": (ptr, desc, shape, good, 64, None, pos, val, vox),
        "a null positions_out": (ptr, desc, shape, good, 64, n, None, val, vox),
        "an extent of 0": (ptr, desc, (0, 11, 70), good, 64, n, pos, val, vox),
    }.items():
        assert detect_raw(lib, *args) < 0, what
        assert n.value == -3 and untouched(), what
    for bad in (dict(dtype=7), dict(location=5), dict(stride=(-1, 70, 1)), dict(stride=(770, 70, 2))):
        d = StackDesc()
        d.dtype, d.location = bad.get("dtype", MVN_F32), bad.get("location", MVN_HOST)
        for k in range(3):
            d.stride[k] = bad.get("stride", (770, 70, 1))[k]
        assert detect_raw(lib, ptr, d, shape, good, 64, n, pos, val, vox) < 0 and n.value == -3 and untouched(), bad
    assert lib.detect_counters() == before  # nothing was launched, nothing completed
    # more candidates than the capacity: the count, and nothing else.  (The passes that counted them were launched:
    # the launch counters say so; no detection completed.)
    assert detect_raw(lib, ptr, desc, shape, good, found - 1, n, pos, val, vox) < 0
    assert n.value == found and untouched() and str(found) in lib.l.mvn_last_error().decode()
    after = lib.detect_counters()
    assert after[2] == before[2] and (after[0] - before[0], after[1] - before[1]) == (3, 1)
    # ... and with that capacity the call succeeds; values_out and voxels_out may be NULL
    n.value = -3
    assert detect_raw(lib, ptr, desc, shape, good, found, n, pos, None, None) == 0
    assert n.value == found and np.all(pos[:found] != -3) and np.all(pos[found:] == -3) and np.all(val == -3)
    assert lib.detect_counters()[2] == before[2] + 1
    # an extent below 3: nothing found, no error
    for thin in ((2, 11, 70), (9, 1, 70), (9, 11, 2)):
        n.value = -3
        held = np.ascontiguousarray(vals[:thin[0], :thin[1], :thin[2]])
        p2, d2, sh2, _ = describe_stack(held)
        assert detect_raw(lib, p2, d2, sh2, good, 64, n, pos, val, vox) == 0 and n.value == 0, thin
        assert np.all(val == -3) and np.all(vox == -3)
        assert same_bits(lib.detect_dog(held, s1, s2), dog_numpy(lib, held, s1, s2)), thin


# ---- 7. memory, counters, timing ----------------------------------------------------------------------------------------
def memory_model(m, capacity):
    return 16 * int(np.prod(m)) + 1536 + 8 + 48 * capacity


def check_memory(lib):
    m = STACKS[1]
    for dtype in DTYPES:
        vals = values(m, dtype)
        for capacity in (1, 100, 4096):
            resident = lib.detect_memory(vals, capacity, as_device=True)
            assert resident == memory_model(m, capacity), (dtype, capacity)
            assert lib.detect_memory(vals, capacity) == resident + vals.nbytes
            assert lib.detect_memory(stack(vals, "pitched", lambda a: a), capacity) == resident + vals.nbytes
            assert lib.detect_memory(stack(vals, "one value", lambda a: a), capacity) == resident + vals.itemsize
    need = C.c_size_t(5)
    assert lib.l.mvn_detect_memory(None, (C.c_int * 3)(*m), 0, 0, C.byref(need)) < 0
    assert lib.l.mvn_detect_memory(None, (C.c_int * 3)(*m), 7, 0, C.byref(need)) == 0
    assert need.value == memory_model(m, 7) + 4 * int(np.prod(m))  # NULL: dense float32 in host memory


def check_counters_and_timing(lib):
    m = STACKS[1]
    vals = values(m, np.uint16)
    s1, s2 = SIGMAS[0]
    c0 = lib.detect_counters()
    lib.detect_beads(vals, s1, s2, THRESHOLD[np.uint16])
    c1 = lib.detect_counters()
    assert tuple(a - b for a, b in zip(c1, c0)) == (3, 1, 1)
    lib.detect_dog(vals, s1, s2)
    c2 = lib.detect_counters()
    assert tuple(a - b for a, b in zip(c2, c1)) == (3, 0, 0)
    for u16 in (True, False):
        ms = lib.detect_time((12, 20, 80), s1, s2, 50.0, u16=u16, reps=2)
        assert len(ms) == 3 and all(x > 0 for x in ms), ms
    c3 = lib.detect_counters()
    assert tuple(a - b for a, b in zip(c3, c2)) == (2 * (3 + 6 * 3), 2 * (1 + 3), 0)
    prm = detect_params(s1, s2, 50.0)
    assert lib.l.mvn_detect_time(0, 1, (C.c_int * 3)(12, 20, 80), C.byref(prm), 0, (C.c_float * 3)()) < 0
