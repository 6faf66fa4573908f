"""Bead PSFs (csrc/mvn_beads.hpp, mvn_extract_psf in include/mvn_engine_api.h): what the tests on the emulation
(test_emu_beads.py) and on the device (test_gpu_beads.py) share - a numpy restatement of the definition, the cases, and
the checks themselves, written once against a Binding.

The restatement is vectorised over the PSF voxels and loops over the beads: float32 arrays for the three lerps (numpy
rounds every array operation once and contracts nothing), float64 for the group sums, in the stated order - beads in
the order given inside groups of 32 from +0.0, the groups in order from P_0 itself, one division, one rounding.

Allowances.  psf_out: zero - every sum order is fixed.  Scores: 1e-6 - the windows are random uniform values, so the
cancellation in the variances costs a small factor, the double sums over at most 2e4 terms are good to 1e-11, and a
wrong window moves a score by far more.  The planted PSF's centroid: 0.05 voxel, with the restatement's own error below
half of that (checked first, on the CPU), so the bound is the definition's and not the kernel's.
"""
import ctypes as C
import math

import numpy as np

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import MVN_F32, MVN_HOST, StackDesc, describe_stack
import psf_reference as pr
import resample_reference as rs

F = np.float32
GROUP = native.BEADS_GROUP
DTYPES = (np.uint16, np.float32)
STACKS = ((9, 11, 70), (6, 7, 40))
# (5, 3, 67): a row that crosses a 64-lane wave; (7, 9, 11) in (6, 7, 40): wider than the stack along two axes
PSFS = ((3, 5, 7), (1, 3, 5), (5, 3, 67), (7, 9, 11))
COUNTS = (1, 32, 33, 70)  # the group boundary from both sides
LAYOUTS = ("dense", "pitched", "one value")
# where a stack lies: name -> (array -> the object handed to the binding, keywords of the call).  The emulation's
# pointers may be called device memory; test_gpu_beads.py adds tensors on the device in a child process.
HOST = {"host": (lambda a: a, {})}
EMU_PLACES = dict(HOST, device=(lambda a: a, {"as_device": True}))


def apart(fn, *args):
    """fn(*args) in a thread of its own.  The library's last error is per thread and no call clears it: checks that
    provoke errors run apart, so that tests of the same process that expect an empty last error still find one."""
    import threading
    box = []

    def run():
        try:
            fn(*args)
        except BaseException as e:  # handed to the caller's thread
            box.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box:
        raise box[0]


# ---- the definition -------------------------------------------------------------------------------------------------
def mir(i, n):
    """the mirror without repeating the edge sample (numpy.pad's "reflect"), for any integer i"""
    if n == 1:
        return np.zeros_like(i)
    q = np.mod(i, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


def lerp(p, q, f):
    assert p.dtype == F and q.dtype == F and type(f) is F
    d = q - p
    t = f * d
    return p + t


def window(raw, pos, r):
    """s_b(j) for every voxel j of the window of extents r around the bead at pos: float32"""
    m = raw.shape
    lo, hi, f = [], [], []
    for k in range(3):
        B = int(math.floor(pos[k]))
        f.append(F(np.float64(pos[k]) - np.float64(B)))
        i = B + np.arange(r[k]) - (r[k] - 1) // 2
        lo.append(mir(i, m[k])), hi.append(mir(i + 1, m[k]))
    S = lambda a, b, c: np.asarray(raw[np.ix_(a, b, c)]).astype(F)
    a = {(p, q): lerp(S(x0, x1, lo[2]), S(x0, x1, hi[2]), f[2])
         for p, x0 in enumerate((lo[0], hi[0])) for q, x1 in enumerate((lo[1], hi[1]))}
    b = [lerp(a[(p, 0)], a[(p, 1)], f[1]) for p in range(2)]
    out = lerp(b[0], b[1], f[0])
    assert out.dtype == F and out.shape == tuple(r)
    return out


def extract_numpy(raw, beads, r, remove_min=False):
    beads = np.asarray(beads, np.float64).reshape(-1, 3)
    T = None
    for g in range(0, len(beads), GROUP):
        P = np.zeros(r, np.float64)
        for pos in beads[g:g + GROUP]:
            P = P + window(raw, pos, r).astype(np.float64)
        T = P if T is None else T + P
    psf = (T / np.float64(len(beads))).astype(F)
    return (psf - psf.min()).astype(F) if remove_min else psf


def scores_numpy(raw, beads, r, psf):
    """Pearson's correlation of every bead's window with psf (before its minimum is removed), in float64"""
    P = psf.astype(np.float64)
    n = float(P.size)
    out = []
    for pos in np.asarray(beads, np.float64).reshape(-1, 3):
        s = window(raw, pos, r).astype(np.float64)
        cov = (s * P).sum() - s.sum() * P.sum() / n
        den = math.sqrt(max(((s * s).sum() - s.sum() ** 2 / n) * ((P * P).sum() - P.sum() ** 2 / n), 0.0))
        out.append(cov / den if den > 0 and math.isfinite(den) else 0.0)
    return np.array(out)


# ---- the cases ------------------------------------------------------------------------------------------------------
def values(m, dtype, seed=0):
    rng = np.random.default_rng(seed + 7 * sum(m))
    if dtype is np.uint16:
        return rng.integers(90, 4000, m, dtype=np.uint16)
    return (rng.random(m, dtype=F) * F(900.0) + F(100.0)).astype(F)


def specials(m):
    """the corner, the far corner m - 1 exactly (the high neighbour mirrors and meets f = 0), an integer position, and a
    hair below an integer along every axis"""
    top = [x - 1 for x in m]
    mid = [float(x // 2) for x in m]
    below = [float(np.nextafter(np.float64(max(x // 2, 1)), 0.0)) if x > 1 else 0.0 for x in m]
    return [[0.0, 0.0, 0.0], [float(x) for x in top], mid, below]


def positions(m, count, seed=0):
    """count positions inside the stack that begin with the special ones"""
    rng = np.random.default_rng(seed + count + 13 * sum(m))
    pts = specials(m)
    while len(pts) < count:
        p = rng.random(3) * (np.array(m) - 1)
        if len(pts) % 5 == 0:
            p = np.floor(p)
        pts.append([float(x) for x in p])
    return np.array(pts[:count], np.float64)


def stack(vals, layout, place):
    """the values as a stack of the layout, lying where `place` puts arrays"""
    m = vals.shape
    if layout == "dense":
        return place(np.ascontiguousarray(vals))
    if layout == "pitched":  # a row pitch above m2
        big = np.full((m[0], m[1], m[2] + 5), 7, vals.dtype)
        big[:, :, :m[2]] = vals
        return place(big)[:, :, :m[2]]
    one = place(np.ascontiguousarray(vals[:1, :1, :1]))  # strides {0, 0, 0}
    return one.expand(*m) if hasattr(one, "expand") else np.broadcast_to(one, m)


# ---- 1. bit equality with the restatement -----------------------------------------------------------------------------
def check_bits(lib, m, r, places):
    for dtype in DTYPES:
        vals = values(m, dtype)
        for count in COUNTS:
            sets = [positions(m, count)] if count > 1 else [np.array([p]) for p in specials(m)]
            for beads in sets:
                want = extract_numpy(vals, beads, r)
                for where, (place, kw) in sorted(places.items()):
                    got = lib.extract_psf(stack(vals, "dense", place), beads, r, **kw)
                    assert got.dtype == F and np.array_equal(got, want), (m, r, dtype, count, where, beads[0])
        # a row pitch above m2, and one value for every voxel
        beads = positions(m, 33, seed=3)
        for layout in LAYOUTS[1:]:
            held = vals if layout == "pitched" else np.broadcast_to(vals[:1, :1, :1], m)
            want = extract_numpy(held, beads, r)
            for where, (place, kw) in sorted(places.items()):
                got = lib.extract_psf(stack(vals, layout, place), beads, r, **kw)
                assert np.array_equal(got, want), (m, r, dtype, layout, where)


# ---- 2. closed form ---------------------------------------------------------------------------------------------------
def check_closed_form(lib, places=HOST):
    m, r = STACKS[0], PSFS[0]
    h = [(x - 1) // 2 for x in r]
    B = (4, 5, 30)  # at least h + 1 from every face
    cut = tuple(slice(B[k] - h[k], B[k] + h[k] + 1) for k in range(3))
    for dtype in DTYPES:
        vals = values(m, dtype, seed=2)
        for where, (place, kw) in sorted(places.items()):
            raw = stack(vals, "dense", place)
            one = lib.extract_psf(raw, [B], r, **kw)
            assert np.array_equal(one, vals[cut].astype(F)), (dtype, where)
            assert np.array_equal(lib.extract_psf(raw, [B, B], r, **kw), one), (dtype, where)
            flat = lib.extract_psf(raw, [B, B], r, remove_min=True, **kw)
            assert flat.min() == 0 and np.array_equal(flat, extract_numpy(vals, [B, B], r, remove_min=True))
        beads = positions(m, 33, seed=5)
        got = lib.extract_psf(vals, beads, r, remove_min=True)
        assert got.min() == 0 and np.array_equal(got, extract_numpy(vals, beads, r, remove_min=True)), dtype


# ---- 3. scores --------------------------------------------------------------------------------------------------------
SCORE_TOL = 1e-6


def planted(m, r, centres, dtype, seed, noise_at=None):
    """a flat stack with the same random window (and one cell more: the high neighbours) at every centre"""
    rng = np.random.default_rng(seed)
    h = [(x - 1) // 2 for x in r]
    ext = [x + 1 for x in r]
    draw = lambda: rng.integers(100, 4000, ext) if dtype is np.uint16 else rng.random(ext) * 900 + 100
    pattern = draw()
    vals = np.full(m, 50, np.float64)
    for i, c in enumerate(centres):
        cut = tuple(slice(c[k] - h[k], c[k] - h[k] + ext[k]) for k in range(3))
        vals[cut] = pattern if i != noise_at else draw()  # (noise of the pattern's own distribution)
    return vals.astype(dtype)


def check_scores(lib, places=HOST):
    m, r = STACKS[0], PSFS[0]
    for dtype in DTYPES:
        vals = values(m, dtype, seed=4)  # random uniform values
        for count in (1, 33, 70):
            beads = positions(m, count, seed=9)
            for where, (place, kw) in sorted(places.items()):
                for remove_min in (False, True):
                    psf, sc = lib.extract_psf(stack(vals, "dense", place), beads, r, remove_min=remove_min, scores=True,
                                              **kw)
                    assert np.array_equal(psf, extract_numpy(vals, beads, r, remove_min))
                    want = scores_numpy(vals, beads, r, extract_numpy(vals, beads, r))
                    err = float(np.abs(sc - want).max())
                    print("scores of %d beads, %s, %s: worst error %.3g" % (count, dtype.__name__, where, err))
                    assert err <= SCORE_TOL and np.all(np.abs(sc) <= 1 + SCORE_TOL), (dtype, count, where, err)
        # identical beads score 1; one of them replaced by noise scores below every other
        centres = [(2, 3, 5), (2, 3, 20), (2, 3, 35), (6, 7, 50), (6, 7, 62)]
        same = planted(m, r, centres, dtype, 11)
        _, sc = lib.extract_psf(same, centres, r, scores=True)
        assert np.all(np.abs(sc - 1) <= SCORE_TOL), sc
        odd = planted(m, r, centres, dtype, 11, noise_at=3)
        _, sc = lib.extract_psf(odd, centres, r, scores=True)
        assert np.argmin(sc) == 3 and sc[3] < np.delete(sc, 3).min(), sc
        assert float(np.abs(sc - scores_numpy(odd, centres, r, extract_numpy(odd, centres, r))).max()) <= SCORE_TOL
        # a constant stack (a value whose sums are exact in double): exactly 0
        const = np.full(m, 1000 if dtype is np.uint16 else 3.5, dtype)
        psf, sc = lib.extract_psf(const, positions(m, 33), r, scores=True)
        assert np.all(psf == const[0, 0, 0]) and np.all(sc == 0), sc


# ---- 4. a planted PSF -------------------------------------------------------------------------------------------------
BLOB_STACK, BLOB_PSF, BLOB_SIGMA = (24, 28, 96), (9, 9, 9), (1.2, 1.4, 1.5)
CENTROID_TOL = 0.05


def blob_beads():
    """40 sub-voxel positions, no two closer than the window, every window (and its high neighbours) inside the stack"""
    rng = np.random.default_rng(17)
    pts = [(z + rng.random() * 0.25, y + rng.random() * 0.25, 5.02 + 9.4 * i + rng.random() * 0.04)
           for z in (5.3, 17.7) for y in (6.25, 20.6) for i in range(10)]
    return np.array(pts, np.float64)


def blob_stack():
    beads = blob_beads()
    grid = [np.arange(n, dtype=np.float64) for n in BLOB_STACK]
    vals = np.zeros(BLOB_STACK, np.float64)
    for p in beads:
        g = [np.exp(-((grid[k] - p[k]) ** 2) / (2 * BLOB_SIGMA[k] ** 2)) for k in range(3)]
        vals += 1000.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    return vals.astype(F), beads


def centroid(psf):
    P = psf.astype(np.float64)
    return [float((P * np.arange(P.shape[k]).reshape([-1 if a == k else 1 for a in range(3)])).sum() / P.sum())
            - (P.shape[k] - 1) / 2 for k in range(3)]


def check_planted_psf(lib):
    vals, beads = blob_stack()
    d = np.abs(beads[:, None, :] - beads[None, :, :]).max(axis=2) + 99 * np.eye(len(beads))
    assert len(beads) == 40 and d.min() >= 9  # no two closer than the window
    want = extract_numpy(vals, beads, BLOB_PSF)
    own = max(abs(c) for c in centroid(want))
    print("centroid error of the restatement: %.4f voxel" % own)
    assert own < CENTROID_TOL / 2  # the bound is the definition's
    psf, sc = lib.extract_psf(vals, beads, BLOB_PSF, scores=True)
    got = max(abs(c) for c in centroid(psf))
    print("centroid error of the library: %.4f voxel; lowest score %.4f" % (got, sc.min()))
    assert got <= CENTROID_TOL and np.array_equal(psf, want)
    assert sc.min() > 0.9  # every bead is a copy of the PSF, resampled about itself
    # the kernel derivation accepts it, and a resampled call that derives from it is the call on the restatement's PSF
    k1, k2 = lib.derive_kernels([psf], None, 0)
    assert abs(float(k1[0].astype(np.float64).sum()) - 1) <= 1e-6
    c = rs.make_call("even block")
    lib.check(lib.l.mvn_release_cached_engines())
    for type_ in (0, 1):
        rc, got_psi, _ = pr.derived_call(lib, c, [psf, psf], "zero", type_)
        rc2, want_psi, _ = pr.derived_call(lib, c, [want, want], "zero", type_)
        assert rc == 0 and rc2 == 0, lib.l.mvn_last_error().decode()
        assert not np.array_equal(got_psi, c["psi0"]) and np.array_equal(got_psi, want_psi), type_


# ---- 5. errors leave the outputs untouched --------------------------------------------------------------------------------
def extract_raw(lib, ptr, desc, m, beads, r, flags, psf, scores, num_beads=None):
    beads = np.ascontiguousarray(beads, np.float64).reshape(-1, 3)
    return lib.l.mvn_extract_psf(0, C.c_void_p(ptr), C.byref(desc) if desc is not None else None, (C.c_int * 3)(*m),
                                 beads.ctypes.data_as(C.POINTER(C.c_double)),
                                 len(beads) if num_beads is None else num_beads, (C.c_int * 3)(*r), flags,
                                 psf.ctypes.data_as(C.POINTER(C.c_float)) if psf is not None else None,
                                 scores.ctypes.data_as(C.POINTER(C.c_double)) if scores is not None else None, None)


def check_errors(lib):
    m, r = STACKS[1], PSFS[0]
    vals = values(m, np.float32)
    beads = positions(m, 4)  # (the special ones: no window of theirs reaches the NaN below)
    nan_stack = vals.copy()
    nan_stack[1, 5, 30] = np.nan
    under_the_nan = np.vstack([beads, [[1.0, 4.5, 30.25]]])
    psf, sc = np.full(r, -3, F), np.full(8, -3.0)
    edit = lambda k, v: np.vstack([beads[:2], [[v if a == k else beads[2][a] for a in range(3)]], beads[3:]])
    cases = {
        "even extents": (vals, beads, (3, 4, 7), 0, None),
        "an extent of 131": (vals, beads, (3, 5, 131), 0, None),
        "an extent of 0": (vals, beads, (0, 5, 7), 0, None),
        "an unknown flag": (vals, beads, r, 2, None),
        "a NaN position": (vals, edit(1, np.nan), r, 0, None),
        "an infinite position": (vals, edit(0, np.inf), r, 0, None),
        "a position of m - 1 + 1e-9": (vals, edit(2, m[2] - 1 + 1e-9), r, 0, None),
        "a negative position": (vals, edit(0, -1e-9), r, 0, None),
        "no beads": (vals, beads, r, 0, 0),
        "a NaN under a bead": (nan_stack, under_the_nan, r, 0, None),
    }
    before = lib.extract_counters()
    for what, (raw, bd, rr, flags, count) in cases.items():
        ptr, desc, shape, _ = describe_stack(raw)
        rc = extract_raw(lib, ptr, desc, shape, bd, rr, flags, psf, sc, count)
        why = lib.l.mvn_last_error().decode()
        assert rc < 0 and why, what
        assert np.all(psf == -3) and np.all(sc == -3), what
        if "position" in what:
            assert "bead 2" in why, (what, why)
        if what == "a NaN under a bead":
            assert "a non-finite PSF" in why, why
    ptr, desc, shape, _ = describe_stack(vals)
    assert extract_raw(lib, None, desc, shape, beads, r, 0, psf, sc) < 0  # null pointers
    assert extract_raw(lib, ptr, desc, shape, beads, r, 0, None, sc) < 0
    assert lib.l.mvn_extract_psf(0, C.c_void_p(ptr), C.byref(desc), (C.c_int * 3)(*m), None, 4, (C.c_int * 3)(*r), 0,
                                 psf.ctypes.data_as(C.POINTER(C.c_float)), None, None) < 0
    for bad in (dict(dtype=7), dict(location=5), dict(stride=(-1, 40, 1)), dict(stride=(280, 40, 2))):
        d = StackDesc()
        d.dtype, d.location = bad.get("dtype", MVN_F32), bad.get("location", MVN_HOST)
        for k in range(3):
            d.stride[k] = bad.get("stride", (280, 40, 1))[k]
        assert extract_raw(lib, ptr, d, shape, beads, r, 0, psf, sc) < 0 and np.all(psf == -3), bad
    assert extract_raw(lib, ptr, desc, (0, 7, 40), beads, r, 0, psf, sc) < 0
    assert lib.extract_counters()[2] == before[2]  # nothing completed
    # the NaN is the only thing wrong with that stack, and the outputs are written on success
    assert extract_raw(lib, *describe_stack(nan_stack)[:3], beads, r, 0, psf, sc) == 0
    assert not np.any(psf == -3) and np.all(sc[:4] != -3) and np.all(sc[4:] == -3)
    assert lib.extract_counters()[2] == before[2] + 1


# ---- 6. memory, counters, timing ----------------------------------------------------------------------------------------
def memory_model(num_beads, r, scores):
    n, G = int(np.prod(r)), -(-num_beads // GROUP)
    return 32 * num_beads + 8 * G * n + 4 * n + 1028 + ((10240 + 8) * num_beads if scores else 0)


def check_memory(lib):
    m, r = STACKS[0], PSFS[2]
    for dtype in DTYPES:
        vals = values(m, dtype)
        for count in (1, 33, 70):
            for scores in (False, True):
                resident = lib.extract_memory(vals, count, r, scores, as_device=True)
                assert resident == memory_model(count, r, scores), (count, scores)
                assert lib.extract_memory(vals, count, r, scores) == resident + vals.nbytes
                assert lib.extract_memory(stack(vals, "pitched", lambda a: a), count, r, scores) == resident + vals.nbytes
                one = stack(vals, "one value", lambda a: a)
                assert lib.extract_memory(one, count, r, scores) == resident + vals.itemsize
    need = C.c_size_t(5)
    assert lib.l.mvn_extract_memory(None, (C.c_int * 3)(*m), 0, (C.c_int * 3)(*r), 0, 0, C.byref(need)) < 0
    assert lib.l.mvn_extract_memory(None, (C.c_int * 3)(*m), 4, (C.c_int * 3)(*r), 0, 0, C.byref(need)) == 0
    assert need.value == memory_model(4, r, False) + 4 * int(np.prod(m))  # NULL: dense float32 in host memory


def check_counters_and_timing(lib):
    m, r = STACKS[1], PSFS[1]
    vals = values(m, np.uint16)
    c0 = lib.extract_counters()
    lib.extract_psf(vals, positions(m, 70), r)
    c1 = lib.extract_counters()
    assert tuple(a - b for a, b in zip(c1, c0)) == (1, 0, 1)  # one launch of the gather whatever the bead count
    lib.extract_psf(vals, positions(m, 33), r, remove_min=True, scores=True)
    c2 = lib.extract_counters()
    assert tuple(a - b for a, b in zip(c2, c1)) == (1, 1, 1)
    for u16 in (True, False):
        ms = lib.extract_time((8, 16, 80), 40, (3, 5, 7), u16=u16, reps=2)
        assert len(ms) == 3 and all(x > 0 for x in ms), ms
    c3 = lib.extract_counters()
    assert tuple(a - b for a, b in zip(c3, c2)) == (2 * 3, 0, 0)
    assert lib.l.mvn_extract_time(0, 1, (C.c_int * 3)(4, 16, 80), 40, (C.c_int * 3)(3, 5, 7), 2, (C.c_float * 3)()) < 0
