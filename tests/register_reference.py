"""Bead registration (csrc/mvn_register.hpp, mvn_register_beads in include/mvn_engine_api.h): what the tests on the
emulation (test_emu_register.py) and on the device (test_gpu_register.py) share - a numpy restatement of steps 1 to 7
of the definition, the cases, and the checks themselves, written once against a Binding.

The restatement: numpy float64 arrays for the prior, the squared distances and the residuals, float32 arrays for the
descriptor distances (numpy rounds every array operation once and contracts nothing; sums are written out term by
term, never numpy.sum, whose pairwise order is not the definition's), a stable argsort for the (distance, index) order,
Python integers under a 64-bit mask for the sample, and Python floats (IEEE doubles, one rounding per operation) for the
fit and the refit, cofactor by cofactor as the header writes them.

Allowances.  Neighbours, candidates with d1 and d2, the counts, the inlier pairs, the matrix and the errors against the
restatement: zero - every order of operations is fixed.  Against numpy.linalg.lstsq on the returned pairs: 1e-9
entrywise, the issue's figure (the same least-squares problem solved another way in double; coordinates are <= 200
and S_aa is well conditioned, so either rounding is below 1e-11).

Sets.  B = a subset of A under a rotation of 2 degrees about axis 0 through the box centre, the scales
(1.01, 0.99, 1.005) and a shift, with Gaussian noise, plus uniform outliers, permuted.  The exact case (no noise,
max_error 1e-6, all 60 pairs expected) needs every bead to be a candidate, which the definition grants only where the
transform keeps each bead's neighbour ORDER: the map changes a distance by a factor in 0.99 .. 1.01, so two neighbours
whose distances differ by less than 1.01 / 0.99 may swap, and a swapped pair of the first three leaves no common
descriptor.  `separated_set` therefore re-draws beads until the five nearest distances of every bead are at least
2.5 % apart - a rule on the set alone.
"""
import ctypes as C
import math

import numpy as np

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import register_params
from beads_reference import apart  # noqa: F401

F = np.float32
MASK = (1 << 64) - 1
BOX = (60.0, 200.0, 200.0)
SIZES = ((5, 5, 0), (60, 48, 12), (65, 64, 1), (257, 200, 57), (300, 240, 60))  # (nA, kept, outliers)
HYPOTHESES = (1, 255, 257, 1000)
RATIO, MAX_ERROR, MIN_INLIERS = 3.0, 0.5, 4
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))
SHIFT = (1.5, -2.0, 3.0)


# ---- the sets --------------------------------------------------------------------------------------------------------
def truth_matrix(angle_deg=2.0, scales=(1.01, 0.99, 1.005), shift=SHIFT, centre=None):
    """(L | t) of b = R S (a - c) + c + shift: a rotation about axis 0 through c after the scales."""
    c = np.asarray(centre if centre is not None else [x / 2 for x in BOX], np.float64)
    w = math.radians(angle_deg)
    R = np.array([[1, 0, 0], [0, math.cos(w), -math.sin(w)], [0, math.sin(w), math.cos(w)]], np.float64)
    L = R @ np.diag(np.asarray(scales, np.float64))
    t = c + np.asarray(shift, np.float64) - L @ c
    return np.concatenate([L, t[:, None]], axis=1)


def apply(M, p):
    M = np.asarray(M, np.float64).reshape(3, 4)
    return p @ M[:, :3].T + M[:, 3]


def make_sets(na, kept, outliers, noise=0.05, seed=0, a=None, M=None):
    """(a, b, true) with true[j] = the index in a of bead j of b, or -1 for an outlier."""
    rng = np.random.default_rng([seed, na, kept, outliers])
    if a is None:
        a = rng.uniform(0.0, 1.0, (na, 3)) * np.asarray(BOX)
    M = truth_matrix() if M is None else M
    keep = rng.permutation(na)[:kept]
    b = apply(M, a[keep])
    if noise:
        b = b + rng.normal(0.0, noise, b.shape)
    b = np.concatenate([b, rng.uniform(0.0, 1.0, (outliers, 3)) * np.asarray(BOX)])
    true = np.concatenate([keep, np.full(outliers, -1)])
    perm = rng.permutation(len(b))
    return np.ascontiguousarray(a), np.ascontiguousarray(b[perm]), true[perm]


def separated_set(n, seed=0, gap=1.025, tries=100000):
    """n points of the box whose five nearest distances, bead by bead, are a factor `gap` apart: their neighbour order
    survives a map that changes distances by less."""
    rng = np.random.default_rng([seed, n, 77])
    p = rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(BOX)
    for _ in range(tries):
        d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(d, np.inf)
        near = np.sort(d, axis=1)[:, :5]
        bad = np.nonzero((near[:, 1:] < gap * near[:, :-1]).any(axis=1))[0]
        if len(bad) == 0:
            return np.ascontiguousarray(p)
        p[bad[0]] = rng.uniform(0.0, 1.0, 3) * np.asarray(BOX)
    raise AssertionError("no separated set")


# ---- the definition ----------------------------------------------------------------------------------------------------
def prior_apply(a, T):
    T = np.asarray(T, np.float64).reshape(3, 4)
    z, y, x = a[:, 0], a[:, 1], a[:, 2]
    return np.stack([((T[k, 0] * z + T[k, 1] * y) + T[k, 2] * x) + T[k, 3] for k in range(3)], axis=1)


def neighbours_numpy(p):
    n = len(p)
    d = p[None, :, :] - p[:, None, :]  # d[i, j] = p_j - p_i
    D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.argsort(D, axis=1, kind="stable")  # (distance, index) ascending
    rows = np.arange(n)[:, None]
    return order[order != rows].reshape(n, n - 1)[:, :4].astype(np.int32)  # the index is excluded, not a zero distance


def descriptors_numpy(p, nn):
    q = (p[nn] - p[:, None, :]).astype(F)  # (n, 4, 3)
    return np.stack([q[:, list(t), :].reshape(len(p), 9) for t in TRIPLES], axis=1)  # (n, 4, 9)


def match_numpy(da, db):
    """(d1, j1, d2) per bead of A."""
    d = np.full((len(da), len(db)), np.inf, F)
    for x in range(4):
        for y in range(4):
            e = da[:, None, x, :] - db[None, :, y, :]
            s = e[..., 0] * e[..., 0]
            for k in range(1, 9):
                s = s + e[..., k] * e[..., k]
            d = np.minimum(d, s)
    j1 = np.argmin(d, axis=1)  # (the first of equal minima: the lower j)
    rows = np.arange(len(da))
    d1 = d[rows, j1]
    rest = d.copy()
    rest[rows, j1] = np.inf
    return d1, j1.astype(np.int32), rest.min(axis=1)


def candidates_numpy(a, b, ratio=RATIO, prior=None):
    """(pairs (K, 2), distances (K, 2)) of steps 1 to 4."""
    ap = prior_apply(a, prior) if prior is not None else a
    da = descriptors_numpy(ap, neighbours_numpy(ap))
    db = descriptors_numpy(b, neighbours_numpy(b))
    d1, j1, d2 = match_numpy(da, db)
    passes = d1 * F(ratio) < d2
    claims = np.bincount(j1[passes], minlength=len(b))
    keep = np.nonzero(passes & (claims[j1] == 1))[0]
    return (np.stack([keep, j1[keep]], axis=1).astype(np.int32).reshape(-1, 2),
            np.stack([d1[keep], d2[keep]], axis=1).astype(F).reshape(-1, 2))


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample_numpy(seed, h, n):
    picks = []
    for q in range(4):
        u = mix((seed + 0x9E3779B97F4A7C15 * (16 * h + q + 1)) & MASK)
        r = ((u >> 32) * (n - q)) >> 32
        for s in sorted(picks):
            if s <= r:
                r += 1
        picks.append(r)
    return picks


def solve(E, G):
    """L = (G adj E) / det E by cofactors (lists of 3 lists of Python floats), or None."""
    c = [[E[1][1] * E[2][2] - E[1][2] * E[2][1], E[1][2] * E[2][0] - E[1][0] * E[2][2], E[1][0] * E[2][1] - E[1][1] * E[2][0]],
         [E[0][2] * E[2][1] - E[0][1] * E[2][2], E[0][0] * E[2][2] - E[0][2] * E[2][0], E[0][1] * E[2][0] - E[0][0] * E[2][1]],
         [E[0][1] * E[1][2] - E[0][2] * E[1][1], E[0][2] * E[1][0] - E[0][0] * E[1][2], E[0][0] * E[1][1] - E[0][1] * E[1][0]]]
    det = (E[0][0] * c[0][0] + E[0][1] * c[0][1]) + E[0][2] * c[0][2]
    if det == 0.0 or not math.isfinite(det):
        return None
    L = [[((G[k][0] * c[j][0] + G[k][1] * c[j][1]) + G[k][2] * c[j][2]) / det for j in range(3)] for k in range(3)]
    return L if all(math.isfinite(v) for row in L for v in row) else None


def offset(L, ca, cb):
    t = [cb[k] - ((L[k][0] * ca[0] + L[k][1] * ca[1]) + L[k][2] * ca[2]) for k in range(3)]
    return t if all(math.isfinite(v) for v in t) else None


def fit4(a4, b4):
    """The model through four pairs (lists of 4 lists of 3 floats), or None."""
    E = [[a4[c + 1][k] - a4[0][k] for c in range(3)] for k in range(3)]
    G = [[b4[c + 1][k] - b4[0][k] for c in range(3)] for k in range(3)]
    L = solve(E, G)
    if L is None:
        return None
    t = offset(L, a4[0], b4[0])
    return None if t is None else (L, t)


def residual2(model, ra, rb):
    """The squared residuals of the records (arrays (K, 3)) under a model: a float64 array."""
    L, t = model
    r = [(((L[k][0] * ra[:, 0] + L[k][1] * ra[:, 1]) + L[k][2] * ra[:, 2]) + t[k]) - rb[:, k] for k in range(3)]
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]


def ransac_numpy(ra, rb, hyps, seed, max_error):
    """(score, h) of the best hypothesis."""
    best = (0, 0)
    la, lb = ra.tolist(), rb.tolist()
    bound = max_error * max_error
    for h in range(hyps):
        s = sample_numpy(seed, h, len(ra))
        model = fit4([la[m] for m in s], [lb[m] for m in s])
        score = 0 if model is None else int(np.count_nonzero(residual2(model, ra, rb) <= bound))
        if score > best[0]:
            best = (score, h)
    return best


def refit_numpy(ra, rb, inl, min_inliers, max_error, refits=native.REGISTER_REFITS):
    bound = max_error * max_error
    la, lb = ra.tolist(), rb.tolist()
    model = None
    for _ in range(refits):
        n = len(inl)
        ca, cb = [], []
        for k in range(3):
            sa, sb = la[inl[0]][k], lb[inl[0]][k]
            for m in inl[1:]:
                sa, sb = sa + la[m][k], sb + lb[m][k]
            ca.append(sa / float(n))
            cb.append(sb / float(n))
        Saa = [[0.0] * 3 for _ in range(3)]
        Sba = [[0.0] * 3 for _ in range(3)]
        for k in range(3):
            for l in range(3):
                saa = sba = None
                for m in inl:
                    al = la[m][l] - ca[l]
                    paa, pba = (la[m][k] - ca[k]) * al, (lb[m][k] - cb[k]) * al
                    saa = paa if saa is None else saa + paa
                    sba = pba if sba is None else sba + pba
                Saa[k][l], Sba[k][l] = saa, sba
        L = solve(Saa, Sba)
        t = None if L is None else offset(L, ca, cb)
        if t is None:
            return None, []
        model = (L, t)
        nxt = np.nonzero(residual2(model, ra, rb) <= bound)[0].tolist()
        if len(nxt) < min_inliers:
            return None, []
        same = nxt == inl
        inl = nxt
        if same:
            break
    return model, inl


def register_numpy(a, b, hyps, max_error=MAX_ERROR, ratio=RATIO, min_inliers=MIN_INLIERS, prior=None, seed=0):
    """{'nc', 'matrix' (3, 4) or None, 'pairs' (K, 2), 'errors' (2,) or None} of steps 1 to 7."""
    pairs, _ = candidates_numpy(a, b, ratio, prior)
    out = {"nc": len(pairs), "matrix": None, "pairs": np.zeros((0, 2), np.int32), "errors": None}
    if len(pairs) < 4:
        return out
    ra, rb = np.ascontiguousarray(a[pairs[:, 0]]), np.ascontiguousarray(b[pairs[:, 1]])
    score, h = ransac_numpy(ra, rb, hyps, seed, max_error)
    if score < min_inliers:
        return out
    s = sample_numpy(seed, h, len(ra))
    model = fit4([ra[m].tolist() for m in s], [rb[m].tolist() for m in s])
    inl = np.nonzero(residual2(model, ra, rb) <= max_error * max_error)[0].tolist()
    assert len(inl) == score
    model, inl = refit_numpy(ra, rb, inl, min_inliers, max_error)
    if model is None:
        return out
    e = [math.sqrt(v) for v in residual2(model, ra[inl], rb[inl]).tolist()]
    total = e[0]
    for v in e[1:]:
        total = total + v
    L, t = model
    out["matrix"] = np.array([L[k] + [t[k]] for k in range(3)], np.float64)
    out["pairs"] = pairs[inl]
    out["errors"] = np.array([total / float(len(e)), max(e)], np.float64)
    return out


# ---- the raw call ------------------------------------------------------------------------------------------------------
SENTINEL = -7.0


class Outputs:
    """The outputs of mvn_register_beads, filled with a sentinel."""

    def __init__(self, cap):
        self.m = np.full(12, SENTINEL, np.float64)
        self.pairs = np.full((max(cap, 1), 2), int(SENTINEL), np.int32)
        self.err = np.full(2, SENTINEL, np.float64)
        self.nc, self.ni = C.c_int(int(SENTINEL)), C.c_int(int(SENTINEL))

    def untouched(self, counts=True):
        return (np.all(self.m == SENTINEL) and np.all(self.pairs == int(SENTINEL)) and np.all(self.err == SENTINEL)
                and (not counts or (self.nc.value == int(SENTINEL) and self.ni.value == int(SENTINEL))))


def dptr(x):
    return None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))


def register_raw(lib, a, na, b, nb, prm, o, device=-1, nulls=()):
    """mvn_register_beads as it stands: returns its return value; `nulls` names the arguments to pass as NULL."""
    args = {"a": dptr(a), "b": dptr(b), "prm": C.byref(prm) if prm is not None else None, "matrix_out": dptr(o.m),
            "num_candidates": C.byref(o.nc), "num_inliers": C.byref(o.ni),
            "pairs_out": o.pairs.ctypes.data_as(C.POINTER(C.c_int)), "errors_out": dptr(o.err)}
    for name in nulls:
        args[name] = None
    return lib.l.mvn_register_beads(int(device), args["a"], int(na), args["b"], int(nb), args["prm"], args["matrix_out"],
                                    args["num_candidates"], args["num_inliers"], args["pairs_out"], args["errors_out"],
                                    None)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- the checks --------------------------------------------------------------------------------------------------------
_SHARED = {}


def shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def sets_of(size):
    return shared(("sets", size), lambda: make_sets(*size))


def check_neighbours(lib, size):
    a, b, _ = sets_of(size)
    for p in (a, b):
        assert same_bits(lib.register_neighbours(p), neighbours_numpy(p)), size


def check_candidates(lib, size):
    a, b, _ = sets_of(size)
    want = shared(("cand", size), lambda: candidates_numpy(a, b))
    pairs, d = lib.register_candidates(a, b, RATIO)
    assert same_bits(pairs, want[0]) and same_bits(d, want[1]), (size, len(pairs), len(want[0]))


def check_registration(lib, size, hyps, prior=None, sets=None, key=None):
    a, b, _ = sets if sets is not None else sets_of(size)
    want = shared(("reg", key or size, hyps), lambda: register_numpy(a, b, hyps, prior=prior))
    o = Outputs(min(len(a), len(b)))
    prm = register_params(MAX_ERROR, RATIO, hyps, MIN_INLIERS, prior, 0)
    assert register_raw(lib, a, len(a), b, len(b), prm, o) == 0, lib.l.mvn_last_error()
    assert o.nc.value == want["nc"], (size, hyps, o.nc.value, want["nc"])
    if want["matrix"] is None:
        assert o.ni.value == 0 and o.untouched(counts=False)
        return want
    k = len(want["pairs"])
    assert o.ni.value == k, (size, hyps, o.ni.value, k)
    assert same_bits(o.pairs[:k], want["pairs"]) and np.all(o.pairs[k:] == int(SENTINEL))
    assert same_bits(o.m, want["matrix"].reshape(12)), (size, hyps, o.m, want["matrix"])
    assert same_bits(o.err, want["errors"]), (size, hyps, o.err, want["errors"])
    return want


def lstsq_matrix(a, b):
    X = np.concatenate([a, np.ones((len(a), 1))], axis=1)
    return np.linalg.lstsq(X, b, rcond=None)[0].T


def check_planted_truth(lib):
    a, b, true = make_sets(60, 48, 12, noise=0.05, seed=1)
    m, pairs, err = lib.register_beads(a, b, MAX_ERROR, RATIO, 512, MIN_INLIERS)
    assert m is not None
    print("planted truth: %d pairs, errors %s" % (len(pairs), err))
    assert np.all(true[pairs[:, 1]] == pairs[:, 0])
    assert len(pairs) >= 24, len(pairs)
    worst = np.abs(m - lstsq_matrix(a[pairs[:, 0]], b[pairs[:, 1]])).max()
    print("planted truth: against lstsq %.3g" % worst)
    assert worst <= 1e-9
    # without noise: every pair, and the truth itself
    a = separated_set(60)
    M = truth_matrix()
    a, b, true = make_sets(60, 60, 0, noise=0.0, seed=2, a=a, M=M)
    m, pairs, err = lib.register_beads(a, b, 1e-6, RATIO, 512, MIN_INLIERS)
    assert m is not None
    print("exact: %d pairs, errors %s, against the truth %.3g" % (len(pairs), err, np.abs(m - M).max()))
    assert len(pairs) == 60 and np.all(true[pairs[:, 1]] == pairs[:, 0])
    assert np.abs(m - M).max() <= 1e-9


def quarter_turn():
    """A rotation by 90 degrees about axis 0 through the box centre, and its inverse, as 3 x 4 matrices."""
    c = np.asarray([x / 2 for x in BOX])
    R = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    return (np.concatenate([R, (c - R @ c)[:, None]], axis=1), np.concatenate([R.T, (c - R.T @ c)[:, None]], axis=1))


def check_prior(lib):
    size = SIZES[1]
    a, b, true = sets_of(size)
    Q, Qinv = quarter_turn()
    turned = np.ascontiguousarray(apply(Qinv, a))  # the view as a stage turned by a quarter delivers it: Q turns it back
    plain = lib.register_beads(a, b, MAX_ERROR, RATIO, 512, MIN_INLIERS)
    with_prior = lib.register_beads(turned, b, MAX_ERROR, RATIO, 512, MIN_INLIERS, prior=Q)
    assert plain[0] is not None and with_prior[0] is not None
    assert np.array_equal(plain[1], with_prior[1])
    check_registration(lib, size, 512, prior=Q, sets=(turned, b, true), key="prior")


def check_no_model(lib):
    g = np.arange(3.0)
    lattice = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(27, 3))
    o = Outputs(27)
    prm = register_params(MAX_ERROR, RATIO, 64, MIN_INLIERS)
    before = lib.register_counters()
    assert register_raw(lib, lattice, 27, lattice, 27, prm, o) == 0
    assert o.nc.value == 0 and o.ni.value == 0 and o.untouched(counts=False)
    after = lib.register_counters()
    assert tuple(x - y for x, y in zip(after, before)) == (1, 0, 1)
    # a flat set against its shifted copy: every determinant is 0
    rng = np.random.default_rng(11)
    flat = rng.uniform(0.0, 1.0, (40, 3)) * np.asarray(BOX)
    flat[:, 0] = 12.0
    flat = np.ascontiguousarray(flat)
    moved = np.ascontiguousarray(flat + np.asarray(SHIFT))
    o = Outputs(40)
    assert register_raw(lib, flat, 40, moved, 40, prm, o) == 0
    assert o.nc.value > 0 and o.ni.value == 0 and o.untouched(counts=False), (o.nc.value, o.ni.value)
    assert tuple(x - y for x, y in zip(lib.register_counters(), after)) == (1, 1, 1)


def check_four_candidates(lib):
    """Five beads of which exactly four become candidates: every hypothesis is a permutation of the same four."""
    def build():
        for seed in range(1000):
            rng = np.random.default_rng([seed, 4])
            a = np.ascontiguousarray(rng.uniform(0.0, 1.0, (5, 3)) * np.asarray(BOX))
            b = np.ascontiguousarray(apply(truth_matrix(0.0, (1, 1, 1)), a))
            b[4] = b[4] + np.asarray([0.0, 25.0, -25.0])  # one bead moved: its descriptors change in both views
            if len(candidates_numpy(a, b)[0]) == 4:
                return a, b
        raise AssertionError("no set with four candidates")
    a, b = shared("four", build)
    pairs, _ = lib.register_candidates(a, b, RATIO)
    assert len(pairs) == 4 and same_bits(pairs, candidates_numpy(a, b)[0])
    for hyps in (1, 257):
        want = register_numpy(a, b, hyps)
        ra, rb = a[pairs[:, 0]], b[pairs[:, 1]]
        assert ransac_numpy(ra, rb, hyps, 0, MAX_ERROR) == (4, 0)
        check_registration(lib, (5, 5, 0), hyps, sets=(a, b, None), key="four")
        assert want["matrix"] is not None and len(want["pairs"]) == 4


def check_sample(lib):
    for n in (4, 5, 257, 65536):
        for h in (0, 1, 2 ** 24 - 1):
            for seed in (0, 12345678901234567890):
                got = lib.register_sample(seed, h, n).tolist()
                assert got == sample_numpy(seed, h, n), (n, h, seed, got)
                assert len(set(got)) == 4 and all(0 <= v < n for v in got)
    out = (C.c_int * 4)(-7, -7, -7, -7)
    assert lib.l.mvn_register_sample(0, 0, 3, out) < 0 and lib.l.mvn_register_sample(0, -1, 4, out) < 0
    assert lib.l.mvn_register_sample(0, 2 ** 24, 4, out) < 0 and lib.l.mvn_register_sample(0, 0, 4, None) < 0
    assert list(out) == [-7] * 4


def check_chunk_independence(lib):
    size = SIZES[4]
    a, b, _ = sets_of(size)
    base = lib.register_candidates(a, b, RATIO)
    assert len(base[0]) > 0
    for nb in (257, 513, 1025):
        k = nb - len(b)  # far away, and far from each other: they enter nobody's neighbourhood and match nothing
        far = 1e4 + 1e3 * np.arange(k, dtype=np.float64)[:, None] * np.asarray([1.0, 1.3, 1.7])
        padded = np.ascontiguousarray(np.concatenate([b, far]))
        got = lib.register_candidates(a, padded, RATIO)
        assert same_bits(got[0], base[0]) and same_bits(got[1], base[1]), nb


def render(shape, centres, sigma=1.5, amplitude=3000.0, base=100.0):
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    v = np.full(shape, base, np.float64)
    for c in centres:
        v += amplitude * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * sigma * sigma))
    return np.rint(v).astype(np.uint16)


def check_chain(lib):
    shape = (40, 64, 96)
    rng = np.random.default_rng(5)
    centres = []
    while len(centres) < 28:
        c = np.array([rng.uniform(7, s - 1 - 7) for s in shape])
        if all(np.abs(c - o).max() >= 9 for o in centres):
            centres.append(c)
    centres = np.array(centres)
    M = truth_matrix(1.5, (1.0, 1.01, 0.99), SHIFT, centre=[(s - 1) / 2 for s in shape])
    moved = apply(M, centres)
    inside = np.all((moved >= 7) & (moved <= np.asarray(shape) - 1 - 7), axis=1)
    q = 2.0 ** 0.25
    beads_a = lib.detect_beads(render(shape, centres), 1.5, 1.5 * q, 20.0)[0]
    beads_b = lib.detect_beads(render(shape, moved[inside]), 1.5, 1.5 * q, 20.0)[0]
    print("chain: %d and %d detections of %d and %d beads" % (len(beads_a), len(beads_b), 28, int(inside.sum())))
    m, pairs, err = lib.register_beads(beads_a, beads_b, 0.5, RATIO, 256, MIN_INLIERS)
    assert m is not None
    # a detection's planted centre: the nearest one
    ia = np.array([np.argmin(np.abs(centres - p).sum(1)) for p in beads_a])
    ib = np.array([np.argmin(np.abs(moved - p).sum(1)) for p in beads_b])
    assert np.all(ia[pairs[:, 0]] == ib[pairs[:, 1]])
    print("chain: %d inliers of %d, errors %s" % (len(pairs), int(inside.sum()), err))
    assert len(pairs) >= 20
    assert np.abs(m - lstsq_matrix(beads_a[pairs[:, 0]], beads_b[pairs[:, 1]])).max() <= 1e-9
    worst = np.sqrt(((apply(m, centres[inside]) - moved[inside]) ** 2).sum(1)).max()
    print("chain: worst distance of a planted centre %.4f" % worst)
    assert worst <= 0.5


def check_errors(lib):
    a, b, _ = sets_of(SIZES[1])
    good = dict(max_error=MAX_ERROR, ratio=RATIO, hypotheses=16, min_inliers=MIN_INLIERS)
    before = lib.register_counters()

    def refused(a_=a, na=None, b_=b, nb=None, nulls=(), device=-1, prior=None, flags=None, **kw):
        prm = register_params(**dict(good, **kw), prior=prior, flags=flags)
        o = Outputs(60)
        rc = register_raw(lib, a_, len(a_) if na is None else na, b_, len(b_) if nb is None else nb, prm, o, device, nulls)
        assert rc < 0 and o.untouched(), (nulls, kw, na, nb, rc)
        assert lib.l.mvn_last_error()

    for name in ("a", "b", "prm", "matrix_out", "num_candidates", "num_inliers"):
        refused(nulls=(name,))
    for n in (4, 0, -1, native.REGISTER_MAX_BEADS + 1):
        refused(na=n)
        refused(nb=n)
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy()
        x[17, 1] = bad
        refused(a_=x)
        refused(b_=np.ascontiguousarray(x[:len(b)]))
        T = np.eye(3, 4)
        T[2, 3] = bad
        refused(prior=T)
        refused(max_error=bad)
        refused(ratio=bad)
    refused(ratio=0.99)
    refused(max_error=0.0)
    refused(max_error=-1.0)
    refused(hypotheses=0)
    refused(hypotheses=native.REGISTER_MAX_HYPOTHESES + 1)
    refused(min_inliers=3)
    refused(flags=2)
    refused(flags=3, prior=np.eye(3, 4))
    refused(device=1000)
    assert lib.register_counters() == before
    # the optional outputs may be NULL; a non-finite prior without the flag is not read
    T = np.full((3, 4), np.nan)
    prm = register_params(**good, prior=T, flags=0)
    o = Outputs(60)
    assert register_raw(lib, a, len(a), b, len(b), prm, o, nulls=("pairs_out", "errors_out")) == 0
    assert o.ni.value > 0 and np.all(o.pairs == int(SENTINEL)) and np.all(o.err == SENTINEL) and np.all(o.m != SENTINEL)
    # the utilities
    idx = np.full((60, 4), -7, np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.l.mvn_register_neighbours(-1, dptr(a), 4, ip) < 0 and lib.l.mvn_register_neighbours(-1, None, 60, ip) < 0
    assert lib.l.mvn_register_neighbours(-1, dptr(a), 60, None) < 0 and np.all(idx == -7)
    need = C.c_size_t(5)
    assert lib.l.mvn_register_memory(4, 60, 1, C.byref(need)) < 0 and lib.l.mvn_register_memory(60, 60, 0, C.byref(need)) < 0
    assert lib.l.mvn_register_memory(60, 60, 1, None) < 0 and need.value == 5


def memory_model(na, nb):
    tiles = -(-nb // 64)
    c = min(tiles, -(-1024 // -(-na // 256)))
    chunk = 64 * -(-tiles // c)
    chunks = -(-nb // chunk)
    return 184 * (na + nb) + 12 * na * (chunks + 1) + 48 * min(na, nb) + 8


def check_memory(lib):
    for na, nb in ((5, 5), (60, 60), (300, 1025), (65536, 65536), (5, 65536), (65536, 5), (2000, 2000), (50000, 50000)):
        for hyps in (1, 100000):
            assert lib.register_memory(na, nb, hyps) == memory_model(na, nb), (na, nb)


def check_counters_and_timing(lib):
    a, b, _ = sets_of(SIZES[1])
    c0 = lib.register_counters()
    assert lib.register_beads(a, b, MAX_ERROR, RATIO, 16)[0] is not None
    c1 = lib.register_counters()
    assert tuple(x - y for x, y in zip(c1, c0)) == (1, 1, 1)
    lib.register_candidates(a, b)
    lib.register_neighbours(a)
    c2 = lib.register_counters()
    assert tuple(x - y for x, y in zip(c2, c1)) == (1, 0, 0)
    ms = lib.register_time(300, 200, 500, reps=2)
    assert len(ms) == 3 and all(x > 0 for x in ms), ms
    assert tuple(x - y for x, y in zip(lib.register_counters(), c2)) == (3, 3, 0)
    assert lib.l.mvn_register_time(0, 300, 200, 500, 0, (C.c_float * 3)()) < 0
    assert lib.l.mvn_register_time(0, 300, 200, 500, 1, None) < 0
