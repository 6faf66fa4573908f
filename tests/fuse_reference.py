"""Fusion (csrc/mvn_fuse.hpp, mvn_fuse_resampled in include/mvn_engine_api.h): what the tests on the emulation
(test_emu_fuse.py) and on the device (test_gpu_fuse.py) share - the numpy restatement of the arithmetic, the groups of
views, and the checks themselves, written once against a Binding.

Per output voxel, views in view order, everything float32:  t_v = w_v * s_v,  N = ((t_0 + t_1) + ...) + t_{V-1},
W = ((w_0 + w_1) + ...) + w_{V-1},  F = W > 0 ? N / W : fill;  a uint16 output stores
F >= 65535 ? 65535 : F > 0 ? rint(F) : 0.  numpy rounds every float32 array operation once and contracts nothing.
"""
import ctypes as C

import numpy as np

from libmultiviewnative_amd.abi import MVN_DEVICE, MVN_F32, MVN_HOST, MVN_U16, StackDesc, ViewGeometry, view_geometry
import resample_reference as rs

F = np.float32
FILLS = (0.0, 123.5)
RECORD_BYTES = 176  # per view: the table of mvn_fuse_memory_resampled (include/mvn_engine_api.h)


# ---- the definition -------------------------------------------------------------------------------------------------
def fuse_numpy(images, weights, fill):
    """F of the formula from the views' samples and unnormalised weights (float32 arrays), in view order"""
    images = [np.asarray(i, F) for i in images]
    weights = [np.asarray(w, F) for w in weights]
    with np.errstate(all="ignore"):
        N = weights[0] * images[0]
        W = weights[0].copy()
        for s, w in zip(images[1:], weights[1:]):
            N = N + w * s
            W = W + w
        assert N.dtype == F and W.dtype == F
        return np.where(W > 0, N / W, F(fill)).astype(F)


def to_uint16(f):
    with np.errstate(all="ignore"):
        return np.where(f >= F(65535), F(65535), np.where(f > 0, np.rint(f), F(0))).astype(np.uint16)


def as_output(f, dtype):
    return to_uint16(f) if dtype is np.uint16 else f


# ---- the groups -----------------------------------------------------------------------------------------------------
# a third geometry for the block of (10, 14, 70): planes z < 2 and columns x < 8 lie outside its raw stack, ramps behind them
THIRD = ((10, 14, 70), (6, 8, 9), [[0.5, 0, 0, -0.6], [0, 0.5, 0, 0.1], [0, 0, 0.11, -0.8]], (0, 0, 0), (1, 1.5, 1))
CASES = dict(rs.CASES, **{"third view": THIRD})
GROUPS = {
    "(3, 5, 7)": ("identity", "rotation by 30 degrees"),
    "(4, 6, 10)": ("integer shift", "rotation by 90 degrees with scale"),
    "(2, 3, 20)": ("fractional shift", "one raw plane"),
    "(10, 14, 70)": ("anisotropic scale", "rotation by 30 degrees across tiles"),
    "(10, 14, 70) x 3": ("anisotropic scale", "rotation by 30 degrees across tiles", "third view"),
}
MIXED = (np.uint16, np.float32, np.uint16)  # element type of view 0, 1, 2
TYPE_COMBINATIONS = {"mixed": MIXED, "uint16": (np.uint16,) * 3, "float32": (np.float32,) * 3}
OUT_LAYOUTS = ("dense", "window")


def block_of(group):
    return CASES[GROUPS[group][0]][0]


def raw_stack(name, dtype, view):
    shape = CASES[name][1]
    rng = np.random.default_rng(31 + 7 * view + sum(shape))
    if dtype is np.uint16:
        return rng.integers(100, 4000, shape).astype(np.uint16)
    return rng.uniform(100.0, 4000.0, shape).astype(F)


def geometry(name, hard_edges=False):
    block, raw, M, border, rng = CASES[name]
    return view_geometry(raw, M, border, (0, 0, 0) if hard_edges else rng)


def group_views(group, dtypes=MIXED, layout="dense", hard_edges=False):
    names = GROUPS[group]
    raws = [rs.laid_out(raw_stack(n, dt, v), layout) for v, (n, dt) in enumerate(zip(names, dtypes))]
    return raws, [geometry(n, hard_edges) for n in names]


def numpy_stacks(group, dtypes=MIXED, hard_edges=False):
    out = []
    for v, (n, dt) in enumerate(zip(GROUPS[group], dtypes)):
        block, raw, M, border, rng = CASES[n]
        out.append(rs.resample_numpy(raw_stack(n, dt, v), M, block, border, (0, 0, 0) if hard_edges else rng)[:2])
    return [o[0] for o in out], [o[1] for o in out]


def _check_groups():
    for group, names in GROUPS.items():
        assert len({CASES[n][0] for n in names}) == 1, group
        _, ws = numpy_stacks(group)
        W = ws[0].copy()
        for w in ws[1:]:
            W = W + w
        covered = float((W > 0).mean())
        both = float(((ws[0] > 0) & (ws[1] > 0)).mean())
        assert 0.5 <= covered < 1, (group, covered)
        assert both >= 0.05, (group, both)
        if len(names) == 3:  # the order of the sums is pinned where three views meet
            three = float(((ws[0] > 0) & (ws[1] > 0) & (ws[2] > 0)).mean())
            assert three >= 0.05, (group, three)
    assert any(len(n) == 3 for n in GROUPS.values())


_check_groups()


# ---- outputs --------------------------------------------------------------------------------------------------------
def new_output(block, dtype, layout):
    """(the array the library writes, the array that owns it) pre-filled with a value no fusion gives"""
    sentinel = 54321 if dtype is np.uint16 else F(-7.25)
    if layout == "dense":
        out = np.full(block, sentinel, dtype)
        return out, out
    big = np.full(tuple(s + 3 for s in block), sentinel, dtype)
    return big[1:1 + block[0], 2:2 + block[1], 1:1 + block[2]], big


def assert_output(win, big, want, what):
    assert np.array_equal(win, want, equal_nan=True), (what, int((win != want).sum()))
    if big is not win:  # the bytes outside the window are untouched
        ref = np.full(big.shape, big.flat[0], big.dtype)
        ref[1:1 + win.shape[0], 2:2 + win.shape[1], 1:1 + win.shape[2]] = want
        assert np.array_equal(big, ref, equal_nan=True), (what, "outside the window")


_STACKS = {}


def library_stacks(lib, group, dtypes, layout="dense"):
    """what mvn_resample_stack (pinned by the resample tests) makes of the views: images and unnormalised weights"""
    key = (id(lib), group, dtypes, layout)
    if key not in _STACKS:
        raws, geoms = group_views(group, dtypes, layout)
        out = [lib.resample_stack(r, g, block_of(group)) for r, g in zip(raws, geoms)]
        _STACKS[key] = ([o[0] for o in out], [o[1] for o in out])
    return _STACKS[key]


def fuse_direct(lib, out, raws, geoms, fill, out_location=MVN_HOST, raw_location=MVN_HOST):
    """mvn_fuse_resampled through ctypes with descriptors made by hand (location: what they claim)"""
    def desc(a, loc):
        d = StackDesc()
        d.dtype = MVN_U16 if a.dtype == np.uint16 else MVN_F32
        d.location = loc
        for k in range(3):
            d.stride[k] = a.strides[k] // a.itemsize
        return d
    n = len(raws)
    descs = (StackDesc * n)(*[desc(r, raw_location) for r in raws])
    ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
    garr = (ViewGeometry * n)(*geoms)
    od = desc(out, out_location)
    return lib.l.mvn_fuse_resampled(C.c_void_p(out.ctypes.data), C.byref(od), (C.c_int * 3)(*out.shape), n, ptrs, descs,
                                    garr, float(fill), None, 0)


# ---- 1. against the library's own resample pass ------------------------------------------------------------------------
def check_against_resample_pass(lib, group, out_dtype, fuse=None):
    """every fill, combination of element types, raw layout and output layout of a group; `fuse`: how the arrays reach
    the library (default: Binding.fuse_resampled on host arrays)"""
    fuse = fuse or (lambda out, raws, geoms, fill: lib.fuse_resampled(out, raws, geoms, fill))
    block = block_of(group)
    count = 0
    for combo, dtypes in TYPE_COMBINATIONS.items():
        for layout in rs.LAYOUTS:
            raws, geoms = group_views(group, dtypes, layout)
            images, ws = library_stacks(lib, group, dtypes, layout)
            for fill in FILLS:
                want = as_output(fuse_numpy(images, ws, fill), out_dtype)
                for out_layout in OUT_LAYOUTS:
                    win, big = new_output(block, out_dtype, out_layout)
                    fuse(win, raws, geoms, fill)
                    assert_output(win, big, want, (group, combo, layout, fill, out_layout))
                    count += 1
            if layout == "dense":
                f = fuse_numpy(images, ws, 123.5)
                assert (f == F(123.5)).any() and (f != F(123.5)).any(), group  # filled voxels, and fused ones
    return count


# ---- 2. against pure numpy: weights of exactly 0 or 1 ------------------------------------------------------------------
def check_against_numpy(lib, group, out_dtype):
    raws, geoms = group_views(group, hard_edges=True)
    images, ws = numpy_stacks(group, hard_edges=True)
    assert all(np.isin(w, (0, 1)).all() for w in ws)
    want = as_output(fuse_numpy(images, ws, 123.5), out_dtype)
    win, big = new_output(block_of(group), out_dtype, "dense")
    lib.fuse_resampled(win, raws, geoms, 123.5)
    assert_output(win, big, want, group)


# ---- 3. the uint16 rule ---------------------------------------------------------------------------------------------------
def check_uint16_rule(lib):
    group = "(10, 14, 70)"
    block = block_of(group)
    _, geoms = group_views(group)
    names = GROUPS[group]
    base = [raw_stack(n, np.float32, v) for v, n in enumerate(names)]
    nan = [b.copy() for b in base]
    nan[0][2, 3, 2:5] = np.nan
    for what, raws, seen in (
            ("beyond 65535", [b * F(40) for b in base], lambda f: (f > 65535).any() and ((f > 0) & (f < 65535)).any()),
            ("negative samples", [b - F(2000) for b in base], lambda f: (f < 0).any() and (f > 0).any()),
            ("a NaN sample", nan, lambda f: np.isnan(f).any() and (f > 0).any())):
        out = [lib.resample_stack(r, g, block) for r, g in zip(raws, geoms)]
        f = fuse_numpy([o[0] for o in out], [o[1] for o in out], 70000.0)
        assert seen(f), what
        win, big = new_output(block, np.uint16, "dense")
        lib.fuse_resampled(win, raws, geoms, 70000.0)  # (the fill is saturated by the same rule)
        assert_output(win, big, to_uint16(f), what)
        assert (win == 65535).any() and (win == 0).any() if what != "beyond 65535" else (win == 65535).any()
    # a fraction of exactly .5: two views through the identity with weights of exactly 1, values a and a + 1 (+ 2 ...)
    block, raw, M, _, _ = rs.CASES["identity"]
    g = view_geometry(raw, M, (0, 0, 0), (0, 0, 0))
    rng = np.random.default_rng(5)
    a = rng.integers(100, 4000, raw).astype(np.uint16)
    b = (a + rng.integers(0, 4, raw) * 2 + 1).astype(np.uint16)  # a + b is odd
    images, ws = zip(*[rs.resample_numpy(r, M, block)[:2] for r in (a, b)])
    f = fuse_numpy(images, ws, 0.0)
    half = (f % 1 == 0.5)
    assert half.any() and (np.floor(f[half]) % 2 == 0).any() and (np.floor(f[half]) % 2 == 1).any()
    win, big = new_output(block, np.uint16, "dense")
    lib.fuse_resampled(win, [a, b], [g, g], 0.0)
    assert_output(win, big, to_uint16(f), "ties")
    assert (win[half] % 2 == 0).all()  # ties went to even


# ---- 4. psi start ---------------------------------------------------------------------------------------------------------
PSI_FILL = 300.0


def with_psi_start(lib, mode, fill, fn):
    lib.set_psi_start(mode, fill)
    try:
        return fn()
    finally:
        lib.set_psi_start(0, 0.0)


def garbage(block):
    g = np.full(block, np.nan, F)
    g[::2] = F(-1e30)
    return g


def fused_start(lib, c, weights, fill=PSI_FILL):
    """psi0 of the restatement on the library's own stacks: the caller's weights, or (None) the unnormalised computed"""
    images, ws = rs.library_stacks(lib, c)
    return fuse_numpy(images, ws if weights is None else weights, fill)


def check_psi_start(lib, key, pad_mode, weights_mode):
    c = rs.make_call(key)
    weights = None if weights_mode == 1 else c["w"]
    psi0 = fused_start(lib, c, weights)
    if weights_mode == 1:
        assert (psi0 == F(PSI_FILL)).any()
        out = np.empty(c["block"], F)
        lib.fuse_resampled(out, c["raws"], c["geoms"], PSI_FILL)
        assert np.array_equal(out, psi0), "the two kernels disagree"
    lib.check(lib.l.mvn_release_cached_engines())
    c0 = lib.fuse_counters()
    want = rs.resampled_call(lib, dict(c, psi0=psi0), pad_mode, weights=weights)
    c1 = lib.fuse_counters()
    assert c1 == c0, "psi start 0 launched a fusion"
    got = with_psi_start(lib, 1, PSI_FILL, lambda: rs.resampled_call(lib, c, pad_mode, weights=weights,
                                                                      psi=garbage(c["block"])))
    c2 = lib.fuse_counters()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (0, 1), (c1, c2)
    assert np.isfinite(got).all() and not np.array_equal(got, psi0)
    assert np.array_equal(got, want), (key, pad_mode, weights_mode, int((got != want).sum()))
    lib.check(lib.l.mvn_release_cached_engines())


def check_psi_start_block_after_block(lib, location=None):
    """two blocks cut from the same raw stacks on a cached engine, the switch on, off and on again"""
    c = rs.make_call("even block")
    lib.check(lib.l.mvn_release_cached_engines())
    for shift, start in (((0, 0, 0), 1), ((1, 2, 3), 0), ((1, 2, 3), 1), ((0, 0, 0), 1)):
        geoms = []
        for n in c["names"]:
            block, raw, M, border, rng = rs.CASES[n]
            M = np.asarray(M, np.float64).copy()
            M[:, 3] = M[:, 3] + M[:, :3] @ np.asarray(shift, np.float64)
            geoms.append(view_geometry(raw, M, border, rng))
        cb = dict(c, geoms=geoms)
        psi0 = fused_start(lib, cb, None)
        if start == 1:
            got = with_psi_start(lib, 1, PSI_FILL, lambda: rs.resampled_call(lib, cb, "zero", psi=garbage(c["block"]),
                                                                              location=location))
        else:
            got = rs.resampled_call(lib, dict(cb, psi0=psi0), "zero", location=location)
        images, ws = rs.library_stacks(lib, cb)
        want = rs.plain_call(lib, dict(cb, psi0=psi0), images, rs.normalize_numpy(ws), "zero")
        assert np.array_equal(got, want), (shift, start)
    lib.check(lib.l.mvn_release_cached_engines())


def check_psi_start_composition(lib):
    """with acceleration, TV, background and statistics, as resample_reference.check_composition"""
    c = rs.make_call("odd block", seed=17)
    psi0 = fused_start(lib, c, None)
    lam, iters = 0.01, 4
    lib.check(lib.l.mvn_release_cached_engines())
    lib.set_acceleration(1)
    lib.set_regularization(1, 1.0)
    lib.set_background([3.0, 2.0])
    lib.set_convergence(0.0)
    try:
        want = rs.resampled_call(lib, dict(c, psi0=psi0), "zero", lam=lam, iters=iters)
        run_w, rows_w = lib.last_convergence()
        got = with_psi_start(lib, 1, PSI_FILL, lambda: rs.resampled_call(lib, c, "zero", lam=lam, iters=iters,
                                                                          psi=garbage(c["block"])))
        run_g, rows_g = lib.last_convergence()
    finally:
        lib.set_convergence(-1)
        lib.set_background(None)
        lib.set_regularization(0)
        lib.set_acceleration(0)
        lib.check(lib.l.mvn_release_cached_engines())
    assert np.array_equal(got, want)
    assert run_g == run_w == iters and np.array_equal(rows_g, rows_w)
    plain = rs.resampled_call(lib, dict(c, psi0=psi0), "zero", lam=lam, iters=iters)
    assert not np.array_equal(got, plain)  # the switches act
    lib.check(lib.l.mvn_release_cached_engines())


# ---- 5. the engine API ------------------------------------------------------------------------------------------------
def check_engine_api(lib):
    c = rs.make_call("even block")
    want = np.empty(c["block"], F)
    lib.fuse_resampled(want, c["raws"], c["geoms"], PSI_FILL)
    e = lib.engine(c["block"], 2)
    try:
        for v in range(2):
            e.set_view_resampled(v, c["raws"][v], c["geoms"][v], c["k1"][v], c["k2"][v])
        e.set_psi(garbage(c["block"]))
        before = lib.fuse_counters()
        e.fuse_psi(PSI_FILL)
        assert lib.fuse_counters()[1] - before[1] == 1
        assert np.array_equal(e.get_psi(), want)
        try:
            e.fuse_psi(float("inf"))
        except Exception as err:
            assert "fill" in str(err)
        else:
            raise AssertionError("a non-finite fill was taken")
        assert np.array_equal(e.get_psi(), want)
    finally:
        e.close()


def check_engine_refusals(lib):
    """a halo hook and a uint16 image volume (an engine with streamed views is made by the memory planner of the
    blocking calls only: the engine API cannot reach that refusal)"""
    c = rs.make_call("even block")
    images, ws = rs.library_stacks(lib, c)
    for what in ("halo", "uint16"):
        e = lib.engine(c["block"], 2)
        try:
            if what == "uint16":
                lib.set_image_storage(1)
            try:
                for v in range(2):
                    image = np.rint(images[v]).astype(np.uint16) if what == "uint16" else images[v]
                    e.set_view(v, image, ws[v], c["k1"][v], c["k2"][v])
            finally:
                lib.set_image_storage(0)
            e.set_psi(c["psi0"])
            if what == "halo":
                e.set_halo_hook(lambda spectrum, view, conv: None)
            before = lib.fuse_counters()
            try:
                e.fuse_psi(1.0)
            except Exception as err:
                assert what in str(err), str(err)
            else:
                raise AssertionError("an engine with %s fused into psi" % what)
            assert lib.fuse_counters() == before
            assert np.array_equal(e.get_psi(), c["psi0"]), what
        finally:
            e.close()


# ---- 6. errors, memory, counters ----------------------------------------------------------------------------------------
def check_errors(lib):
    group = "(4, 6, 10)"
    block = block_of(group)
    raws, geoms = group_views(group)

    def bad_matrix():
        blk, raw, M, border, rng = CASES[GROUPS[group][1]]
        M = np.asarray(M, np.float64).copy()
        M[1, 2] = float("inf")
        return view_geometry(raw, M, border, rng)

    def refused(what, rc, out, ref):
        assert rc < 0 and lib.l.mvn_last_error().decode(), what
        assert np.array_equal(out, ref), what

    for dtype in (np.float32, np.uint16):
        out, _ = new_output(block, dtype, "dense")
        ref = out.copy()
        refused("no views", fuse_direct(lib, out, [], [], 0.0), out, ref)
        assert "num_views" in lib.l.mvn_last_error().decode()
        refused("a non-finite matrix entry", fuse_direct(lib, out, raws, [geoms[0], bad_matrix()], 0.0), out, ref)
        refused("a NaN fill", fuse_direct(lib, out, raws, geoms, float("nan")), out, ref)
        refused("an infinite fill", fuse_direct(lib, out, raws, geoms, float("inf")), out, ref)
        assert "fill" in lib.l.mvn_last_error().decode()
        od = StackDesc()
        od.dtype = MVN_U16 if dtype is np.uint16 else MVN_F32
        od.stride[0], od.stride[1], od.stride[2] = block[1] * block[2], -block[2], 1
        n = len(raws)
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
        rc = lib.l.mvn_fuse_resampled(C.c_void_p(out.ctypes.data), C.byref(od), (C.c_int * 3)(*block), n, ptrs, None,
                                      None, 0.0, None, 0)
        refused("a NULL geom", rc, out, ref)
        assert "geom" in lib.l.mvn_last_error().decode()
        descs = (StackDesc * n)()
        for v, r in enumerate(raws):
            descs[v].dtype = MVN_U16 if r.dtype == np.uint16 else MVN_F32
            for k in range(3):
                descs[v].stride[k] = r.strides[k] // r.itemsize
        rc = lib.l.mvn_fuse_resampled(C.c_void_p(out.ctypes.data), C.byref(od), (C.c_int * 3)(*block), n, ptrs, descs,
                                      (ViewGeometry * n)(*geoms), 0.0, None, 0)
        refused("a negative stride on out", rc, out, ref)
        assert "stride" in lib.l.mvn_last_error().decode()
    # the switch: a mode of 2 and a non-finite fill leave it as it was; a refused call leaves psi untouched
    lib.set_psi_start(1, 2.5)
    try:
        assert lib.l.mvn_set_psi_start(2, 0.0) < 0 and "mode" in lib.l.mvn_last_error().decode()
        assert lib.l.mvn_set_psi_start(0, float("nan")) < 0 and "fill" in lib.l.mvn_last_error().decode()
        assert lib.get_psi_start() == (1, 2.5)
        c = rs.make_call("even block")
        psi = c["psi0"].copy()
        call = lib.resample_call(psi, c["raws"], [c["geoms"][0], bad_matrix()], c["k1"], c["k2"], 0.006, rs.MINV, 3)
        before = lib.fuse_counters()
        rc = lib.l.mvn_deconvolve_resampled(C.c_void_p(call.psi_ptr), call.ws, C.byref(call.desc), call.geom, 1, 0)
        assert rc < 0 and lib.l.mvn_last_error().decode()
        assert np.array_equal(psi, c["psi0"]) and lib.fuse_counters() == before
    finally:
        lib.set_psi_start(0, 0.0)
    assert lib.get_psi_start() == (0, 0.0)


def check_memory(lib):
    """host stacks as they are; device memory by descriptors made by hand (nothing is read through them)"""
    group = "(4, 6, 10)"
    block = block_of(group)
    voxels = int(np.prod(block))
    raws, geoms = group_views(group)
    table = RECORD_BYTES * len(raws)
    for dtype in (np.float32, np.uint16):
        for layout in OUT_LAYOUTS:
            win, _ = new_output(block, dtype, layout)
            need = lib.fuse_memory(win, raws, geoms)
            assert need == table + voxels * win.itemsize + sum(r.nbytes for r in raws), (dtype, layout, need)
    one = [np.broadcast_to(r.dtype.type(5), r.shape) for r in raws]
    win, _ = new_output(block, np.float32, "dense")
    assert lib.fuse_memory(win, one, geoms) == table + voxels * 4 + sum(r.itemsize for r in raws)

    def described(out_loc, raw_loc):
        def desc(a, loc):
            d = StackDesc()
            d.dtype = MVN_U16 if a.dtype == np.uint16 else MVN_F32
            d.location = loc
            for k in range(3):
                d.stride[k] = a.strides[k] // a.itemsize
            return d
        n = len(raws)
        need = C.c_size_t(0)
        lib.check(lib.l.mvn_fuse_memory_resampled(C.byref(desc(win, out_loc)), (C.c_int * 3)(*block), n,
                                                  (StackDesc * n)(*[desc(r, raw_loc) for r in raws]),
                                                  (ViewGeometry * n)(*geoms), 0, C.byref(need)))
        return need.value
    assert described(MVN_DEVICE, MVN_DEVICE) == table  # an all-device call: the table of the views' records alone
    assert described(MVN_HOST, MVN_DEVICE) == table + voxels * 4
    assert described(MVN_DEVICE, MVN_HOST) == table + sum(r.nbytes for r in raws)


def check_counters_and_timing(lib):
    group = "(10, 14, 70)"
    _, geoms = group_views(group)
    for u16 in (False, True):
        before, rbefore = lib.fuse_counters(), lib.resample_counters()
        ms = lib.fuse_time(geoms, block_of(group), u16=u16, reps=2)
        print("fuse_time (u16 = %s): %r" % (u16, ms))
        assert len(ms) == 3 and all(m > 0 for m in ms), ms
        after = lib.fuse_counters()
        assert (after[0] - before[0], after[1] - before[1]) == (3, 0)  # reps + 1 passes
        assert lib.resample_counters()[0] - rbefore[0] == 3 * len(geoms)
    raws, geoms = group_views(group)
    win, _ = new_output(block_of(group), np.float32, "dense")
    before = lib.fuse_counters()
    lib.fuse_resampled(win, raws, geoms, 0.0)
    after = lib.fuse_counters()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0)
