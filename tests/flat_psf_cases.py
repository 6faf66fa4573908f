"""Inputs under which EVERY tap of a PSF counts, for the direct dim0 leg (csrc/mvn_dim0_direct.hpp, kd_dim0<K>) and the
fused middle pass (csrc/mvn_mid_fused.hpp, kf_mid<K>): shared by tests/test_emu_flat_psf.py, the -m gpu twin
tests/test_gpu_flat_psf.py, tests/test_flat_psf_inputs.py and the fuzz tools.

The Gaussian PSFs of ref_fixtures.py have outer coefficients of 1e-6 .. 1e-13 of their peak at 31 taps: a kernel that drops
or misplaces them stays far inside 1e-5 of the maximum.  Here every PSF coefficient is uniform in [0.5, 1.5] before the
PSF is normalised, kernel2 is drawn independently of kernel1 (not its flip), and views and psi0 are white (uniform in
[50, 150]: every bin of the dim1 and dim2 transforms is populated).  Zeroing ONE tap plane then moves the float64 result by
about 1e-2 of its maximum (test_flat_psf_inputs.py asserts MIN_TAP_EFFECT).

Reference: the float64 restatement (numpy_restatement.py).  Bound: no absolute number - the C oracle (a float32 pipeline
of the same length) runs on the same inputs, d_orc is its max-abs distance to the float64 result over max |ref|, and the
kernel under test must lie within BOUND_FACTOR * d_orc (FMA contraction and another summation order).  Beside it:
BOUND_FACTOR * d_orc <= 1e-5 (the project's bound) and <= MIN_TAP_EFFECT / 100, so the bound can never hide a lost tap."""
import os

import numpy as np

from libmultiviewnative_amd.abi import WorkspaceHolder
from libmultiviewnative_amd.native import MvnError
import numpy_restatement as nr

try:  # (same transforms, threaded; numpy's where scipy is not installed)
    import scipy.fft as _fft
    _FFT_KW = {"workers": min(8, os.cpu_count() or 1)}
except ImportError:  # pragma: no cover
    _fft, _FFT_KW = np.fft, {}

MIN_VALUE = 1e-4
BOUND_FACTOR = 4.0
PROJECT_BOUND = 1e-5
MIN_TAP_EFFECT = 1e-3  # of max |ref|: least change of the float64 result when one tap plane is zeroed (asserted on the CPU)
ORC_THREADS = 8


# ---- inputs ---------------------------------------------------------------------------------------------------------
def flat_psf(rng, kshape):
    k = rng.uniform(0.5, 1.5, kshape)
    return (k / k.sum()).astype(np.float32)


def flat_inputs(shape, kshape, nviews=2, seed=0, kshape2=None):
    """views, kernels1, kernels2, weights (1 / nviews), psi0 - seeded."""
    rng = np.random.default_rng(seed)
    views = [rng.uniform(50.0, 150.0, shape).astype(np.float32) for _ in range(nviews)]
    k1 = [flat_psf(rng, kshape) for _ in range(nviews)]
    k2 = [flat_psf(rng, kshape2 or kshape) for _ in range(nviews)]
    w = np.full(shape, 1.0 / nviews, np.float32)
    psi0 = rng.uniform(50.0, 150.0, shape).astype(np.float32)
    return views, k1, k2, [w] * nviews, psi0


def one_hot_inputs(shape, k, t1, t2, seed=0):
    """One view, weights 1: kernel1 is 1 at tap t1 of a (k, 1, 1) PSF, kernel2 is 1 at tap t2."""
    rng = np.random.default_rng(seed)
    view = rng.uniform(50.0, 150.0, shape).astype(np.float32)
    psi0 = rng.uniform(50.0, 150.0, shape).astype(np.float32)
    k1, k2 = np.zeros((k, 1, 1), np.float32), np.zeros((k, 1, 1), np.float32)
    k1[t1], k2[t2] = 1.0, 1.0
    return [view], [k1], [k2], [np.ones(shape, np.float32)], psi0


def one_hot_reference(inputs, k, t1, t2):
    """lambda 0, one iteration, in float64: psi0 * roll(view / roll(psi0, t1 - k // 2), t2 - k // 2) along dim0."""
    views, _, _, _, psi0 = inputs
    p = psi0.astype(np.float64)
    return p * np.roll(views[0].astype(np.float64) / np.roll(p, t1 - k // 2, 0), t2 - k // 2, 0)


def one_hot_taps(k):
    """(t1, t2) of the probes: the first and last tap of every batch of 8, the first two and the last two."""
    return [(t, k - 1 - t) for t in sorted({0, 1, 7, 8, 15, 16, 23, 24, k - 2, k - 1}) if 0 <= t < k]


# ---- references -----------------------------------------------------------------------------------------------------
def float64_deconvolve(psi, views, k1s, k2s, weights, lam, min_value, iterations, simultaneous=False):
    """numpy_restatement.deconvolve with threaded transforms (same operations in the same order, float64)."""
    psi = psi.astype(np.float64).copy()
    shape, ax = psi.shape, (0, 1, 2)
    fwd = lambda x: _fft.rfftn(x, axes=ax, **_FFT_KW)
    inv = lambda x: _fft.irfftn(x, s=shape, axes=ax, **_FFT_KW)
    s1 = [fwd(nr.wrapped_insert(k, shape)) for k in k1s]
    s2 = [fwd(nr.wrapped_insert(k, shape)) for k in k2s]
    for _ in range(iterations):
        base = psi.copy()
        acc = np.zeros_like(psi)
        for v in range(len(views)):
            src = base if simultaneous else psi
            blurred = inv(fwd(src) * s1[v])
            with np.errstate(divide="ignore", invalid="ignore"):
                q = views[v].astype(np.float64) * (1.0 / blurred)
            integral = inv(fwd(q) * s2[v])
            new = nr.update(src, integral, weights[v].astype(np.float64), lam, min_value)
            if simultaneous:
                acc += new - src
            else:
                psi = new
        if simultaneous:
            psi = base + acc
    return psi


_REFS = {}


def references(inputs, lam, iterations, simultaneous=False, key=None):
    """(float64 result, d_orc) for these inputs: d_orc = max |oracle - ref| / max |ref| of the C oracle (float32, the
    sequential sweep or its simultaneous twin).  Small results are kept under `key`, shared by the forms of one case, and
    never written to."""
    if key is not None and key in _REFS:
        return _REFS[key]
    from oracle import binding as orc
    views, k1, k2, w, psi0 = inputs
    ref = float64_deconvolve(psi0, views, k1, k2, w, lam, MIN_VALUE, iterations, simultaneous)
    h = WorkspaceHolder(views, k1, k2, w, lam, MIN_VALUE, iterations)
    o = (orc.cpu_deconvolve_simultaneous if simultaneous else orc.cpu_deconvolve)(psi0, h, ORC_THREADS)
    out = (ref, distance(o, ref))
    if key is not None and ref.nbytes <= (4 << 20):
        ref.setflags(write=False)
        _REFS[key] = out
    return out


def oracle_distance(inputs, ref, lam=0.0, iterations=1):
    """d_orc against a float64 result computed elsewhere (the closed form of the one-hot probes)."""
    from oracle import binding as orc
    views, k1, k2, w, psi0 = inputs
    return distance(orc.cpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, lam, MIN_VALUE, iterations), ORC_THREADS), ref)


def distance(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def check(got, ref, d_orc, what, failures=None):
    """The bound rule of this module's docstring; prints both distances.  With a list, a miss of the kernel is appended
    to it (a test that loops over PSF depths reports every failing one); the two conditions on the bound itself always
    assert."""
    d_got = distance(got, ref) if np.isfinite(got).all() else float("inf")
    bound = BOUND_FACTOR * d_orc
    print("%s: got %.3g, d_orc %.3g (%.2f x)" % (what, d_got, d_orc, d_got / d_orc if d_orc > 0 else float("inf")))
    assert bound <= PROJECT_BOUND, (what, d_orc)
    assert bound <= MIN_TAP_EFFECT / 100.0, (what, d_orc)
    if d_got <= bound:
        return d_got
    if failures is None:
        raise AssertionError("%s: %.3g from float64, oracle %.3g, bound %.3g" % (what, d_got, d_orc, bound))
    failures.append("%s: %.3g from float64, oracle %.3g" % (what, d_got, d_orc))
    return d_got


def run_abi(binding, inputs, lam, iterations):
    views, k1, k2, w, psi0 = inputs
    return binding.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, lam, MIN_VALUE, iterations))


def run_simultaneous(binding, inputs, lam, iterations, chunks=0):
    """The simultaneous loop on a resident engine through compute_delta / apply_delta, or (chunks > 0) its chunked form."""
    views, k1, k2, w, psi0 = inputs
    e = binding.engine(psi0.shape, len(views))
    try:
        for v in range(len(views)):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        n = e.delta_chunks(chunks) if chunks else 0
        for _ in range(iterations):
            if chunks:
                e.compute_delta_head(lam, MIN_VALUE)
                for c in range(n):
                    e.compute_delta_chunk(c, n)
                for c in range(n):
                    e.apply_delta_chunk(c, n, True)
            else:
                e.compute_delta(lam, MIN_VALUE)
                e.apply_delta()
        return e.get_psi()
    finally:
        e.close()


def dim0_kinds(binding, inputs, lam=0.0):
    """Which dim0 kernels one sweep of a resident engine launches under the switches in force (the engine's profile):
    {'axis0_direct': n, 'axis0_fused': n, 'mid_fused': n, ...} with the kinds that ran."""
    views, k1, k2, w, psi0 = inputs
    e = binding.engine(psi0.shape, len(views))
    try:
        for v in range(len(views)):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        e.profile(True)
        e.iterate(1, lam, MIN_VALUE)
        e.sync()
        return {k: n for k, (_, n) in e.profile_read().items() if n > 0 and (k.startswith("axis0") or k == "mid_fused")}
    finally:
        e.close()


# ---- the direct dim0 leg --------------------------------------------------------------------------------------------
DIRECT_DEPTHS = list(range(1, 34))  # every PSF depth the leg takes; even k runs the K = k | 1 template, a zero tap appended
PLANES = [(6, 8), (9, 15), (16, 32)]  # (d1, d2): odd d2 and odd d1 occur
SWEEPS = 2


def piece_len(k, d0, plane, want):
    """mvn_dim0_piece_len (csrc/mvn_dim0_direct.hpp): output planes per piece of a column, 0 = whole columns."""
    if plane >= want or plane < 1:
        return 0
    pieces = min(-(-want // plane), d0 // (2 * (k | 1) + 8))
    return 0 if pieces < 2 else -(-d0 // pieces)


def bins_per_plane(d1, d2):
    """Layout::C bins per row (csrc/mvn_plan.hpp) times d1 - what Engine::dim0_conv passes as `plane`, in the packed and
    in the split layout alike: the split layout's Nyquist bins are a plane of their own (plane2), cut by seg2."""
    return d1 * (d2 // 2 if d2 % 2 == 0 else (d2 + 1) // 2)


def direct_cases(k, form="columns"):
    """[(shape, kshape, lam, seed)] of PSF depth k.  'columns': d0 at the minimum (k | 1) + 4 and at a larger odd value
    (no multiple of 8).  'pieces': d0 of two and of three pieces of the shortest length, 2 (k | 1) + 8, plus a remainder
    so that the last piece is shorter.  'slabs2' / 'slabs3': even d2, every slab of at least k // 2 planes and deep
    enough for the template with its halos, the slabs unequal."""
    K = k | 1
    if form == "pieces":
        d0s = [2 * (2 * K + 8) + 1, 3 * (2 * K + 8) + 5]
    elif form in ("slabs2", "slabs3"):
        P = int(form[-1])
        d0s = [P * max(5, k // 2) + 1, P * max(5, k // 2) + 12]
    else:
        d0s = [K + 4, K + 4 + 12 + (k % 3) * 2]  # (K is odd: the second one too)
    out = []
    for i, d0 in enumerate(d0s):
        d1, d2 = PLANES[(k + i) % 3]
        if form.startswith("slabs") and d2 % 2:
            d1, d2 = PLANES[(k + i + 1) % 3]
        kshape = (k, (1, 3)[(k + i) % 2], 1 + (k + i) % 3)
        out.append(((d0, d1, d2), kshape, 0.006 if (k + i) % 2 else 0.0, 9000 + 10 * k + i))
    return out


STAGGER_PLANES = [(24, 50), (17, 63)]  # 600 and 544 bins: three workgroups of 256, which start at planes 0, 7 and 14
                                       # (the planes above are one workgroup each: MVN_D0_STAGGER would do nothing)
PIECES_WANT = 4096  # MVN_DIM0_DIRECT_MIN_PLANE of the pieces forms: 16 .. 171 pieces wanted, the minimum length decides

# form: (switches, case family, dim0 kernel kind that must run)
DIRECT_FORMS = {
    "product defaults": ({}, "columns", "axis0_direct"),
    "split nyquist": ({"MVN_NYQ_PACKED": "0"}, "columns", "axis0_direct"),
    "whole columns": ({"MVN_DIM0_DIRECT_MIN_PLANE": "0"}, "pieces", "axis0_direct"),  # long columns, walked whole
    "pieces": ({"MVN_DIM0_DIRECT_MIN_PLANE": str(PIECES_WANT)}, "pieces", "axis0_direct"),
    "pieces split": ({"MVN_DIM0_DIRECT_MIN_PLANE": str(PIECES_WANT), "MVN_NYQ_PACKED": "0"}, "pieces", "axis0_direct"),
    "stagger 7": ({"MVN_D0_STAGGER": "7", "MVN_DIM0_DIRECT_MIN_PLANE": "0"}, "stagger", "axis0_direct"),
    "two slabs": ({"MVN_DEVICES": "0,0"}, "slabs2", "axis0_direct"),
    "three slabs": ({"MVN_DEVICES": "0,0,0"}, "slabs3", "axis0_direct"),
    "fft dim0": ({"MVN_DIM0_DIRECT": "0"}, "columns", "axis0_fused"),  # the same inputs through the fused FFT dim0 pass
}
SIMULTANEOUS_DEPTHS = [2, 15, 32, 33]
DIRECT_ONE_HOT = [32, 33]


def _form_cases(k, family):
    if family != "stagger":
        return direct_cases(k, family)
    return [((s[0], ) + STAGGER_PLANES[(k + i) % 2], ks, lam, seed + 5)
            for i, (s, ks, lam, seed) in enumerate(direct_cases(k, "columns"))]


def direct_form(binding, monkeypatch, form, tag):
    """Every PSF depth in one form of the leg (the caller has removed the suite's pins, set MVN_PAD_MODE=none and drops
    the cached engines); every failing depth is reported."""
    env, family, kind = DIRECT_FORMS[form]
    devices = env.get("MVN_DEVICES")
    for kk, vv in env.items():
        if kk != "MVN_DEVICES":
            monkeypatch.setenv(kk, vv)
    binding.l.mvn_release_cached_engines()
    failures, worst = [], (0.0, 0.0)
    for k in DIRECT_DEPTHS:
        if devices and k // 2 < 1:
            continue  # (slabs exchange k // 2 halo planes: a one-plane PSF has none and runs on one device)
        for shape, kshape, lam, seed in _form_cases(k, family):
            inputs = flat_inputs(shape, kshape, 2, seed)
            what = "%s [%s] k %d %s psf %s lam %g" % (tag, form, k, shape, kshape, lam)
            # the form, from what an engine launches and from the plan's rule for pieces (slabs: the call counts as
            # a multi-device one only if every slab's engine takes the direct leg, HaloGroup::all_direct)
            if not devices:
                kinds = dim0_kinds(binding, inputs, lam)
                other = {"axis0_direct": "axis0_fused", "axis0_fused": "axis0_direct"}[kind]
                assert kinds.get(kind, 0) == 2 * 2 and other not in kinds and "mid_fused" not in kinds, (what, kinds)
                plen = piece_len(k, shape[0], bins_per_plane(shape[1], shape[2]),
                                 int(env.get("MVN_DIM0_DIRECT_MIN_PLANE", 131072)))
                if form.startswith("pieces"):
                    assert 0 < plen < shape[0], (what, plen)
                elif kind == "axis0_direct":
                    assert plen == 0, (what, plen)
            ref, d_orc = references(inputs, lam, SWEEPS, key=(shape, kshape, lam, seed, False))
            if devices:
                monkeypatch.setenv("MVN_DEVICES", devices)
                try:
                    before = binding.l.mvn_multi_device_calls()
                    got = run_abi(binding, inputs, lam, SWEEPS)
                    assert binding.l.mvn_multi_device_calls() == before + 1, what  # (no fall-back to one device)
                finally:
                    monkeypatch.delenv("MVN_DEVICES", raising=False)
            else:
                got = run_abi(binding, inputs, lam, SWEEPS)
            d = check(got, ref, d_orc, what, failures)
            if d_orc > 0 and (worst[1] == 0 or d / d_orc > worst[0] / worst[1]):
                worst = (d, d_orc)
    binding.l.mvn_release_cached_engines()
    print("%s [%s] worst: got %.3g at d_orc %.3g" % (tag, form, worst[0], worst[1]))
    assert not failures, "\n".join(failures)


def direct_simultaneous(binding, k, tag):
    failures = []
    for shape, kshape, lam, seed in direct_cases(k, "columns") + direct_cases(k, "pieces"):
        inputs = flat_inputs(shape, kshape, 2, seed)
        kinds = dim0_kinds(binding, inputs, lam)
        assert kinds.get("axis0_direct", 0) == 4 and "axis0_fused" not in kinds, kinds
        ref, d_orc = references(inputs, lam, SWEEPS, True, key=(shape, kshape, lam, seed, True))
        check(run_simultaneous(binding, inputs, lam, SWEEPS), ref, d_orc,
              "%s [simultaneous] k %d %s psf %s lam %g" % (tag, k, shape, kshape, lam), failures)
    assert not failures, "\n".join(failures)


def direct_one_hot(binding, k, tag):
    """Every tap of a k-plane PSF on its own, t2 = k - 1 - t1, on the shallowest volume the template takes."""
    failures = []
    shape = ((k | 1) + 4, 6, 8)
    for t1 in range(k):
        t2 = k - 1 - t1
        inputs = one_hot_inputs(shape, k, t1, t2, seed=8000 + 40 * k + t1)
        if t1 in (0, k - 1):
            kinds = dim0_kinds(binding, inputs)
            assert kinds.get("axis0_direct", 0) == 2 and "axis0_fused" not in kinds, kinds
        ref = one_hot_reference(inputs, k, t1, t2)
        check(run_abi(binding, inputs, 0.0, 1), ref, oracle_distance(inputs, ref),
              "%s one-hot k %d taps %d / %d" % (tag, k, t1, t2), failures)
    assert not failures, "\n".join(failures)


# ---- the fused middle pass ------------------------------------------------------------------------------------------
MID_DEPTHS_GPU = list(range(1, 32))
MID_DEPTHS_EMU = [1, 2, 8, 9, 16, 17, 24, 25, 31]
MID_WIDE = ((16, 512, 512), (9, 31, 31))  # a PSF that is wide across the plane
MID_ONE_HOT = [31, 16]


def mid_d0(k):
    """Planes of the (d0, 512, 512) volume of depth k: the wrap and the loop's exits vary with k.  (Volumes of fewer than
    (k | 1) + 4 planes keep the transform along dim0.)"""
    return (k | 1) + 4 + (k % 5)


# One tap on 5 .. 7 planes: a walk of d0 + K - 1 < 8 steps, shorter than one batch of 8 lines.  The waves beyond the walk's
# end fetch nothing, and what their registers held used to be transformed and tracked as input of batch 0: a non-finite
# pattern there flooded the result with NaN, on the device only and not in every run (mf_setup zeroes them now).
MID_SHORT_WALKS = [(1, 5), (1, 7)]  # (6 planes: mid_d0(1), among the depths)


def mid_case(binding, shape, kshape, lam, seed, tag, iterations=1, nviews=2):
    """One sequential case of the fused pass through the blocking call; the fused launches are counted.  The caller sets
    MVN_PAD_MODE=none and MVN_MID_FUSED=2 and drops the cached engines."""
    inputs = flat_inputs(shape, kshape, nviews, seed)
    c0 = binding.l.mvn_mid_fused_launch_count()
    got = run_abi(binding, inputs, lam, iterations)
    assert binding.l.mvn_mid_fused_launch_count() - c0 == iterations * nviews * 2, tag
    ref, d_orc = references(inputs, lam, iterations)
    return check(got, ref, d_orc, "%s %s psf %s lam %g" % (tag, shape, kshape, lam))


MID_SLAB_D0 = 31  # the PSF's own depth (a volume may not be shallower): slabs of 15 and 16 planes with 15 halo planes on
                  # either side - each of them is the whole other slab


def mid_slabs(binding, monkeypatch, tag):
    """31 taps in the slab form (MVN_DEVICES=0,0) at the smallest d0 there is: both slabs launch the fused pass (their
    walks run from the lower halo to the upper one, no wrap), held to float64."""
    inputs = flat_inputs((MID_SLAB_D0, 512, 512), (31, 3, 3), 2, 6200)
    monkeypatch.setenv("MVN_DEVICES", "0,0")
    try:
        before, c0 = binding.l.mvn_multi_device_calls(), binding.l.mvn_mid_fused_launch_count()
        got = run_abi(binding, inputs, 0.006, 1)
        assert binding.l.mvn_multi_device_calls() == before + 1
        assert binding.l.mvn_mid_fused_launch_count() - c0 == 1 * 2 * 2 * 2  # iterations x views x convolutions x slabs
    finally:
        monkeypatch.delenv("MVN_DEVICES", raising=False)
    ref, d_orc = references(inputs, 0.006, 1)
    check(got, ref, d_orc, "%s two slabs (%d, 512, 512) psf (31, 3, 3)" % (tag, MID_SLAB_D0))


def slabs_reject_a_psf_deeper_than_the_volume(binding, monkeypatch):
    """A volume of fewer planes than a PSF is rejected and psi left untouched, with MVN_DEVICES as without: a slab with its
    halo planes is deep enough for the PSF, the volume is not (the slab path used to run such a call and return values
    7.6e-3 off the cyclic convolution it stands for)."""
    for shape, k in (((14, 6, 8), 15), ((30, 16, 32), 31)):
        views, k1, k2, w, psi0 = flat_inputs((k, ) + shape[1:], (k, 3, 3), 2, 6400)
        cut = [x[:shape[0]].copy() for x in views], k1, k2, [x[:shape[0]].copy() for x in w], psi0[:shape[0]].copy()
        for devices in (None, "0,0"):
            if devices:
                monkeypatch.setenv("MVN_DEVICES", devices)
            try:
                before = binding.l.mvn_multi_device_calls()
                got = run_abi(binding, cut, 0.006, 1)
                assert binding.l.mvn_multi_device_calls() == before, (shape, devices)
                assert np.array_equal(got, cut[4]), (shape, devices)
            finally:
                monkeypatch.delenv("MVN_DEVICES", raising=False)
        # the resident group of slab engines (mvn_group_*) refuses the same stacks when they are loaded
        import pytest
        g = binding.group([0, 0], shape, k // 2, 2)
        try:
            with pytest.raises(MvnError):
                g.load(cut[4], WorkspaceHolder(cut[0], cut[1], cut[2], cut[3], 0.006, MIN_VALUE, 1))
        finally:
            g.close()


def mid_simultaneous(binding, tag, k=15):
    """The simultaneous loop on the fused pass: whole steps and the chunked form, each against float64."""
    shape = (mid_d0(k), 512, 512)
    inputs = flat_inputs(shape, (k, 3, 3), 2, 6300)
    ref, d_orc = references(inputs, 0.006, 1, simultaneous=True)
    for chunks in (0, 4):
        c0 = binding.l.mvn_mid_fused_launch_count()
        got = run_simultaneous(binding, inputs, 0.006, 1, chunks)
        # (whole steps and chunks alike: one launch per view and convolution)
        assert binding.l.mvn_mid_fused_launch_count() - c0 == 1 * 2 * 2, chunks
        check(got, ref, d_orc, "%s simultaneous %s %s psf (%d, 3, 3)" % (tag, "chunked" if chunks else "whole steps", shape, k))


def mid_one_hot(binding, k, t1, t2, tag):
    shape = (mid_d0(k), 512, 512)
    inputs = one_hot_inputs(shape, k, t1, t2, seed=7000 + 40 * k + t1)
    c0 = binding.l.mvn_mid_fused_launch_count()
    got = run_abi(binding, inputs, 0.0, 1)
    assert binding.l.mvn_mid_fused_launch_count() - c0 == 2, tag
    ref = one_hot_reference(inputs, k, t1, t2)
    return check(got, ref, oracle_distance(inputs, ref), "%s one-hot k %d taps %d / %d" % (tag, k, t1, t2))
