"""The numpy restatement of the noise model (include/mvn_engine_api.h, mvn_set_background / mvn_set_likelihood): the
Richardson-Lucy loop with a camera background in the forward model, stepped view update by view update through the CPU
oracle, and the per-(sweep, view) statistics {D, Y, M}.  Shared by test_emu_noise_model.py and test_gpu_noise_model.py;
references are computed once per process and never modified."""
import functools
from collections import namedtuple

import numpy as np

from oracle import binding as orc
from ref_fixtures import realistic_views
from tv_reference import CASES, MINV, N_SWEEPS, lines_inputs, rel_errors, tv_factor_np  # noqa: F401

F = np.float32
BACKGROUND = 100.0
PSI_MX, PSI_RMS = 1e-4, 1e-5  # the project's stated tolerance for psi
M_BOUND = 1e-5

# psi after the sweeps; rows[k, v] = {D (float64 definition), Y, M}; d32[k, v] = D by the float32 formula
Ref = namedtuple("Ref", "psi rows d32")


def camera_stacks(views, seed=11, offset=BACKGROUND):
    """cam_v = min(poisson(view_v) + offset, 65535) as uint16: one generator per case, views in order"""
    rng = np.random.default_rng(seed)
    return [np.minimum(rng.poisson(v.astype(np.float64)) + offset, 65535).astype(np.uint16) for v in views]


def start_estimate(cams, offset=BACKGROUND):
    return np.full(cams[0].shape, float(cams[0].mean()) - offset, dtype=F)


def view_statistics(y, m, q, window=None):
    """{D64, Y, M, D32} of one view update over `window` (a tuple of slices; None: everything).  y: the image, m: the
    blurred estimate plus background, q: the quotient written, all float32."""
    if window is not None:
        y, m, q = y[window], m[window], q[window]
    y64, m64 = y.astype(np.float64), m.astype(np.float64)
    with np.errstate(all="ignore"):
        pos = y64 > 0
        ys = np.where(pos, y64, 1.0)
        d64 = np.where(pos, ys * np.log(ys / m64) - y64 + m64, m64 - y64).sum()
        t32 = ((y * np.log(q).astype(F)).astype(F) - y).astype(F)
        t32 = np.where(y > 0, (t32 + m).astype(F), (m - y).astype(F))
        d32 = t32.astype(np.float64).sum()
    return float(d64), float(y64.sum()), float(m64.sum()), float(d32)


def nm_view_update(psi, view, k1, k2, w, b, minv, lam=0.0, eps=None, window=None, guard=False):
    """One view update with background b; returns (psi, (D64, Y, M, D32))."""
    x = orc.cpu_convolution(psi, k1).astype(F)
    m = (x + F(b)).astype(F) if b != 0 else x
    with np.errstate(all="ignore"):
        q = orc.compute_quotient(view, m).astype(F)
    if guard:
        q = np.where(view == 0, F(0), q).astype(F)
    st = view_statistics(view, m, q, window)
    integral = orc.cpu_convolution(q, k2)
    if lam > 0 and eps is not None:
        with np.errstate(all="ignore"):
            integral = (integral.astype(F) * tv_factor_np(psi, lam, eps)).astype(F)
    return orc.final_values(psi, integral, w, minv, 0.0).astype(F), st


def nm_sweep(psi, views, k1, k2, w, bs, minv, lam=0.0, eps=None, window=None, guard=False):
    """One sequential sweep; returns (psi, rows [V, 4] = {D64, Y, M, D32})."""
    psi = psi.astype(F).copy()
    rows = []
    for v in range(len(views)):
        psi, st = nm_view_update(psi, views[v], k1[v], k2[v], w[v], bs[v], minv, lam, eps, window, guard)
        rows.append(st)
    return psi, np.array(rows, dtype=np.float64)


def nm_loop(psi0, views, k1, k2, w, bs, minv, n, lam=0.0, eps=None, window=None, guard=False):
    psi = psi0.astype(F).copy()
    rows = []
    for _ in range(n):
        psi, r = nm_sweep(psi, views, k1, k2, w, bs, minv, lam, eps, window, guard)
        rows.append(r)
    rows = np.array(rows)
    psi.setflags(write=False)
    rows.setflags(write=False)
    return Ref(psi, rows[:, :, :3], rows[:, :, 3])


def nm_loop_accelerated(psi0, views, k1, k2, w, bs, minv, n, lam=0.0, eps=None):
    """tv_reference.tv_loop_accelerated with the background in the sweep; returns (psi, rows [n, V, 4])."""
    y = psi0.astype(F).copy()
    x = y
    xprev = gprev = None
    mv = F(minv)
    rows = []
    with np.errstate(all="ignore"):
        for k in range(1, n + 1):
            x, r = nm_sweep(y, views, k1, k2, w, bs, minv, lam, eps)
            rows.append(r)
            if k == n:
                break
            g = (x - y).astype(F)
            a = F(0.0)
            if gprev is not None:
                num = float((g.astype(np.float64) * gprev.astype(np.float64)).sum())
                den = float((gprev.astype(np.float64) * gprev.astype(np.float64)).sum())
                r = num / den if den != 0.0 else 0.0
                if not np.isfinite(r):
                    r = 0.0
                a = F(min(max(r, 0.0), 1.0))
            if xprev is None:
                ynew = x.copy()
            else:
                t = (x + (a * (x - xprev).astype(F)).astype(F)).astype(F)
                ynew = np.where(t > mv, t, mv).astype(F)
            xprev, gprev, y = x, g, ynew
    return x, np.array(rows)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(camera stacks as uint16, the same as float32, k1, k2, weights, psi0, environment) of a case of CASES"""
    shape, V, ks, env = CASES[name]
    _, views, k1, k2, w, _ = realistic_views(shape, V, ks, seed=3)
    cams = camera_stacks(views)
    for c in cams:
        c.setflags(write=False)
    return cams, [c.astype(F) for c in cams], k1, k2, w, start_estimate(cams), env


@functools.lru_cache(maxsize=None)
def case_reference(name, backgrounds=(BACKGROUND, BACKGROUND)):
    _, views, k1, k2, w, psi0, _ = case_inputs(name)
    return nm_loop(psi0, views, k1, k2, w, backgrounds, MINV, N_SWEEPS)


@functools.lru_cache(maxsize=None)
def lines_case_inputs():
    views, k1, k2, w, _ = lines_inputs()
    cams = camera_stacks(views)
    return cams, [c.astype(F) for c in cams], k1, k2, w, start_estimate(cams)


@functools.lru_cache(maxsize=None)
def lines_case_reference():
    _, views, k1, k2, w, psi0 = lines_case_inputs()
    return nm_loop(psi0, views, k1, k2, w, (BACKGROUND, BACKGROUND), MINV, N_SWEEPS)


@functools.lru_cache(maxsize=None)
def d_bound():
    """10 x the largest deviation of the float32 formula from the float64 definition over the five cases' rows: the
    factor ten covers the device's log and the 1e-7 of the FFTs (the margin test_emu_acceleration.py gives the a_k)."""
    worst = 0.0
    for name in sorted(CASES):
        r = case_reference(name)
        worst = max(worst, float(np.abs(r.d32 / r.rows[:, :, 0] - 1.0).max()))
    return 10.0 * worst


def check_statistics(got, ref, cams, what, window=None):
    """got [sweeps, V, 3] against a Ref within the bounds; prints the achieved figures, returns them"""
    assert got.shape == ref.rows.shape, (what, got.shape, ref.rows.shape)
    dd = float(np.abs(got[:, :, 0] / ref.rows[:, :, 0] - 1.0).max())
    dm = float(np.abs(got[:, :, 2] / ref.rows[:, :, 2] - 1.0).max())
    print("%s: D within %.3g (bound %.3g), M within %.3g" % (what, dd, d_bound(), dm))
    assert dd <= d_bound(), (what, dd, d_bound())
    assert dm <= M_BOUND, (what, dm)
    for v, c in enumerate(cams):
        y = int((c if window is None else c[window]).astype(np.int64).sum())
        assert (got[:, v, 1] == float(y)).all(), (what, v, got[:, v, 1], y)  # doubles sum integers below 2^53 exactly
    return dd, dm


def nm_call(b, psi0, h, background, likelihood=1, pad="none", described=None):
    """the blocking call (or `described`, a function that makes one) under the padding policy `pad` with the noise
    model set for its duration; returns (psi, rows [sweeps, V, 3])"""
    before_pad = b.get_pad_mode()
    b.set_pad_mode(pad)
    b.set_background(background)
    b.set_likelihood(likelihood)
    before = b.l.mvn_last_error()  # (the void call reports through the message alone)
    try:
        got = described(h) if described else b.gpu_deconvolve(psi0, h, pad_mode=False)
    finally:
        b.set_background(None)
        b.set_likelihood(0)
        b.set_pad_mode(before_pad)
    err = b.l.mvn_last_error()
    assert err == before, err
    return got, b.last_likelihood()
