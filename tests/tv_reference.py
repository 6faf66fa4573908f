"""The numpy restatement of the total-variation factor (include/mvn_engine_api.h, mvn_set_regularization) and the
Richardson-Lucy loop with it stepped view update by view update through the CPU oracle.  Shared by test_emu_tv.py and
test_gpu_tv.py; references are computed once per process and never modified."""
import functools
import os

import numpy as np

from oracle import binding as orc
from ref_fixtures import realistic_views

F = np.float32
MINV = 1e-4
N_SWEEPS = 6
LAMBDAS = (0.002, 0.005)

# the five parity shapes of test_emu_acceleration.PARITY_CASES: name -> (shape, views, PSF extents, environment)
CASES = {
    "fixed rows": ((12, 16, 64), 2, (5, 5, 5), {}),
    "odd rows": ((10, 14, 45), 2, (5, 5, 5), {}),
    "wave rows": ((6, 8, 512), 2, (5, 5, 5), {}),
    "less than one workgroup": ((3, 5, 2), 2, (3, 3, 1), {}),
    "packed nyquist": ((16, 32, 64), 2, (5, 5, 5), {"MVN_NYQ_PACKED": "1"}),
}


def _segment_planes():
    """MVN_TV_SEG of csrc/mvn_tv.hpp: the planes one workgroup walks"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libmultiviewnative_amd", "csrc")
    for line in open(os.path.join(csrc, "mvn_tv.hpp")):
        if line.startswith("#define MVN_TV_SEG "):
            return int(line.split()[2])
    raise AssertionError("MVN_TV_SEG not found")


# more planes than one workgroup walks: two segments, the second a short one, both with a predecessor across the seam
MORE_THAN_A_SEGMENT = (_segment_planes() + 3, 5, 6)
PASS_SHAPES = [
    (3, 5, 2),      # x+1 and x-1 are the same voxel
    (2, 3, 5),
    (10, 14, 45),   # an odd row pitch
    (6, 8, 512),
    (5, 37, 130),   # tile edges inside both plane axes
    MORE_THAN_A_SEGMENT,
]


def pass_inputs(shape):
    """(what the issue names: the start estimate of realistic_views - a constant volume, every gradient 0 and
    m = epsilon -, and a view of the same fixture with 5 % multiplicative noise, so that no two neighbours agree)"""
    _, views, _, _, _, psi0 = realistic_views(shape, 1, tuple(min(s, 3) | 1 for s in shape), seed=3)
    rng = np.random.default_rng(5)
    noisy = (views[0] * rng.uniform(0.95, 1.05, shape)).astype(np.float32)
    return {"start estimate": psi0, "noisy view": noisy}


def tv_factor_np(u, lam, eps):
    """t = 1 / (1 - lam div(grad u / |grad u|_eps)): float32 after every operation, every axis cyclic (np.roll)."""
    u = np.asarray(u, dtype=F)
    lam, e2 = F(lam), F(F(eps) * F(eps))
    with np.errstate(all="ignore"):
        gz = (np.roll(u, -1, 0) - u).astype(F)
        gy = (np.roll(u, -1, 1) - u).astype(F)
        gx = (np.roll(u, -1, 2) - u).astype(F)
        s = ((gx * gx).astype(F) + (gy * gy).astype(F)).astype(F)
        s = (s + (gz * gz).astype(F)).astype(F)
        m = np.sqrt((s + e2).astype(F)).astype(F)
        r = (F(1.0) / m).astype(F)
        px, py, pz = (gx * r).astype(F), (gy * r).astype(F), (gz * r).astype(F)
        dx = (px - np.roll(px, 1, 2)).astype(F)
        dy = (py - np.roll(py, 1, 1)).astype(F)
        dz = (pz - np.roll(pz, 1, 0)).astype(F)
        dv = ((dx + dy).astype(F) + dz).astype(F)
        return (F(1.0) / (F(1.0) - (lam * dv).astype(F)).astype(F)).astype(F)


def tv_sweep(psi, views, k1, k2, w, lam, eps, minv):
    """One sequential sweep through the CPU oracle; lam == 0 (or eps None) is the plain loop without Tikhonov."""
    psi = psi.astype(F).copy()
    for v in range(len(views)):
        blurred = orc.cpu_convolution(psi, k1[v])
        q = orc.compute_quotient(views[v], blurred)
        integral = orc.cpu_convolution(q, k2[v])
        if lam > 0 and eps is not None:
            with np.errstate(all="ignore"):
                integral = (integral.astype(F) * tv_factor_np(psi, lam, eps)).astype(F)
        psi = orc.final_values(psi, integral, w[v], minv, 0.0).astype(F)
    return psi


def tv_loop(psi0, views, k1, k2, w, lam, eps, minv, n):
    psi = psi0.astype(F).copy()
    for _ in range(n):
        psi = tv_sweep(psi, views, k1, k2, w, lam, eps, minv)
    return psi


def tv_loop_accelerated(psi0, views, k1, k2, w, lam, eps, minv, n):
    """accel_reference of test_emu_acceleration.py with the TV sweep in place of the plain one."""
    y = psi0.astype(F).copy()
    x = y
    xprev = gprev = None
    mv = F(minv)
    with np.errstate(all="ignore"):
        for k in range(1, n + 1):
            x = tv_sweep(y, views, k1, k2, w, lam, eps, minv)
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
    return x


def total_variation(psi):
    """sum |grad psi|: forward differences, cyclic, summed in double"""
    u = psi.astype(np.float64)
    g2 = sum((np.roll(u, -1, d) - u) ** 2 for d in range(3))
    return float(np.sqrt(g2).sum())


def case_inputs(name):
    shape, V, ks, env = CASES[name]
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=3)
    return views, k1, k2, w, psi0, env


def case_epsilon(psi0):
    return 0.01 * float(psi0.mean())


@functools.lru_cache(maxsize=None)
def case_reference(name, lam):
    """psi after N_SWEEPS sweeps; lam == 0: the plain loop"""
    views, k1, k2, w, psi0, _ = case_inputs(name)
    x = tv_loop(psi0, views, k1, k2, w, lam, case_epsilon(psi0), MINV, N_SWEEPS)
    x.setflags(write=False)
    return x


def lines_inputs():
    # 512 x 512 planes with PSFs of 3 planes under MVN_MID_FUSED=2: the fused middle pass on the line layout
    shape, ks = (12, 512, 512), (3, 5, 3)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, ks, seed=60)
    k2 = [np.ascontiguousarray(k[::-1, :, :]) for k in k1]
    return views, k1, k2, w, psi0


LINES_LAMBDA = 0.005


@functools.lru_cache(maxsize=None)
def lines_reference():
    views, k1, k2, w, psi0 = lines_inputs()
    x = tv_loop(psi0, views, k1, k2, w, LINES_LAMBDA, case_epsilon(psi0), MINV, N_SWEEPS)
    x.setflags(write=False)
    return x


def padded_reference(psi0, views, k1, k2, w, lam, eps, minv, n):
    """The zero_padd policy applied by hand: the TV loop on the embedded stacks - the factor over the padded volume,
    cyclic at its extents -, cropped on exit."""
    dims = psi0.shape
    kmax = [max(max(a.shape[d], b.shape[d]) for a, b in zip(k1, k2)) for d in range(3)]
    ext = tuple(dims[d] + kmax[d] - 1 for d in range(3))
    off = tuple((kmax[d] - 1) // 2 for d in range(3))
    sl = tuple(slice(off[d], off[d] + dims[d]) for d in range(3))

    def embed(a):
        out = np.zeros(ext, F)
        out[sl] = a
        return out

    x = tv_loop(embed(psi0), [embed(v) for v in views], k1, k2, [embed(a) for a in w], lam, eps, minv, n)
    return x[sl]


def rel_errors(got, ref):
    err = np.abs(got.astype(np.float64) - ref)
    return (float(err.max() / np.abs(ref).max()),
            float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(np.asarray(ref, np.float64) ** 2))))


def tv_call(b, psi0, h, eps, pad="none", kind=1):
    """the blocking call with the regulariser set for its duration"""
    b.set_regularization(kind, eps)
    before = b.l.mvn_last_error()  # (the void call reports through the message alone)
    try:
        got = b.gpu_deconvolve(psi0, h, pad_mode=pad)
    finally:
        b.set_regularization(0)
    err = b.l.mvn_last_error()
    assert err == before, err
    return got
