"""Convergence statistics and the early stop on the MI355X (MVN_EPI_UPDATE_STATS, csrc/mvn_pass_bodies.hpp), for
every kernel form that carries the psi update: the line layout (512 x 512 planes, direct leg), the wave rows
(d2 = 512), a fixed walk, the generic rows (odd d2) and H = 960 (d2 = 1920).  Each case asserts the form it
reached.  Statistics against a float64 numpy restatement over the CPU oracle's psi sequence; psi bit for bit with
the statistics on and off; the early stop; the blocking call, submit / wait, a streamed view and MVN_DEVICES agree
bit for bit."""
import os

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    yield b
    b.set_convergence(-1)


def _call(b, psi0, h, tol, pad="none", mem=None):
    b.set_convergence(tol)
    b.set_memory_mode(mem)
    try:
        got = b.gpu_deconvolve(psi0, h, pad_mode=pad)
    finally:
        b.set_memory_mode(None)
        b.set_convergence(-1)
    err = b.l.mvn_last_error().decode()
    assert not err, err
    run, rows = b.last_convergence()
    return got, run, rows


def _oracle_stats(psi0, views, k1, k2, w, lam, min_value, iterations):
    psi = psi0.astype(np.float32).copy()
    out = []
    for _ in range(iterations):
        s = m = p = 0.0
        for v in range(len(views)):
            integral = orc.cpu_convolution(orc.compute_quotient(views[v], orc.cpu_convolution(psi, k1[v], 16)),
                                           k2[v], 16)
            nxt = orc.final_values(psi, integral, w[v], min_value, lam).astype(np.float32)
            d = np.abs(nxt - psi).astype(np.float64)
            s += d.sum()
            m = max(m, float(d.max()))
            p += nxt.astype(np.float64).sum()
            psi = nxt
        out.append((s, m, p))
    return np.array(out), psi


# (form, shape, views, PSF)
FORMS = [
    ("lines", (16, 512, 512), 2, (5, 7, 7)),
    ("wave", (8, 64, 512), 2, (5, 5, 5)),
    ("fixed", (12, 32, 64), 3, (5, 5, 5)),
    ("generic", (10, 14, 45), 2, (5, 5, 5)),
    ("h960", (3, 8, 1920), 2, (3, 5, 5)),
]


def _assert_form(gpu, form, shape, launches):
    info = gpu.plan_describe(shape)
    if form == "lines":
        assert info["fx_rows"] == 1 and info["h"] == 256 and launches > 0
    elif form == "wave":
        assert info["fx_rows"] == 1 and info["h"] == 256 and launches == 0
    elif form == "fixed":
        assert info["fx_rows"] == 1 and info["h"] == 32
    elif form == "generic":
        assert info["fx_rows"] == 0
    else:
        assert info["fx_rows"] == 1 and info["h"] == 960


@pytest.mark.parametrize("form,shape,V,ks", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_stats_psi_and_early_stop(gpu, form, shape, V, ks, lam):
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=21)
    h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
    before = gpu.l.mvn_mid_fused_launch_count()
    off, run_off, rows_off = _call(gpu, psi0, h, -1.0)
    _assert_form(gpu, form, shape, gpu.l.mvn_mid_fused_launch_count() - before)
    assert run_off == 3 and rows_off.shape == (0, 3)
    on, run, rows = _call(gpu, psi0, h, 0.0)
    assert run == 3 and np.array_equal(on, off), "statistics changed psi"
    ref, psi_ref = _oracle_stats(psi0, views, k1, k2, w, lam, 1e-4, 3)
    np.testing.assert_allclose(rows[:, 0], ref[:, 0], rtol=1e-4)
    np.testing.assert_allclose(rows[:, 2], ref[:, 2], rtol=1e-4)
    assert np.abs(rows[:, 1] - ref[:, 1]).max() <= 1e-5 * np.abs(psi_ref).max()
    # early stop after sweep 2 of a 6-sweep call
    h6 = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 6)
    _, _, rows6 = _call(gpu, psi0, h6, 0.0)
    assert np.array_equal(rows6[:3], rows)
    r = rows6[:, 0] / rows6[:, 2]
    assert r[1] < r[0], r
    stopped, run_t, rows_t = _call(gpu, psi0, h6, 0.5 * (r[0] + r[1]))
    assert run_t == 2 and np.array_equal(rows_t, rows6[:2])
    h2 = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 2)
    two, _, _ = _call(gpu, psi0, h2, -1.0)
    # (the fused and the plain last pass round differently on the device: test_fused_pipeline_invariants)
    assert np.abs(stopped.astype(np.float64) - two).max() <= 1e-6 * np.abs(two).max()


@pytest.mark.parametrize("form,shape,V,ks", FORMS[:3], ids=[f[0] for f in FORMS[:3]])
def test_paths_agree(gpu, form, shape, V, ks):
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, ks, seed=22)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    ref, run, rows = _call(gpu, psi0, h, 0.0)
    out = np.ascontiguousarray(psi0, dtype=np.float32).copy()
    pad_before = gpu.get_pad_mode()
    gpu.set_pad_mode("none")
    gpu.set_convergence(0.0)
    try:
        t = gpu.deconvolve_submit(out, h)
    finally:
        gpu.set_convergence(-1)
    gpu.deconvolve_wait(t)
    gpu.set_pad_mode(pad_before)
    run2, rows2 = gpu.last_convergence()
    assert run2 == run and np.array_equal(rows2, rows) and np.array_equal(out, ref)
    streamed, run3, rows3 = _call(gpu, psi0, h, 0.0, mem="stream:1")
    assert run3 == run and np.array_equal(rows3, rows) and np.array_equal(streamed, ref)
    before = gpu.l.mvn_multi_device_calls()
    os.environ["MVN_DEVICES"] = "0,0"
    try:
        multi, run4, rows4 = _call(gpu, psi0, h, 0.0)
    finally:
        del os.environ["MVN_DEVICES"]
    assert gpu.l.mvn_multi_device_calls() == before
    assert run4 == run and np.array_equal(rows4, rows) and np.array_equal(multi, ref)


def _big(V):
    rng = np.random.default_rng(5)
    n = 512
    g = np.exp(-0.5 * ((np.arange(31) - 15) / 3.0) ** 2).astype(np.float32)
    k = (g[:, None, None] * g[None, :, None] * g[None, None, :]).astype(np.float32)
    k /= k.sum()
    views = [(rng.random((n, n, n), dtype=np.float32) * 50 + 10) for _ in range(V)]
    ws = [np.full((n, n, n), 1.0 / V, np.float32) for _ in range(V)]
    psi0 = np.full((n, n, n), 30.0, np.float32)
    return views, [k] * V, [k[::-1, ::-1, ::-1].copy()] * V, ws, psi0


def test_headline_512_bit_equal(gpu):
    views, k1, k2, w, psi0 = _big(6)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 2)
    off, _, _ = _call(gpu, psi0, h, -1.0, pad="zero")
    on, run, rows = _call(gpu, psi0, h, 0.0, pad="zero")
    assert run == 2 and np.isfinite(rows).all()
    assert np.array_equal(on, off)


def test_headline_512_single_view_sums(gpu):
    views, k1, k2, w, psi0 = _big(1)
    h1 = WorkspaceHolder(views, k1, k2, w, 0.0, 1e-4, 1)
    h2 = WorkspaceHolder(views, k1, k2, w, 0.0, 1e-4, 2)
    one, _, _ = _call(gpu, psi0, h1, -1.0, pad="zero")
    two, run, rows = _call(gpu, psi0, h2, 0.0, pad="zero")
    assert run == 2
    s1 = np.abs(one.astype(np.float64) - psi0).sum()
    s2 = np.abs(two.astype(np.float64) - one).sum()
    np.testing.assert_allclose(rows[0, 0], s1, rtol=1e-3)
    np.testing.assert_allclose(rows[1, 0], s2, rtol=1e-3)
