"""Total-variation regularisation on the MI355X (k_tv_factor, csrc/mvn_tv.hpp, and the MVN_EPI_UPDATE_TV /
MVN_EPI_UPDATE_STATS_TV epilogues): the cases of tests/test_emu_tv.py on the real kernels - same shapes, same
references, same tolerances.  The pass alone is compared bit for bit: every operation of it is a correctly rounded
float32 + - x / sqrt without contraction on both sides."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import realistic_views
from tv_reference import (CASES, LAMBDAS, LINES_LAMBDA, MINV, N_SWEEPS, PASS_SHAPES, case_epsilon, case_inputs,
                          case_reference, lines_inputs, lines_reference, padded_reference, pass_inputs, rel_errors,
                          total_variation, tv_call, tv_factor_np, tv_loop_accelerated)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    yield b
    b.set_regularization(0)
    b.set_acceleration(0)
    b.set_convergence(-1)


@pytest.mark.parametrize("shape", PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pass_equals_the_numpy_restatement(gpu, shape):
    for what, u in pass_inputs(shape).items():
        eps = 0.01 * float(u.mean())
        c0 = gpu.tv_launch_count()
        t = gpu.tv_factor(u, 0.005, eps)
        assert gpu.tv_launch_count() - c0 == 1
        ref = tv_factor_np(u, 0.005, eps)
        bad = int((t.view(np.uint32) != ref.view(np.uint32)).sum())
        print("%s %s: t in [%.6f, %.6f], %d of %d words differ, max |dt| %.3g"
              % (shape, what, t.min(), t.max(), bad, t.size, float(np.abs(t - ref).max())))
        assert bad == 0, (shape, what)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_matches_the_reference(gpu, monkeypatch, name, lam):
    views, k1, k2, w, psi0, env = case_inputs(name)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    gpu.l.mvn_release_cached_engines()
    eps = case_epsilon(psi0)
    c0 = gpu.tv_launch_count()
    got = tv_call(gpu, psi0, WorkspaceHolder(views, k1, k2, w, lam, MINV, N_SWEEPS), eps)
    assert gpu.tv_launch_count() - c0 == N_SWEEPS * len(views)
    mx, rms = rel_errors(got, case_reference(name, lam))
    print("%s, lambda %g: max %.3g rms %.3g" % (name, lam, mx, rms))
    assert mx <= 1e-4 and rms <= 1e-5, (name, lam, mx, rms)
    plain = gpu.gpu_deconvolve(psi0, WorkspaceHolder(views, k1, k2, w, 0.0, MINV, N_SWEEPS))
    diff = rel_errors(got, plain)[0]
    print("  against the plain loop: max %.3g" % diff)
    assert diff >= 5e-3, (name, lam, diff)
    if lam == 0.005:
        tv_on, tv_off = total_variation(got), total_variation(plain)
        print("  sum |grad psi|: %.6g with TV, %.6g plain" % (tv_on, tv_off))
        assert tv_on < tv_off, (name, tv_on, tv_off)
    gpu.l.mvn_release_cached_engines()


def test_line_layout(gpu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    gpu.l.mvn_release_cached_engines()
    views, k1, k2, w, psi0 = lines_inputs()
    c0, t0 = gpu.l.mvn_mid_fused_launch_count(), gpu.tv_launch_count()
    got = tv_call(gpu, psi0, WorkspaceHolder(views, k1, k2, w, LINES_LAMBDA, MINV, N_SWEEPS), case_epsilon(psi0))
    assert gpu.l.mvn_mid_fused_launch_count() - c0 == N_SWEEPS * 2 * 2  # iterations x views x convolutions
    assert gpu.tv_launch_count() - t0 == N_SWEEPS * 2
    mx, rms = rel_errors(got, lines_reference())
    print("line layout: max %.3g rms %.3g" % (mx, rms))
    assert mx <= 1e-4 and rms <= 1e-5, (mx, rms)
    gpu.l.mvn_release_cached_engines()


def test_pad_zero_against_the_hand_padded_reference(gpu):
    shape, lam = (12, 16, 24), 0.005
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 5, 5), seed=3)
    eps = case_epsilon(psi0)
    ref = padded_reference(psi0, views, k1, k2, w, lam, eps, MINV, N_SWEEPS)
    got = tv_call(gpu, psi0, WorkspaceHolder(views, k1, k2, w, lam, MINV, N_SWEEPS), eps, pad="zero")
    mx, rms = rel_errors(got, ref)
    print("zero: max %.3g rms %.3g" % (mx, rms))
    assert mx <= 1e-4 and rms <= 1e-5, (mx, rms)


@pytest.mark.parametrize("name", ["fixed rows", "odd rows", "less than one workgroup"])
def test_invariants(gpu, name):
    views, k1, k2, w, psi0, _ = case_inputs(name)
    eps = case_epsilon(psi0)
    rng = np.random.default_rng(1)
    start = (psi0 * rng.uniform(0.5, 1.5, psi0.shape)).astype(np.float32)
    h0 = WorkspaceHolder(views, k1, k2, w, 0.0, MINV, 4)
    plain = gpu.gpu_deconvolve(start, h0)
    c0 = gpu.tv_launch_count()
    assert np.array_equal(tv_call(gpu, start, h0, eps), plain)  # kind 1, lambda_ == 0: the plain bits, no launch
    ht = WorkspaceHolder(views, k1, k2, w, 0.005, MINV, 4)

    def counters():
        return np.array((gpu.l.mvn_mid_fused_launch_count(), gpu.l.mvn_split_launch_count()) + gpu.stream_counters()
                        + gpu.image_storage_counters())

    before = counters()
    tik = gpu.gpu_deconvolve(start, ht)
    after = counters()
    assert np.array_equal(tv_call(gpu, start, ht, 123.0, kind=0), tik)  # kind 0: the call as it ever was ...
    assert np.array_equal(counters() - after, after - before)  # ... with its launch counts
    assert gpu.tv_launch_count() == c0
    got = tv_call(gpu, start, ht, eps)
    assert gpu.tv_launch_count() - c0 == 4 * len(views)
    assert not np.array_equal(got, tik) and not np.array_equal(got, plain)
    assert np.array_equal(tv_call(gpu, start, ht, eps), got)  # the same call twice: the same bits
    # lambda_ = 1/12: refused, psi untouched, message set
    gpu.set_regularization(1, eps)
    try:
        out = gpu.gpu_deconvolve(start, WorkspaceHolder(views, k1, k2, w, 1.0 / 12.0, MINV, 2))
    finally:
        gpu.set_regularization(0)
    assert "1/12" in gpu.l.mvn_last_error().decode() and np.array_equal(out, start)


def test_inf_voxel_as_without_tv(gpu):
    views, k1, k2, w, psi0, _ = case_inputs("fixed rows")
    start = psi0.copy()
    start[3, 4, 5] = np.inf
    plain = gpu.gpu_deconvolve(start, WorkspaceHolder(views, k1, k2, w, 0.0, MINV, 2))
    got = tv_call(gpu, start, WorkspaceHolder(views, k1, k2, w, 0.005, MINV, 2), case_epsilon(psi0))
    assert np.array_equal(got, plain, equal_nan=True) and np.isfinite(got[0, 0, 0])
    ones = [np.ones_like(x) for x in w]
    got = tv_call(gpu, start, WorkspaceHolder(views, k1, k2, ones, 0.005, MINV, 2), case_epsilon(psi0))
    far = np.ones(got.shape, bool)
    far[3, 4, 5] = False
    assert np.abs(got[far] - MINV).max() <= 1e-5


def test_call_paths_agree(gpu):
    from libmultiviewnative_amd import native
    shape, V, n_it, lam = (16, 32, 64), 3, 6, 0.005
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=12)
    views16 = [np.round(v).astype(np.uint16) for v in views]  # integer-valued, so that the stacks exist as uint16
    views = [v.astype(np.float32) for v in views16]
    eps = case_epsilon(psi0)
    h = WorkspaceHolder(views, k1, k2, w, lam, MINV, n_it)
    before = gpu.get_pad_mode()
    gpu.set_pad_mode("none")
    try:
        ref = tv_call(gpu, psi0, h, eps)
        # submit / wait: the regulariser is captured at submit
        out = np.ascontiguousarray(psi0, dtype=np.float32).copy()
        gpu.set_regularization(1, eps)
        t = gpu.deconvolve_submit(out, h)
        gpu.set_regularization(0)
        gpu.deconvolve_wait(t)
        assert np.array_equal(out, ref)
        # described: strided host stacks
        wide = [np.zeros(shape[:2] + (shape[2] + 3,), np.float32) for _ in range(V)]
        for v in range(V):
            wide[v][..., :shape[2]] = views[v]
        out = psi0.copy()
        gpu.set_regularization(1, eps)
        gpu.deconvolve_described(out, [x[..., :shape[2]] for x in wide], w, k1, k2, lam, MINV, n_it)
        assert np.array_equal(out, ref)
        # described: uint16 images kept as uint16
        out = psi0.copy()
        gpu.set_image_storage(1)
        d0 = gpu.image_storage_counters()
        gpu.deconvolve_described(out, views16, w, k1, k2, lam, MINV, n_it)
        gpu.set_image_storage(0)
        assert gpu.image_storage_counters()[0] - d0[0] == n_it * V
        assert np.array_equal(out, ref)
        # stream:1
        gpu.set_memory_mode("stream:1")
        c0 = gpu.stream_counters()
        got = gpu.gpu_deconvolve(psi0, h, pad_mode=False)
        gpu.set_memory_mode(None)
        assert gpu.stream_counters()[0] - c0[0] == 1 and np.array_equal(got, ref)
        # convergence statistics on: psi unchanged
        gpu.set_convergence(0.0)
        got = gpu.gpu_deconvolve(psi0, h, pad_mode=False)
        gpu.set_convergence(-1)
        run, rows = gpu.last_convergence()
        assert run == n_it and rows.shape == (n_it, 3) and np.isfinite(rows).all()
        assert np.array_equal(got, ref)
        # acceleration on, against the reference extended with the extrapolation
        gpu.set_acceleration(1)
        acc = gpu.gpu_deconvolve(psi0, h, pad_mode=False)
        gpu.set_acceleration(0)
        mx, rms = rel_errors(acc, tv_loop_accelerated(psi0, views, k1, k2, w, lam, eps, MINV, n_it))
        print("accelerated: max %.3g rms %.3g" % (mx, rms))
        assert mx <= 1e-4 and rms <= 1e-5, (mx, rms)
    finally:
        gpu.set_image_storage(0)
        gpu.set_memory_mode(None)
        gpu.set_convergence(-1)
        gpu.set_acceleration(0)
        gpu.set_regularization(0)
        gpu.set_pad_mode(before)
    # the resident engine
    e = native.EngineHandle(gpu, shape, V)
    try:
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        e.set_regularization(1, eps)
        e.iterate(n_it, lam, MINV)
        assert np.array_equal(e.get_psi(), ref)
        with pytest.raises(native.MvnError, match="total-variation"):
            e.compute_delta(lam, MINV)
    finally:
        e.close()


def test_memory_grows_by_one_volume(gpu):
    shape = (16, 32, 64)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 5, 5), seed=12)
    h = WorkspaceHolder(views, k1, k2, w, 0.005, MINV, 3)
    h0 = WorkspaceHolder(views, k1, k2, w, 0.0, MINV, 3)
    before = gpu.get_pad_mode()
    gpu.set_pad_mode("none")
    try:
        off, off0 = gpu.deconvolve_memory(h), gpu.deconvolve_memory(h0)
        gpu.set_regularization(1, 0.1)
        on, on0 = gpu.deconvolve_memory(h), gpu.deconvolve_memory(h0)
    finally:
        gpu.set_regularization(0)
        gpu.set_pad_mode(before)
    assert on - off == 4 * shape[0] * shape[1] * shape[2] and on0 == off0


_GRAPH_CHILD = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from ref_fixtures import realistic_views
shape, V = (32, 32, 32), 2
_, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=12)
eps = 0.01 * float(psi0.mean())
b = native.lib()
e = native.EngineHandle(b, shape, V)
res = []
for v in range(V):
    e.set_view(v, views[v], w[v], k1[v], k2[v])
# (the last rows: the factor volume is freed - by kind 0, by lambda 0 - between two calls of the SAME key, in short calls
# that take no graph and so never look at the captured one; the volume allocated next may be another address)
SEQ = ((1, 0.005, eps, 6), (1, 0.002, eps, 6), (1, 0.005, 2 * eps, 6), (0, 0.005, 0.0, 6), (1, 0.005, eps, 6),
       (0, 0.005, 0.0, 2), (1, 0.005, eps, 6), (1, 0.0, eps, 2), (1, 0.005, eps, 6))
hog = []
for i, (kind, lam, ep, n) in enumerate(SEQ):
    e.set_psi(psi0)
    e.set_regularization(kind, ep)
    if i in (6, 8):  # take the freed volume's place, so that the new one lies elsewhere
        hog.append(native.EngineHandle(b, shape, 1))
    c0 = b.tv_launch_count()
    e.iterate(n, lam, 1e-4)
    res.append(e.get_psi())
    res.append(np.full(shape, float(b.tv_launch_count() - c0), np.float32))
for h in hog:
    h.close()
e.close()
np.save(out, np.stack(res))
"""


def test_graph_replayed_sweeps_equal_direct_launches(gpu, tmp_path):
    # MVN_GRAPH=1: sweeps 2 .. n-1 are replayed from a captured graph whose key includes the regulariser's kind,
    # lambda and epsilon - every change of one of them captures anew, and the results are those of direct launches
    outs = []
    for graph in ("1", "0"):
        out = str(tmp_path / ("graph%s.npy" % graph))
        env = dict(os.environ, MVN_GRAPH=graph)
        subprocess.run([sys.executable, "-c", _GRAPH_CHILD, ROOT, out], check=True, env=env, timeout=300)
        outs.append(np.load(out))
    g, d = outs
    assert np.array_equal(g[0::2], d[0::2])
    for again in (8, 12, 16):                               # the same setting again: the same bits
        assert np.array_equal(g[0], g[again])
    assert not np.array_equal(g[0], g[2]) and not np.array_equal(g[0], g[4]) and not np.array_equal(g[0], g[6])
    # launches enqueued by the host: sweeps x 2 views directly; with graphs at most that, none with kind 0 or lambda 0
    assert [float(x[0, 0, 0]) for x in d[1::2]] == [12.0, 12.0, 12.0, 0.0, 12.0, 0.0, 12.0, 0.0, 12.0]
    assert all(float(x[0, 0, 0]) <= 12.0 for x in g[1::2])
    assert [float(g[i][0, 0, 0]) for i in (7, 11, 15)] == [0.0, 0.0, 0.0]
