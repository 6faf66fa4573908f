"""Vector extrapolation between Richardson-Lucy sweeps on the MI355X (k_accel_a, k_accel_reduce, k_accel_b;
csrc/mvn_extrapolate.hpp): the parity cases of tests/test_emu_acceleration.py on the real kernels - same shapes, same
references, same tolerances -, the invariants, the line layout at the sweep boundary, the four call paths and
run-to-run identical bits."""
import os

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from test_emu_acceleration import (MINV, N_SWEEPS, PARITY_CASES, accelerated, assert_parity, case_inputs,
                                   case_reference, lines_inputs, lines_reference)

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
    b.set_acceleration(0)


def _say(msg):
    print(msg)


@pytest.mark.parametrize("name", sorted(PARITY_CASES))
def test_psi_and_alphas_match_the_reference(gpu, monkeypatch, name):
    views, k1, k2, w, psi0, lam, env = case_inputs(name)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    gpu.l.mvn_release_cached_engines()
    ref, ref_alphas, _ = case_reference(name)
    got, alphas = accelerated(gpu, psi0, WorkspaceHolder(views, k1, k2, w, lam, MINV, N_SWEEPS))
    assert_parity(got, alphas, ref, ref_alphas, name, _say)
    gpu.l.mvn_release_cached_engines()


def test_line_layout_at_the_sweep_boundary(gpu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    gpu.l.mvn_release_cached_engines()
    views, k1, k2, w, psi0, lam = lines_inputs()
    ref, ref_alphas, _ = lines_reference()
    c0 = gpu.l.mvn_mid_fused_launch_count()
    got, alphas = accelerated(gpu, psi0, WorkspaceHolder(views, k1, k2, w, lam, MINV, N_SWEEPS))
    assert gpu.l.mvn_mid_fused_launch_count() - c0 == N_SWEEPS * 2 * 2  # iterations x views x convolutions
    assert_parity(got, alphas, ref, ref_alphas, "line layout", _say)
    gpu.l.mvn_release_cached_engines()


@pytest.mark.parametrize("name", ["fixed rows, 2 views", "odd rows", "less than one workgroup"])
def test_invariants(gpu, name):
    views, k1, k2, w, psi0, lam, _ = case_inputs(name)
    rng = np.random.default_rng(1)
    start = (psi0 * rng.uniform(0.5, 1.5, psi0.shape)).astype(np.float32)
    got, alphas = accelerated(gpu, start, WorkspaceHolder(views, k1, k2, w, lam, MINV, 0))
    assert np.array_equal(got, start) and alphas.shape == (0,)
    for n in (1, 2):
        h = WorkspaceHolder(views, k1, k2, w, lam, MINV, n)
        plain = gpu.gpu_deconvolve(start, h)
        got, alphas = accelerated(gpu, start, h)
        assert np.array_equal(got, plain), n
        assert alphas.shape == (n,) and not alphas.any()
    h = WorkspaceHolder(views, k1, k2, w, lam, MINV, 5)
    got, alphas = accelerated(gpu, start, h)
    assert alphas.shape == (5,) and alphas[0] == 0.0 and alphas[-1] == 0.0
    assert (alphas[1:-1] > 0).all() and (alphas <= 1).all()
    assert not np.array_equal(got, gpu.gpu_deconvolve(start, h))
    # the same call again: the same bits, psi and the a_k both (fixed grid, fixed order of every sum)
    again, alphas2 = accelerated(gpu, start, h)
    assert np.array_equal(again, got) and np.array_equal(alphas2, alphas)


def test_call_paths_agree(gpu):
    from libmultiviewnative_amd import native
    shape, V, n_it = (16, 32, 64), 3, 6
    from ref_fixtures import realistic_views
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=12)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, MINV, n_it)
    ref, alphas = accelerated(gpu, psi0, h)
    assert alphas.shape == (n_it,) and (alphas[1:-1] > 0).all()
    # submit / wait
    out = np.ascontiguousarray(psi0, dtype=np.float32).copy()
    before = gpu.get_pad_mode()
    gpu.set_pad_mode("none")
    try:
        gpu.set_acceleration(1)
        t = gpu.deconvolve_submit(out, h)
        gpu.set_acceleration(0)  # (captured at submit)
        gpu.deconvolve_wait(t)
        assert np.array_equal(out, ref) and np.array_equal(gpu.last_acceleration(), alphas)
        # described: strided host stacks, so that the call does not fold into the plain one
        wide = [np.zeros(shape[:2] + (shape[2] + 3,), np.float32) for _ in range(V)]
        for v in range(V):
            wide[v][..., :shape[2]] = views[v]
        out = psi0.copy()
        gpu.set_acceleration(1)
        gpu.deconvolve_described(out, [x[..., :shape[2]] for x in wide], w, k1, k2, 0.006, MINV, n_it)
        gpu.set_acceleration(0)
        assert np.array_equal(out, ref) and np.array_equal(gpu.last_acceleration(), alphas)
    finally:
        gpu.set_acceleration(0)
        gpu.set_pad_mode(before)
    # the resident engine
    e = native.EngineHandle(gpu, shape, V)
    try:
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        run, stats, al = e.iterate_accelerated(n_it, 0.006, MINV)
        assert run == n_it and stats.shape == (0, 3)
        assert np.array_equal(e.get_psi(), ref) and np.array_equal(al, alphas)
    finally:
        e.close()
