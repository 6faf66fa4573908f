"""Convergence statistics and the early stop of the Richardson-Lucy loop (mvn_set_convergence, MVN_EPI_UPDATE_STATS,
csrc/mvn_pass_bodies.hpp) on the host emulation: the per-sweep {S_k, M_k, P_k} against a float64 numpy restatement
stepped view update by view update through the CPU oracle, psi unchanged by the statistics, the early stop, the
crop window of the padded policies, the four call paths, NaN, the memory model and a streamed early stop."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from oracle import binding as orc
from ref_fixtures import realistic_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1 << 20


@pytest.fixture(scope="module")
def emu():
    b = native.Binding(native.EMU_SO)
    yield b
    b.set_convergence(-1)


def _call(b, psi0, h, tol, pad="none"):
    b.set_convergence(tol)
    try:
        got = b.gpu_deconvolve(psi0, h, pad_mode=pad)
    finally:
        b.set_convergence(-1)
    run, rows = b.last_convergence()
    return got, run, rows


def _oracle_stats(psi0, views, k1, k2, w, lam, min_value, iterations):
    """float64 {S, M, P} per sweep from the oracle's psi sequence (cyclic policy 'none')."""
    psi = psi0.astype(np.float32).copy()
    out = []
    for _ in range(iterations):
        s = m = p = 0.0
        for v in range(len(views)):
            blurred = orc.cpu_convolution(psi, k1[v])
            q = orc.compute_quotient(views[v], blurred)
            integral = orc.cpu_convolution(q, k2[v])
            nxt = orc.final_values(psi, integral, w[v], min_value, lam)
            d = np.abs(nxt.astype(np.float32) - psi).astype(np.float64)
            s += d.sum()
            m = max(m, float(d.max()))
            p += nxt.astype(np.float64).sum()
            psi = nxt.astype(np.float32)
        out.append((s, m, p))
    return np.array(out), psi


def test_symbols_declared_exported_bound(emu):
    names = ["mvn_set_convergence", "mvn_get_convergence", "mvn_last_convergence", "mvn_engine_iterate_converge"]
    hdr = open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read()
    exports = open(os.path.join(ROOT, "libmultiviewnative_amd", "csrc", "mvn_exports.map")).read()
    for n in names:
        assert n in native.ENGINE_ABI_SYMBOLS
        assert "MVN_API int %s(" % n in hdr, n
        assert "%s;" % n in exports, n
        assert getattr(emu.l, n)
    assert emu.get_convergence() == -1.0
    emu.set_convergence(0.5)
    assert emu.get_convergence() == 0.5
    emu.set_convergence(-3)
    assert emu.get_convergence() == -1.0
    assert emu.l.mvn_set_convergence(float("nan")) < 0


# (d2 = 64: a fixed walk; d2 = 45: the generic odd rows; d2 = 512: the wave rows)
@pytest.mark.parametrize("shape,V,lam", [((12, 16, 64), 2, 0.0), ((12, 16, 64), 3, 0.006), ((10, 14, 45), 2, 0.006),
                                         ((6, 8, 512), 2, 0.0)])
def test_stats_match_numpy(emu, shape, V, lam):
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=3)
    h = WorkspaceHolder(views, k1, k2, w, lam, 1e-4, 3)
    got, run, rows = _call(emu, psi0, h, 0.0)
    ref, psi_ref = _oracle_stats(psi0, views, k1, k2, w, lam, 1e-4, 3)
    assert run == 3 and rows.shape == (3, 3)
    np.testing.assert_allclose(rows[:, 0], ref[:, 0], rtol=1e-4)
    np.testing.assert_allclose(rows[:, 2], ref[:, 2], rtol=1e-4)
    assert np.abs(rows[:, 1] - ref[:, 1]).max() <= 1e-5 * np.abs(psi_ref).max()
    assert np.abs(got - psi_ref).max() <= 1e-4 * np.abs(psi_ref).max()


@pytest.mark.parametrize("shape", [(12, 16, 64), (10, 14, 45), (6, 8, 512)])
def test_stats_leave_psi_unchanged_and_early_stop(emu, shape):
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (5, 5, 5), seed=5)
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 6)
    off, run_off, rows_off = _call(emu, psi0, h, -1.0)
    assert run_off == 6 and rows_off.shape == (0, 3)
    on, run, rows = _call(emu, psi0, h, 0.0)
    assert run == 6 and np.array_equal(on, off)
    r = rows[:, 0] / rows[:, 2]
    assert r[2] < r[1], r
    t = 0.5 * (r[1] + r[2])
    stopped, run_t, rows_t = _call(emu, psi0, h, t)
    assert run_t == 3
    assert np.array_equal(rows_t, rows[:3])
    h3 = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, 3)
    three, _, _ = _call(emu, psi0, h3, -1.0)
    assert np.array_equal(stopped, three)


def test_window_of_zero_padding(emu):
    """Under the default 'zero' policy the statistics cover the returned stacks only, not the padded volume the
    call runs on.  One view and one sweep: psi before the update is the caller's psi0 inside the window."""
    shape = (12, 16, 30)
    _, views, k1, k2, w, psi0 = realistic_views(shape, 1, (5, 5, 5), seed=8)
    one = WorkspaceHolder(views, k1, k2, w, 0.0, 1e-4, 1)
    got, run, rows = _call(emu, psi0, one, 0.0, pad="zero")
    assert run == 1 and rows.shape == (1, 3)
    d = np.abs(got.astype(np.float64) - psi0.astype(np.float32))
    np.testing.assert_allclose(rows[0, 0], d.sum(), rtol=1e-6)
    np.testing.assert_allclose(rows[0, 1], d.max(), rtol=1e-6)
    np.testing.assert_allclose(rows[0, 2], got.astype(np.float64).sum(), rtol=1e-6)
    # the margins (psi 0 there before the update, min_value at least after it) are not counted
    ext = np.array(shape) + 4
    margin = int(np.prod(ext) - np.prod(shape))
    assert rows[0, 2] < got.astype(np.float64).sum() + margin * 1e-4 * float(w[0].min())
    # and the whole-volume statistics of the cyclic policy differ
    _, _, rows2 = _call(emu, psi0, one, 0.0, pad="none")
    assert not np.array_equal(rows, rows2)


def test_nan_view_and_off(emu):
    _, views, k1, k2, w, psi0 = realistic_views((12, 16, 64), 2, (5, 5, 5), seed=9)
    views = [v.copy() for v in views]
    views[1][3, 4, 5] = np.nan
    h = WorkspaceHolder(views, k1, k2, w, 0.0, 1e-4, 4)
    _, run, rows = _call(emu, psi0, h, 10.0)  # a loose tolerance: NaN must still run every sweep
    assert run == 4 and rows.shape == (4, 3)
    assert np.isnan(rows[:, 0]).all()
    _, run0, rows0 = _call(emu, psi0, h, -1.0)
    assert run0 == 4 and rows0.shape == (0, 3)


def test_engine_iterate_converge(emu):
    shape, V = (12, 16, 64), 2
    _, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=4)
    h = WorkspaceHolder(views, k1, k2, w, 0.0, 1e-4, 3)
    blocking, run_b, rows_b = _call(emu, psi0, h, 0.0)
    e = native.EngineHandle(emu, shape, V)
    try:
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        run, rows = e.iterate_converge(3, 0.0, 1e-4, 0.0)
        got = e.get_psi()
    finally:
        e.close()
    assert run == 3 and rows.shape == (3, 3)
    assert np.array_equal(got, blocking)
    assert np.array_equal(rows, rows_b)


_CHILD = r"""
import os, sys, threading
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from ref_fixtures import realistic_views
MB = 1 << 20
emu = native.Binding(native.EMU_SO)
what = sys.argv[2]
shape, V = (16, 32, 64), 3
_, views, k1, k2, w, psi0 = realistic_views(shape, V, (5, 5, 5), seed=12)
n_it = 6

def call(tol, mem=None, iters=n_it):
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, iters)
    emu.set_convergence(tol)
    emu.set_memory_mode(mem)
    try:
        got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
    finally:
        emu.set_memory_mode(None)
        emu.set_convergence(-1)
    err = emu.l.mvn_last_error().decode()
    assert not err, err
    run, rows = emu.last_convergence()
    return got, run, rows

if what == "paths":
    ref, run, rows = call(0.0)
    assert run == n_it and rows.shape == (n_it, 3)
    # submit / wait: the tolerance is captured at submit and the record moves into the waiting thread
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, n_it)
    out = np.ascontiguousarray(psi0, dtype=np.float32).copy()
    emu.set_convergence(0.0)
    t = emu.deconvolve_submit(out, h)
    emu.set_convergence(-1)
    emu.deconvolve_wait(t)
    r2, rows2 = emu.last_convergence()
    assert r2 == n_it and np.array_equal(rows2, rows) and np.array_equal(out, ref)
    # another thread's record is its own
    seen = []
    th = threading.Thread(target=lambda: seen.append(emu.last_convergence()))
    th.start(); th.join()
    assert seen[0][0] == 0 and seen[0][1].shape == (0, 3)
    # an out-of-core view
    got, r3, rows3 = call(0.0, "stream:1")
    assert r3 == n_it and np.array_equal(rows3, rows) and np.array_equal(got, ref)
    # MVN_DEVICES on fake devices: statistics on keep the call on one device
    before = emu.l.mvn_multi_device_calls()
    os.environ["MVN_DEVICES"] = "0,0"
    try:
        got, r4, rows4 = call(0.0)
    finally:
        del os.environ["MVN_DEVICES"]
    assert emu.l.mvn_multi_device_calls() == before
    assert r4 == n_it and np.array_equal(rows4, rows) and np.array_equal(got, ref)
    print("ok")
elif what == "memory":
    h = WorkspaceHolder(views, k1, k2, w, 0.006, 1e-4, n_it)
    off = emu.deconvolve_memory(h, 0)
    emu.set_convergence(0.0)
    on = emu.deconvolve_memory(h, 0)
    emu.set_convergence(-1)
    rows = shape[0] * shape[1]  # the engine runs on the padded volume: the query's own numbers are used below
    assert on > off, (on, off)
    extra = on - off
    assert extra >= 3 * 8 * V * rows and extra < 3 * 8 * V * 4 * rows + 4 * MB, extra
    emu.check(emu.l.mvn_plan_store_clear())
    os.environ["MVN_EMU_TOTAL_MB"] = str(-(-on // MB))
    got, run, st = call(0.0, "auto")
    assert run == n_it and np.isfinite(st).all()
    print("ok")
elif what == "stream_stop":
    _, _, rows = call(0.0, "stream:1")
    r = rows[:, 0] / rows[:, 2]
    t = 0.5 * (r[1] + r[2])
    before = emu.stream_counters()
    got, run, rows_t = call(t, "stream:1")
    after = emu.stream_counters()
    assert run == 3, run
    assert np.array_equal(rows_t, rows[:3])
    three, _, _ = call(-1.0, "stream:1", iters=3)
    assert np.array_equal(got, three)
    assert after[0] - before[0] == 1 and after[1] - before[1] == 3, (before, after)
    print("ok")
"""


@pytest.mark.parametrize("what", ["paths", "memory", "stream_stop"])
def test_child(what):
    env = dict(os.environ)
    env.pop("MVN_DEVICES", None)
    env.setdefault("MVN_EMU_DEVICES", "2")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, what], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
