"""The noise model on the MI355X (MVN_EPI_DIVIDE_NM / MVN_EPI_DIVIDE_NM_U16, csrc/mvn_pass_bodies.hpp): the cases of
tests/test_emu_noise_model.py on the real kernels - same shapes, same references, same bounds
(tests/noise_model_reference.py).  The five small cases reach five kernel forms: fixed rows, the run-time-radix
kernels at an odd pitch, wave rows, less than one workgroup, and the packed-Nyquist layout; the lines case the
line-layout form.  Every test prints the figures it achieved."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libmultiviewnative_amd.abi import WorkspaceHolder
from noise_model_reference import (BACKGROUND, CASES, MINV, N_SWEEPS, PSI_MX, PSI_RMS, Ref, case_inputs, case_reference,
                                   check_statistics, lines_case_inputs, lines_case_reference, nm_call,
                                   nm_loop_accelerated, rel_errors)

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
    b.set_background(None)
    b.set_likelihood(0)
    b.set_image_storage(0)
    b.set_memory_mode(None)
    b.l.mvn_release_cached_engines()


def holder(views, k1, k2, w, n=N_SWEEPS):
    return WorkspaceHolder(views, k1, k2, w, 0.0, MINV, n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_on_the_device(gpu, monkeypatch, name):
    cams, views, k1, k2, w, psi0, env = case_inputs(name)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    gpu.l.mvn_release_cached_engines()
    try:
        ref = case_reference(name)
        h = holder(views, k1, k2, w)
        # 1. psi and the statistics against the reference; what the background changes; D falls
        got, rows = nm_call(gpu, psi0, h, [BACKGROUND])
        mx, rms = rel_errors(got, ref.psi)
        print("%s: psi max %.3g rms %.3g" % (name, mx, rms))
        assert mx <= PSI_MX and rms <= PSI_RMS, (name, mx, rms)
        check_statistics(rows, ref, cams, name)
        plain = gpu.gpu_deconvolve(psi0, h)
        diff = rel_errors(got, plain)[0]
        print("  against the call with b = 0: max %.3g" % diff)
        assert diff >= 0.02, (name, diff)
        assert gpu.last_likelihood().shape[0] == 0
        per_sweep = rows[:, :, 0].sum(axis=1)
        assert (np.diff(per_sweep) < 0).all(), (name, per_sweep)
        # the same call again: the same bits, psi and statistics
        again, rows_again = nm_call(gpu, psi0, h, [BACKGROUND])
        assert np.array_equal(again, got) and np.array_equal(rows_again, rows), name
        # 2. the switches that change nothing
        for n in (1, N_SWEEPS):
            hn = holder(views, k1, k2, w, n)
            base = plain if n == N_SWEEPS else gpu.gpu_deconvolve(psi0, hn)
            g, r = nm_call(gpu, psi0, hn, None, likelihood=1)
            assert np.array_equal(g, base) and r.shape == (n, len(views), 3) and np.isfinite(r).all(), (name, n)
            g, r = nm_call(gpu, psi0, hn, [0.0, 0.0], likelihood=0)
            assert np.array_equal(g, base) and r.shape[0] == 0, (name, n)
            gpu.set_background([BACKGROUND])
            gpu.set_background(None)
            assert np.array_equal(gpu.gpu_deconvolve(psi0, hn), base), (name, n)
        # 5. the camera stacks as uint16, described, both storage modes: the same bits
        for mode in (0, 1):
            gpu.l.mvn_release_cached_engines()
            gpu.set_image_storage(mode)
            try:
                c0 = gpu.image_storage_counters()
                out = psi0.copy()
                _, r16 = nm_call(gpu, psi0, None, [BACKGROUND], described=lambda _: gpu.deconvolve_described(
                    out, cams, w, k1, k2, 0.0, MINV, N_SWEEPS))
                c1 = gpu.image_storage_counters()
            finally:
                gpu.set_image_storage(0)
            assert np.array_equal(out, got) and np.array_equal(r16, rows), (name, mode)
            assert c1[0] - c0[0] == (N_SWEEPS * len(cams) if mode == 1 else 0), (name, mode, c0, c1)
        # 6. one view streamed from host memory: the same bits
        gpu.l.mvn_release_cached_engines()
        gpu.set_memory_mode("stream:1")
        try:
            g, r = nm_call(gpu, psi0, h, [BACKGROUND])
        finally:
            gpu.set_memory_mode(None)
        assert np.array_equal(g, got) and np.array_equal(r, rows), name
    finally:
        gpu.l.mvn_release_cached_engines()


def test_line_layout(gpu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    gpu.l.mvn_release_cached_engines()
    cams, views, k1, k2, w, psi0 = lines_case_inputs()
    try:
        c0 = gpu.l.mvn_mid_fused_launch_count()
        got, rows = nm_call(gpu, psi0, holder(views, k1, k2, w), [BACKGROUND])
        assert gpu.l.mvn_mid_fused_launch_count() - c0 == N_SWEEPS * 2 * 2  # the line-layout form is the one tested
        ref = lines_case_reference()
        mx, rms = rel_errors(got, ref.psi)
        print("line layout: psi max %.3g rms %.3g" % (mx, rms))
        assert mx <= PSI_MX and rms <= PSI_RMS, (mx, rms)
        check_statistics(rows, ref, cams, "line layout")
        again, rows_again = nm_call(gpu, psi0, holder(views, k1, k2, w), [BACKGROUND])
        assert np.array_equal(again, got) and np.array_equal(rows_again, rows)
    finally:
        gpu.l.mvn_release_cached_engines()


def test_combined_with_tv_acceleration_and_convergence(gpu):
    """the test of this name in tests/test_emu_noise_model.py on the real kernels, and the same values bit for bit
    through the engine API"""
    from libmultiviewnative_amd import native
    cams, views, k1, k2, w, psi0, _ = case_inputs("fixed rows")
    lam, eps = 0.002, 0.01 * float(psi0.mean())
    V = len(views)
    ref_psi, ref_rows = nm_loop_accelerated(psi0, views, k1, k2, w, (BACKGROUND,) * V, MINV, N_SWEEPS, lam, eps)
    h = WorkspaceHolder(views, k1, k2, w, lam, MINV, N_SWEEPS)
    gpu.l.mvn_release_cached_engines()
    gpu.set_regularization(1, eps)
    gpu.set_acceleration(1)
    gpu.set_convergence(0)
    try:
        got, rows = nm_call(gpu, psi0, h, [BACKGROUND])
        run, conv = gpu.last_convergence()
        alphas = gpu.last_acceleration()
        mx, rms = rel_errors(got, ref_psi)
        print("TV + acceleration + convergence: psi max %.3g rms %.3g" % (mx, rms))
        assert mx <= PSI_MX and rms <= PSI_RMS, (mx, rms)
        assert run == N_SWEEPS and conv.shape == (N_SWEEPS, 3) and rows.shape == (N_SWEEPS, V, 3)
        check_statistics(rows, Ref(ref_psi, ref_rows[:, :, :3], ref_rows[:, :, 3]), cams, "combined")
        # a tolerance stop: rows for the sweeps that ran
        r = conv[:, 0] / conv[:, 2]
        tol = float(np.sqrt(r[2] * r[3]))  # between the third and the fourth sweep's figure
        assert r[3] < tol < r[2] and (r[:3] > tol).all()
        gpu.set_convergence(tol)
        got_s, rows_s = nm_call(gpu, psi0, h, [BACKGROUND])
        run_s, _ = gpu.last_convergence()
        assert run_s == 4 and rows_s.shape == (4, V, 3), (run_s, rows_s.shape)
        assert np.array_equal(rows_s, rows[:4])
    finally:
        gpu.set_regularization(0)
        gpu.set_acceleration(0)
        gpu.set_convergence(-1)
        gpu.l.mvn_release_cached_engines()
    # the engine API (no padding, like nm_call): the same kernels on the same values
    e = native.EngineHandle(gpu, psi0.shape, V)
    try:
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        e.set_regularization(1, eps)
        e.set_noise_model([BACKGROUND] * V, 1)
        run_e, conv_e, alphas_e = e.iterate_accelerated(N_SWEEPS, lam, MINV, 0.0)
        rows_e = e.last_likelihood()
        psi_e = e.get_psi()
    finally:
        e.close()
    assert run_e == run and np.array_equal(psi_e, got)
    assert np.array_equal(conv_e, conv) and np.array_equal(alphas_e, alphas) and np.array_equal(rows_e, rows)


_CHILD = r"""
import os, sys
import torch                      # before the library is loaded (INTEGRATION.md section 3)
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
import noise_model_reference as R
gpu = native.lib()
assert gpu.backend_name() == "hip-gfx950"
dev = torch.device("cuda:0")
name = "fixed rows"
cams, views, k1, k2, w, psi0, _ = R.case_inputs(name)
ref = R.case_reference(name)
have_u16 = hasattr(torch, "uint16")
kw = dict(int16_is_uint16=not have_u16)
stream = torch.cuda.Stream(device=dev)
for mode in (0, 1):
    gpu.check(gpu.l.mvn_release_cached_engines())
    gpu.set_image_storage(mode)
    with torch.cuda.stream(stream):
        # a wider row pitch: each stack is a window of a tensor with 6 more columns, filled on the caller's stream
        wide = [torch.zeros(c.shape[:2] + (c.shape[2] + 6,), dtype=torch.uint16 if have_u16 else torch.int16, device=dev)
                for c in cams]
        D = [x[..., 2:2 + c.shape[2]] for x, c in zip(wide, cams)]
        for d, c in zip(D, cams):
            d.copy_(torch.from_numpy(c if have_u16 else c.view(np.int16)), non_blocking=True)
        assert D[0].stride(1) == cams[0].shape[2] + 6
        D_w = [torch.from_numpy(x).to(dev, non_blocking=True) for x in w]
        psi = torch.from_numpy(psi0.copy()).to(dev, non_blocking=True)
        _, rows = R.nm_call(gpu, psi0, None, [R.BACKGROUND], described=lambda _: gpu.deconvolve_described(
            psi, D, D_w, k1, k2, 0.0, R.MINV, R.N_SWEEPS, **kw))
        got = psi.cpu().numpy()
    gpu.set_image_storage(0)
    mx, rms = R.rel_errors(got, ref.psi)
    print("device uint16 stacks, storage mode %d: psi max %.3g rms %.3g" % (mode, mx, rms))
    assert mx <= R.PSI_MX and rms <= R.PSI_RMS, (mode, mx, rms)
    R.check_statistics(rows, ref, cams, "storage mode %d" % mode)
    if mode == 0:
        first = (got, rows)
    else:
        assert np.array_equal(got, first[0]) and np.array_equal(rows, first[1])
# MVN_GRAPH=1 is set for this process: a plain call of 6 sweeps replays a captured sweep, a call with the noise model on
# does not (the graph would hold the backgrounds and the records' addresses) - before and after a capture exists
from libmultiviewnative_amd.abi import WorkspaceHolder
h = WorkspaceHolder(views, k1, k2, w, 0.0, R.MINV, R.N_SWEEPS)
gpu.check(gpu.l.mvn_release_cached_engines())
res = []
for _ in range(2):
    got, rows = R.nm_call(gpu, psi0, h, [R.BACKGROUND])
    mx, rms = R.rel_errors(got, ref.psi)
    print("with MVN_GRAPH=1: psi max %.3g rms %.3g" % (mx, rms))
    assert mx <= R.PSI_MX and rms <= R.PSI_RMS, (mx, rms)
    R.check_statistics(rows, ref, cams, "MVN_GRAPH=1")
    res.append((got, rows))
    plain = gpu.gpu_deconvolve(psi0, h)  # (captures, then replays, a sweep on the same engine)
    assert R.rel_errors(got, plain)[0] >= 0.02
assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
assert np.array_equal(res[0][0], first[0]) and np.array_equal(res[0][1], first[1])
gpu.check(gpu.l.mvn_release_cached_engines())
torch.cuda.synchronize()
print("ok")
"""


def test_uint16_device_tensors_on_the_callers_stream_and_sweep_graphs(gpu):
    # (the module's own library handle stays idle meanwhile: one GPU process works at a time.  Time limit: loading
    # torch and the library into a new process takes seconds, the two calls less)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MVN_GRAPH="1"))
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])
