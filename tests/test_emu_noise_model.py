"""The noise model of the Richardson-Lucy loop (mvn_set_background, mvn_set_likelihood; the divide epilogues
MVN_EPI_DIVIDE_NM / MVN_EPI_DIVIDE_NM_U16 of csrc/mvn_pass_bodies.hpp) on the host emulation: psi and the statistics
{D, Y, M} against the numpy loop over the CPU oracle's pieces (tests/noise_model_reference.py), the invariance of the
default path, the window under the padded policies, the call paths, the memory model and the refusals.

Bounds: psi 1e-4 / 1e-5 (the project's stated tolerance); D relative to the float64 definition per row at most 10 x
the largest deviation of the float32 formula from it over the five cases (noise_model_reference.d_bound, about
2.8e-4); Y exactly the integer sum of the camera counts; M relative 1e-5.  Every test prints what it achieved."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
from noise_model_reference import (BACKGROUND, CASES, MINV, N_SWEEPS, PSI_MX, PSI_RMS, Ref, case_inputs,
                                   case_reference, check_statistics, d_bound, lines_case_inputs, lines_case_reference,
                                   nm_call, nm_loop, nm_loop_accelerated, rel_errors)
from ref_fixtures import expected_good_extent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(native.__file__), "csrc")
F = np.float32


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    b = native.Binding(native.EMU_SO)
    yield b
    b.set_background(None)
    b.set_likelihood(0)
    b.set_regularization(0)
    b.set_convergence(-1)
    b.set_acceleration(0)
    b.set_image_storage(0)
    b.set_memory_mode(None)
    b.l.mvn_release_cached_engines()


@pytest.fixture
def case(request, emu, monkeypatch):
    """the inputs of a case of CASES with its environment in force and no cached engine of another one"""
    def load(name):
        inp = case_inputs(name)
        for key, val in inp[-1].items():
            monkeypatch.setenv(key, val)
        emu.l.mvn_release_cached_engines()
        return inp[:-1]
    yield load
    emu.l.mvn_release_cached_engines()


def holder(views, k1, k2, w, n=N_SWEEPS, lam=0.0):
    return WorkspaceHolder(views, k1, k2, w, lam, MINV, n)


# ---- interface ----------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_bound(emu):
    names = ["mvn_set_background", "mvn_get_background", "mvn_set_likelihood", "mvn_get_likelihood",
             "mvn_last_likelihood", "mvn_engine_set_noise_model", "mvn_engine_last_likelihood"]
    hdr = open(os.path.join(ROOT, "include", "mvn_engine_api.h")).read()
    exports = open(os.path.join(CSRC, "mvn_exports.map")).read()
    for n in names:
        assert n in native.ENGINE_ABI_SYMBOLS
        assert "%s(" % n in hdr, n
        assert "%s;" % n in exports, n
        assert getattr(emu.l, n)
    assert "term = y > 0 ? (y * logf(q) - y) + m : m - y" in hdr
    assert emu.get_background().size == 0 and emu.get_likelihood() == 0
    emu.set_background([100.0, 37.5])
    emu.set_likelihood(1)
    assert emu.get_background().tolist() == [100.0, 37.5] and emu.get_likelihood() == 1
    for bad in ([-1.0], [float("nan")], [1.0, float("inf")]):
        with pytest.raises(native.MvnError, match="finite and >= 0"):
            emu.set_background(bad)
        assert emu.get_background().tolist() == [100.0, 37.5]
    for mode in (2, -1):
        with pytest.raises(native.MvnError, match="likelihood mode"):
            emu.set_likelihood(mode)
        assert emu.get_likelihood() == 1
    emu.set_background(None)
    emu.set_likelihood(0)
    assert emu.get_background().size == 0 and emu.get_likelihood() == 0


# ---- 1. every case against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_and_statistics_match_the_reference(emu, case, name):
    cams, views, k1, k2, w, psi0 = case(name)
    ref = case_reference(name)
    h = holder(views, k1, k2, w)
    got, rows = nm_call(emu, psi0, h, [BACKGROUND])
    mx, rms = rel_errors(got, ref.psi)
    print("%s: psi max %.3g rms %.3g" % (name, mx, rms))
    assert mx <= PSI_MX and rms <= PSI_RMS, (name, mx, rms)
    check_statistics(rows, ref, cams, name)
    # the background changes the estimate (5 % to 48 % of the maximum in the reference): not so without the feature
    plain = emu.gpu_deconvolve(psi0, h)
    diff = rel_errors(got, plain)[0]
    print("  against the call with b = 0: max %.3g" % diff)
    assert diff >= 0.02, (name, diff)
    assert emu.last_likelihood().shape[0] == 0  # both switches off: no rows
    # the loop fits the data better sweep after sweep
    per_sweep = rows[:, :, 0].sum(axis=1)
    print("  sum of D per sweep:", " ".join("%.6g" % d for d in per_sweep))
    assert (np.diff(per_sweep) < 0).all(), (name, per_sweep)


def test_line_layout(emu, monkeypatch):
    monkeypatch.setenv("MVN_PAD_MODE", "none")
    monkeypatch.setenv("MVN_MID_FUSED", "2")
    emu.l.mvn_release_cached_engines()
    cams, views, k1, k2, w, psi0 = lines_case_inputs()
    c0 = emu.l.mvn_mid_fused_launch_count()
    got, rows = nm_call(emu, psi0, holder(views, k1, k2, w), [BACKGROUND])
    assert emu.l.mvn_mid_fused_launch_count() - c0 == N_SWEEPS * 2 * 2  # iterations x views x convolutions
    ref = lines_case_reference()
    mx, rms = rel_errors(got, ref.psi)
    print("line layout: psi max %.3g rms %.3g" % (mx, rms))
    assert mx <= PSI_MX and rms <= PSI_RMS, (mx, rms)
    check_statistics(rows, ref, cams, "line layout")
    emu.l.mvn_release_cached_engines()


# ---- 2. the default path, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_switches_that_change_nothing(emu, case, name):
    cams, views, k1, k2, w, psi0 = case(name)
    for n in (1, N_SWEEPS):
        h = holder(views, k1, k2, w, n)
        plain = emu.gpu_deconvolve(psi0, h)
        assert emu.last_likelihood().shape[0] == 0
        # the likelihood alone measures and changes nothing
        got, rows = nm_call(emu, psi0, h, None, likelihood=1)
        assert np.array_equal(got, plain), (name, n)
        assert rows.shape == (n, len(views), 3) and np.isfinite(rows).all()
        # a background of zeros is no background, and no noise-model pass runs
        got, rows = nm_call(emu, psi0, h, [0.0, 0.0], likelihood=0)
        assert np.array_equal(got, plain) and rows.shape[0] == 0, (name, n)
        # set and cleared again
        emu.set_background([BACKGROUND])
        emu.set_background(None)
        assert np.array_equal(emu.gpu_deconvolve(psi0, h), plain), (name, n)
        assert emu.last_likelihood().shape[0] == 0


# ---- 3. per-view values and the refusals ----------------------------------------------------------------------------
def test_per_view_backgrounds_and_refusals(emu, case):
    name = "fixed rows"
    cams, views, k1, k2, w, psi0 = case(name)
    bs = (100.0, 37.5)
    ref = case_reference(name, bs)
    h = holder(views, k1, k2, w)
    got, rows = nm_call(emu, psi0, h, bs)
    mx, rms = rel_errors(got, ref.psi)
    print("per view %r: psi max %.3g rms %.3g" % (bs, mx, rms))
    assert mx <= PSI_MX and rms <= PSI_RMS, (mx, rms)
    check_statistics(rows, ref, cams, "per view")
    assert rel_errors(ref.psi, case_reference(name).psi)[0] > 1e-3  # (the second value matters)
    # a count that does not match the call's views: refused, psi untouched
    emu.set_background([100.0, 37.5, 1.0])
    try:
        psi = psi0.copy()
        emu.gpu_deconvolve_inplace(psi, h)
        assert "3 background values" in emu.l.mvn_last_error().decode()
        assert np.array_equal(psi, psi0)
    finally:
        emu.set_background(None)
    assert np.array_equal(emu.gpu_deconvolve(psi0, h), emu.gpu_deconvolve(psi0, h))


# ---- 4. the window under the padded policies ------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["zero", "zero_exact"])
def test_padded_policies_measure_the_stacks_window(emu, case, pad):
    cams, views, k1, k2, w, psi0 = case("odd rows")
    dims = psi0.shape
    kmax = [max(max(a.shape[d], b.shape[d]) for a, b in zip(k1, k2)) for d in range(3)]
    ext = [dims[d] + kmax[d] - 1 for d in range(3)]
    if pad == "zero":
        ext = [expected_good_extent(emu, n, d == 2) for d, n in enumerate(ext)]
    off = [(kmax[d] - 1) // 2 for d in range(3)]
    sl = tuple(slice(off[d], off[d] + dims[d]) for d in range(3))

    def embed(a):
        out = np.zeros(ext, F)
        out[sl] = a
        return out

    ref = nm_loop(embed(psi0), [embed(v) for v in views], k1, k2, [embed(a) for a in w], (BACKGROUND,) * 2, MINV,
                  N_SWEEPS, window=sl, guard=pad == "zero")
    got, rows = nm_call(emu, psi0, holder(views, k1, k2, w), [BACKGROUND], pad=pad)
    mx, rms = rel_errors(got, ref.psi[sl])
    print("%s %r: psi max %.3g rms %.3g" % (pad, tuple(ext), mx, rms))
    assert mx <= PSI_MX and rms <= PSI_RMS, (pad, mx, rms)
    check_statistics(rows, ref, cams, pad)  # (Y: the sum over the ORIGINAL stacks)
    # the margin would count: M over the whole padded volume is larger by the background of every margin voxel
    margin = (np.prod(ext) - np.prod(dims)) * BACKGROUND
    assert margin > 1e-2 * ref.rows[0, 0, 2]


# ---- 5. uint16 camera stacks, described, both storage modes ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_uint16_described_stacks_are_bit_equal(emu, case, name):
    cams, views, k1, k2, w, psi0 = case(name)
    want, want_rows = nm_call(emu, psi0, holder(views, k1, k2, w), [BACKGROUND])
    for mode in (0, 1):
        emu.l.mvn_release_cached_engines()
        emu.set_image_storage(mode)
        try:
            c0 = emu.image_storage_counters()
            out = psi0.copy()
            _, rows = nm_call(emu, psi0, None, [BACKGROUND],
                              described=lambda _: emu.deconvolve_described(out, cams, w, k1, k2, 0.0, MINV, N_SWEEPS))
            c1 = emu.image_storage_counters()
        finally:
            emu.set_image_storage(0)
        assert np.array_equal(out, want), (name, mode)
        assert np.array_equal(rows, want_rows), (name, mode)
        assert c1[0] - c0[0] == (N_SWEEPS * len(cams) if mode == 1 else 0), (name, mode, c0, c1)


# ---- 6. streamed views ----------------------------------------------------------------------------------------------
def test_streamed_views_are_bit_equal(emu, case):
    cams, views, k1, k2, w, psi0 = case("fixed rows")
    h = holder(views, k1, k2, w)
    want, want_rows = nm_call(emu, psi0, h, [BACKGROUND])
    emu.l.mvn_release_cached_engines()
    emu.set_memory_mode("stream:1")
    try:
        c0 = emu.stream_counters()
        got, rows = nm_call(emu, psi0, h, [BACKGROUND])
        assert emu.stream_counters()[0] - c0[0] == 1
        # ... and the ring slot's uint16 form
        emu.l.mvn_release_cached_engines()
        emu.set_image_storage(1)
        out = psi0.copy()
        _, rows16 = nm_call(emu, psi0, None, [BACKGROUND],
                            described=lambda _: emu.deconvolve_described(out, cams, w, k1, k2, 0.0, MINV, N_SWEEPS))
    finally:
        emu.set_image_storage(0)
        emu.set_memory_mode(None)
    assert np.array_equal(got, want) and np.array_equal(rows, want_rows)
    assert np.array_equal(out, want) and np.array_equal(rows16, want_rows)


# ---- 7. with total variation, acceleration and the convergence statistics -------------------------------------------
def test_combined_with_tv_acceleration_and_convergence(emu, case):
    cams, views, k1, k2, w, psi0 = case("fixed rows")
    lam, eps = 0.002, 0.01 * float(psi0.mean())
    V = len(views)
    ref_psi, ref_rows = nm_loop_accelerated(psi0, views, k1, k2, w, (BACKGROUND,) * V, MINV, N_SWEEPS, lam, eps)
    h = holder(views, k1, k2, w, lam=lam)
    emu.set_regularization(1, eps)
    emu.set_acceleration(1)
    emu.set_convergence(0)
    try:
        got, rows = nm_call(emu, psi0, h, [BACKGROUND])
        run, conv = emu.last_convergence()
        mx, rms = rel_errors(got, ref_psi)
        print("TV + acceleration + convergence: psi max %.3g rms %.3g" % (mx, rms))
        assert mx <= PSI_MX and rms <= PSI_RMS, (mx, rms)
        assert run == N_SWEEPS and conv.shape == (N_SWEEPS, 3) and rows.shape == (N_SWEEPS, V, 3)
        check_statistics(rows, Ref(ref_psi, ref_rows[:, :, :3], ref_rows[:, :, 3]), cams, "combined")
        # a tolerance stop: rows for the sweeps that ran
        r = conv[:, 0] / conv[:, 2]
        tol = float(np.sqrt(r[2] * r[3]))  # between the third and the fourth sweep's figure
        assert r[3] < tol < r[2] and (r[:3] > tol).all()
        emu.set_convergence(tol)
        got_s, rows_s = nm_call(emu, psi0, h, [BACKGROUND])
        run_s, _ = emu.last_convergence()
        assert run_s == 4 and rows_s.shape == (4, V, 3), (run_s, rows_s.shape)
        assert np.array_equal(rows_s, rows[:4])
    finally:
        emu.set_regularization(0)
        emu.set_acceleration(0)
        emu.set_convergence(-1)


# ---- 8. submit / wait -----------------------------------------------------------------------------------------------
def test_submit_wait_captures_the_noise_model_at_submit(emu, case):
    cams, views, k1, k2, w, psi0 = case("fixed rows")
    h = holder(views, k1, k2, w)
    want = [nm_call(emu, psi0, h, b) for b in ([BACKGROUND], (100.0, 37.5))]
    emu.set_pad_mode("none")
    try:
        psis = [np.ascontiguousarray(psi0.copy()) for _ in range(2)]
        emu.set_likelihood(1)
        emu.set_background([BACKGROUND])
        t0 = emu.deconvolve_submit(psis[0], h)
        emu.set_background((100.0, 37.5))
        t1 = emu.deconvolve_submit(psis[1], h)
        emu.set_background(None)  # (what is set now is not what the tickets run with)
        emu.set_likelihood(0)
        emu.deconvolve_wait(t1)
        rows1 = emu.last_likelihood()
        emu.deconvolve_wait(t0)
        rows0 = emu.last_likelihood()
    finally:
        emu.set_background(None)
        emu.set_likelihood(0)
        emu.set_pad_mode(None)
    assert np.array_equal(psis[0], want[0][0]) and np.array_equal(rows0, want[0][1])
    assert np.array_equal(psis[1], want[1][0]) and np.array_equal(rows1, want[1][1])
    assert not np.array_equal(rows0, rows1)


def all_switches(b, on, eps):
    """convergence statistics, acceleration, total variation, a background and the likelihood: all on, or all off"""
    b.set_convergence(0 if on else -1)
    b.set_acceleration(1 if on else 0)
    b.set_regularization(1 if on else 0, eps)
    b.set_background([BACKGROUND] if on else None)
    b.set_likelihood(1 if on else 0)


def last_records(b):
    run, conv = b.last_convergence()
    return run, conv, b.last_acceleration(), b.last_likelihood()


def test_submit_wait_captures_every_switch_by_value(emu, case):
    cams, views, k1, k2, w, psi0 = case("fixed rows")
    lam, eps = 0.002, 0.01 * float(psi0.mean())
    V = len(views)
    h = holder(views, k1, k2, w, lam=lam)
    emu.set_pad_mode("none")
    try:
        all_switches(emu, True, eps)
        want = emu.gpu_deconvolve(psi0, h, pad_mode=False)
        want_rec = last_records(emu)
        psi = np.ascontiguousarray(psi0.copy())
        t = emu.deconvolve_submit(psi, h)
        all_switches(emu, False, eps)  # (what is set now is not what the ticket runs with)
        emu.deconvolve_wait(t)
        got_rec = last_records(emu)
    finally:
        all_switches(emu, False, eps)
        emu.set_pad_mode(None)
    run, conv, alphas, like = want_rec
    assert run == N_SWEEPS and conv.shape == (N_SWEEPS, 3) and alphas.shape == (N_SWEEPS,) and like.shape == (N_SWEEPS, V, 3)
    assert alphas[1:-1].max() > 0 and not np.array_equal(want, emu.gpu_deconvolve(psi0, h))  # (the switches were on)
    assert np.array_equal(psi, want)
    assert got_rec[0] == run
    for got, ref in zip(got_rec[1:], want_rec[1:]):
        assert got.shape == ref.shape and np.array_equal(got, ref)


def test_memory_query_beside_a_running_call_sees_the_process_wide_switches(emu, case):
    cams, views, k1, k2, w, psi0 = case("fixed rows")
    lam, eps = 0.002, 0.01 * float(psi0.mean())
    n = 40  # (sweeps enough for the call to outlast the query by far)
    h = holder(views, k1, k2, w, n=n, lam=lam)
    emu.set_pad_mode("none")
    done = {}

    def blocking_call():
        done["psi"] = emu.gpu_deconvolve(psi0, h, pad_mode=False)
        done["rec"] = last_records(emu)

    try:
        off = emu.deconvolve_memory(h, 0)
        all_switches(emu, True, eps)
        on = emu.deconvolve_memory(h, 0)
        before = emu.tv_launch_count()
        t = threading.Thread(target=blocking_call)
        t.start()
        deadline = time.monotonic() + 120
        while emu.tv_launch_count() == before:  # the first TV pass: the call has captured its switches and is sweeping
            assert t.is_alive() and time.monotonic() < deadline
        all_switches(emu, False, eps)
        beside = emu.deconvolve_memory(h, 0)
        still_running = t.is_alive()
        t.join()
    finally:
        all_switches(emu, False, eps)
        emu.set_pad_mode(None)
    assert on > off and beside == off, (off, on, beside)
    assert still_running
    run, conv, alphas, like = done["rec"]  # (the call ran with what it captured)
    assert run == n and conv.shape == (n, 3) and alphas.shape == (n,) and like.shape == (n, len(views), 3)


_ALL_ON_CHILD = r"""
import os, sys
import numpy as np
root, streamed = sys.argv[1], int(sys.argv[2])
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from libmultiviewnative_amd import native
from libmultiviewnative_amd.abi import WorkspaceHolder
import noise_model_reference as R
emu = native.Binding(native.EMU_SO)
MB = 1 << 20
cams, views, k1, k2, w, psi0, _ = R.case_inputs("fixed rows")
V = len(views)
lam, eps = 0.002, 0.01 * float(psi0.mean())
h = WorkspaceHolder(views, k1, k2, w, lam, R.MINV, R.N_SWEEPS)
emu.set_pad_mode("none")
switches = [lambda on: emu.set_convergence(0 if on else -1),
            lambda on: emu.set_acceleration(1 if on else 0),
            lambda on: emu.set_regularization(1 if on else 0, eps),
            lambda on: (emu.set_background([R.BACKGROUND] if on else None), emu.set_likelihood(1 if on else 0))]
off = emu.deconvolve_memory(h, streamed)
deltas = []
for sw in switches:  # what each switch adds alone: the figures the tests of the switches pin
    sw(True)
    deltas.append(emu.deconvolve_memory(h, streamed) - off)
    sw(False)
assert all(d > 0 for d in deltas), deltas
for sw in switches:
    sw(True)
need = emu.deconvolve_memory(h, streamed)
print("all off %d, all on %d, deltas %r" % (off, need, deltas))
assert need - off == sum(deltas), (need - off, deltas)
# the call runs in exactly the memory the model names (rounded up to the MB): an undercount fails an allocation
os.environ["MVN_EMU_TOTAL_MB"] = str(-(-need // MB))
emu.set_memory_mode("auto" if streamed == 0 else "stream:%d" % streamed)
before = emu.stream_counters()
got = emu.gpu_deconvolve(psi0, h, pad_mode=False)
err = emu.l.mvn_last_error().decode()
assert not err, err
assert np.isfinite(got).all() and not np.array_equal(got, psi0), "the call did not run"
assert emu.stream_counters()[0] - before[0] == (1 if streamed else 0)
run, conv = emu.last_convergence()
assert run == R.N_SWEEPS and conv.shape == (run, 3) and emu.last_acceleration().shape == (run,)
assert emu.last_likelihood().shape == (run, V, 3)
print("ok")
"""


@pytest.mark.parametrize("streamed", [0, 1])
def test_the_memory_model_of_every_switch_at_once_is_what_the_call_allocates(emu, streamed):
    env = dict(os.environ, OMP_NUM_THREADS="4", **case_inputs("fixed rows")[-1])
    env.pop("MVN_EMU_TOTAL_MB", None)
    r = subprocess.run([sys.executable, "-c", _ALL_ON_CHILD, ROOT, str(streamed)], env=env, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])
    assert "exhausted" not in r.stderr, r.stderr[-4000:]


# ---- 9. the engine API, the refusals, the memory model --------------------------------------------------------------
def test_engine_api_refusals_and_memory(emu, case):
    name = "fixed rows"
    cams, views, k1, k2, w, psi0 = case(name)
    V = len(views)
    ref = case_reference(name, (100.0, 37.5))
    e = native.EngineHandle(emu, psi0.shape, V)
    try:
        for v in range(V):
            e.set_view(v, views[v], w[v], k1[v], k2[v])
        e.set_psi(psi0)
        e.iterate(N_SWEEPS, 0.0, MINV)
        plain = e.get_psi()
        assert e.last_likelihood().shape == (0, V, 3)
        e.set_psi(psi0)
        e.set_noise_model([100.0, 37.5], 1)
        e.iterate(N_SWEEPS, 0.0, MINV, sync=False)
        rows = e.last_likelihood()  # (drains the stream)
        mx, rms = rel_errors(e.get_psi(), ref.psi)
        print("engine: psi max %.3g rms %.3g" % (mx, rms))
        assert mx <= PSI_MX and rms <= PSI_RMS
        check_statistics(rows, ref, cams, "engine")
        # an engine in the mode refuses the simultaneous step and a halo hook
        for fn in (lambda: e.compute_delta(0.0, MINV), lambda: e.compute_delta_head(0.0, MINV),
                   lambda: e.set_halo_hook(lambda *a: None)):
            with pytest.raises(native.MvnError, match="noise model"):
                fn()
        for bad in ([-1.0, 0.0], [float("nan"), 0.0]):
            with pytest.raises(native.MvnError, match="finite and >= 0"):
                e.set_noise_model(bad, 0)
        with pytest.raises(native.MvnError, match="likelihood mode"):
            e.set_noise_model(None, 2)
        # back off: the plain loop's bits, no rows
        e.set_noise_model(None, 0)
        e.set_psi(psi0)
        e.iterate(N_SWEEPS, 0.0, MINV)
        assert np.array_equal(e.get_psi(), plain) and e.last_likelihood().shape[0] == 0
        # ... and an engine with a halo hook refuses the mode
        e.set_halo_hook(lambda *a: None)
        with pytest.raises(native.MvnError, match="halo"):
            e.set_noise_model(None, 1)
        e.set_halo_hook(None)
    finally:
        e.close()
    # mvn_deconvolve_memory grows by exactly the records: per view one record per row of the volume, the counts, and
    # the rows of the call, each allocation rounded to 4 KiB
    def r4k(n):
        return (n + 4095) & ~4095
    h = holder(views, k1, k2, w)
    nrows = psi0.shape[0] * psi0.shape[1]
    records = r4k(24 * nrows * V) + r4k(4 * V) + r4k(24 * N_SWEEPS * V)
    emu.set_pad_mode("none")  # (the volume of the call is the stacks': its rows are psi0's)
    try:
        for streamed in (0, 1):
            off = emu.deconvolve_memory(h, streamed)
            emu.set_likelihood(1)
            on = emu.deconvolve_memory(h, streamed)
            on_d = emu.deconvolve_memory_described(h, streamed)
            emu.set_likelihood(0)
            emu.set_background([BACKGROUND])
            on_b = emu.deconvolve_memory(h, streamed)
            emu.set_background([0.0])
            off_b = emu.deconvolve_memory(h, streamed)
            emu.set_background(None)
            assert on - off == records and on_d == on and on_b == on and off_b == off, (on, off, records)
    finally:
        emu.set_background(None)
        emu.set_likelihood(0)
        emu.set_pad_mode(None)


# ---- 10. non-finite input --------------------------------------------------------------------------------------------
def test_a_non_finite_image_voxel_makes_the_views_d_nan(emu, case):
    cams, views, k1, k2, w, psi0 = case("odd rows")
    views = [v.copy() for v in views]
    views[1][3, 4, 5] = np.nan
    h = holder(views, k1, k2, w)
    with np.errstate(all="ignore"):
        plain = emu.gpu_deconvolve(psi0, h)
        got, rows = nm_call(emu, psi0, h, None, likelihood=1)
    assert np.array_equal(got, plain, equal_nan=True)
    assert np.isnan(rows[:, 1, 0]).all() and np.isnan(rows[:, 1, 1]).all(), rows[:, 1]
    assert np.isfinite(rows[0, 0]).all()  # (view 0 of the first sweep came before the NaN reached psi)


# ---- 11. the quotient guard and image voxels of exactly 0 -----------------------------------------------------------
def test_guarded_zero_voxels_count_their_model_value(emu, case):
    cams, views, k1, k2, w, psi0 = case("odd rows")
    views = [v.copy() for v in views]
    cams = [c.copy() for c in cams]
    for a in views + cams:
        a[2:5, 3:9, 10:30] = 0
    dims = psi0.shape
    ext = [expected_good_extent(emu, dims[d] + 4, d == 2) for d in range(3)]
    sl = tuple(slice(2, 2 + dims[d]) for d in range(3))

    def embed(a):
        out = np.zeros(ext, F)
        out[sl] = a
        return out

    args = ([embed(v) for v in views], k1, k2, [embed(a) for a in w], (BACKGROUND,) * 2, MINV, N_SWEEPS)
    ref = nm_loop(embed(psi0), *args, window=sl, guard=True)
    got, rows = nm_call(emu, psi0, holder(views, k1, k2, w), [BACKGROUND], pad="zero")  # ("zero" guards the quotient)
    mx, rms = rel_errors(got, ref.psi[sl])
    print("guard: psi max %.3g rms %.3g" % (mx, rms))
    assert mx <= PSI_MX and rms <= PSI_RMS
    check_statistics(rows, ref, cams, "guard")
    # term = m on those voxels: at least their background apiece, which the D of the lit voxels alone does not hold
    n_zero = 3 * 6 * 20
    assert (rows[:, :, 0] >= n_zero * BACKGROUND).all(), rows[:, :, 0]
