"""The two utilities of the ABI that no other device test calls, on the MI355X: mvn_tv_time (the shared timing helper
on real events) and mvn_fft3_many_r2c (the shared position-order -> natural-order helper, pinned against the
single-transform path that the oracle tests pin), and an engine whose PSF buffers are replaced while it lives.  Error
paths are not provoked on the device: tests/test_emu_scoped.py drives them on the emulation."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from libmultiviewnative_amd import native
    if not os.path.exists(native.PRODUCT_SO):  # fresh checkout on the GPU box: compile, never fall back
        import __graft_entry__
        __graft_entry__.build()
    b = native.lib()
    assert b.backend_name() == "hip-gfx950"
    return b


@pytest.mark.parametrize("shape", [(3, 5, 2), (10, 14, 45)])
def test_tv_time_utility(gpu, shape):
    ms = gpu.tv_time(shape, reps=1)  # (Binding.check: return code 0)
    assert len(ms) == 2 and all(math.isfinite(t) and t > 0 for t in ms), ms


@pytest.mark.parametrize("shape", [(8, 8, 8), (6, 10, 12)])
def test_batched_r2c_equals_the_single_transform(gpu, shape):
    stacks = np.random.default_rng(17).standard_normal((2,) + shape).astype(np.float32)
    many = gpu.rfft3_many(stacks)
    for b in range(2):
        assert many[b].tobytes() == gpu.rfft3(stacks[b]).tobytes(), (shape, b)


def test_psf_buffers_replaced_on_a_live_engine_equal_fresh_engines(gpu, monkeypatch):
    """tests/psf_replace_case.py, the body tests/test_emu_engine.py runs on the emulation: taps of 16 planes -> 32 planes
    -> 3-D spectrum -> taps again on ONE engine, psi after every stage bit for bit that of a fresh engine."""
    import psf_replace_case
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_ITEMS", raising=False)
    monkeypatch.delenv("MVN_DIM0_DIRECT_MIN_PLANE", raising=False)
    psf_replace_case.run(gpu)
