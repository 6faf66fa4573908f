"""One engine whose PSF buffers are replaced while it lives, against fresh engines: the body shared by
tests/test_emu_engine.py (host emulation) and tests/test_gpu_scoped.py (MI355X).  Run under the product's defaults of
the direct dim0 leg (the caller removes the suite's pin, tests/conftest.py, before the first engine is built)."""
import numpy as np

SHAPE, V = (40, 8, 16), 2
# kernel extents per stage: direct form with taps of 16 planes -> of 32 planes -> 3-D spectrum -> taps of 16 planes again
STAGES = [((3, 3, 3), True), ((17, 3, 3), True), ((35, 3, 3), False), ((3, 3, 3), True)]
LAMBDA, MIN_VALUE, SWEEPS = 0.006, 1e-4, 2


def run(binding):
    rng = np.random.default_rng(23)
    images = [rng.uniform(50, 150, SHAPE).astype(np.float32) for _ in range(V)]
    weights = [rng.uniform(0.2, 0.8, SHAPE).astype(np.float32) for _ in range(V)]
    psi = rng.uniform(80, 120, SHAPE).astype(np.float32)

    def kernels(kshape):
        ks = [rng.uniform(0.1, 1, kshape).astype(np.float32) for _ in range(2 * V)]
        return [k / k.sum() for k in ks]

    def stage(engine, ks, start):
        for v in range(V):
            engine.set_view(v, images[v], weights[v], ks[2 * v], ks[2 * v + 1])
        if start is not None:
            engine.set_psi(start)
        engine.iterate(SWEEPS, LAMBDA, MIN_VALUE)
        return engine.get_psi()

    live = binding.engine(SHAPE, V)
    try:
        assert [live.would_be_direct(k) for k, _ in STAGES] == [d for _, d in STAGES]
        live.set_psi(psi)
        for n, (kshape, _) in enumerate(STAGES):
            ks = kernels(kshape)
            got = stage(live, ks, None)
            fresh = binding.engine(SHAPE, V)
            try:
                want = stage(fresh, ks, psi)
            finally:
                fresh.close()
            assert np.isfinite(got).all() and not np.array_equal(got, psi), (n, kshape)
            assert got.tobytes() == want.tobytes(), (n, kshape, float(np.abs(got - want).max()))
            psi = got
    finally:
        live.close()
