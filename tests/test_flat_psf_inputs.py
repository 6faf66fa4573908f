"""The condition under which the flat-PSF tests (tests/flat_psf_cases.py) mean something, in float64 numpy alone: with
those inputs every single tap plane of either kernel moves the result by at least MIN_TAP_EFFECT of its maximum - a
hundred times the bound the kernels are held to.  The same perturbation of a Gaussian PSF of ref_fixtures.py is printed
beside it (not asserted): its outer taps move nothing a 1e-5 bound could see."""
import numpy as np
import pytest

import flat_psf_cases as fc
from ref_fixtures import realistic_views

SWEEPS = 2


def tap_effects(inputs, lam):
    """relative change of the float64 result for every (view, kernel, tap plane) zeroed on its own"""
    views, k1, k2, w, psi0 = inputs
    ref = fc.float64_deconvolve(psi0, views, k1, k2, w, lam, fc.MIN_VALUE, SWEEPS)
    out = {}
    for v in range(len(views)):
        for which, ks in enumerate((k1, k2)):
            for t in range(ks[v].shape[0]):
                cut = [k.copy() for k in ks]
                cut[v][t] = 0.0
                got = fc.float64_deconvolve(psi0, views, cut if which == 0 else k1, cut if which == 1 else k2, w, lam,
                                            fc.MIN_VALUE, SWEEPS)
                out[(v, which + 1, t)] = fc.distance(got, ref)
    return out


@pytest.mark.parametrize("k", [31, 33])
def test_every_tap_plane_of_a_flat_psf_moves_the_result(k):
    shape = (k + 5, 16, 32)
    eff = tap_effects(fc.flat_inputs(shape, (k, 3, 3), 2, 5000 + k), 0.006)
    lo, hi = min(eff.values()), max(eff.values())
    print("flat PSF, k %d on %s: one tap plane zeroed moves the result by %.3g .. %.3g of its maximum" % (k, shape, lo, hi))
    _, views, k1, k2, w, psi0 = realistic_views(shape, 2, (k, 3, 3), seed=5000 + k)
    g = tap_effects((views, k1, k2, w, psi0), 0.006)
    outer = max(e for (v, which, t), e in g.items() if min(t, k - 1 - t) < 2)
    print("Gaussian PSF of realistic_views, same shape: %.3g .. %.3g, the two outermost planes at either end at most %.3g"
          % (min(g.values()), max(g.values()), outer))
    assert lo >= fc.MIN_TAP_EFFECT, min(eff, key=eff.get)
    # the bound the kernels are held to is at most a hundredth of that
    assert fc.PROJECT_BOUND <= fc.MIN_TAP_EFFECT / 100.0
