"""The Morse twin (tests/morse_twin.py) against things it does not depend on: exact values at the pair minimum, numerical
derivatives in mpmath, the symmetries of a Hessian, and the 13-atom icosahedron of the literature.  No GPU."""
import numpy as np
import pytest

import morse_twin as mt
import pairwise_twin as lj

try:
    import mpmath
except ImportError:                                          # then morse_twin.radial_mp is the longdouble form, and so are the checks
    mpmath = None

LD = np.longdouble
RHOS = [6, 14]


@pytest.mark.parametrize("rho", RHOS)
def test_the_dimer_at_its_minimum_is_exact(rho):
    e, f, s = mt.radial_mp(1, rho)
    assert e == -1 and f == 0 and s == rho * rho / 2
    e, f, s = mt.radial(np.array([1.0], dtype=LD), rho)
    assert e[0] == -1 and f[0] == 0 and s[0] == LD(rho * rho) / 2


@pytest.mark.parametrize("rho", RHOS)
def test_longdouble_radial_agrees_with_mpmath(rho):
    """Within 2^-62 (8 + |a|) of the largest piece of each value (a value can pass through zero: t = 2, r = 1): longdouble
    rounds every operation to 2^-64 and exp turns the rounding of its argument a into |a| 2^-64 of t.  Far below the 2^-53 the
    device bound is built from."""
    r2 = np.exp(np.random.default_rng(rho).uniform(np.log(0.5), np.log(30.0), size=200))
    got = mt.radial(r2.astype(LD), rho)
    if mpmath is None:                                       # without mpmath: the same formulas in fp64, to 2^-48 of the largest piece
        r = np.sqrt(r2); t = np.exp(rho * (1 - r))
        want = (t * t - 2 * t, -rho * t * (t - 1) / r, rho * t * (rho * r * (2 * t - 1) + (t - 1)) / (2 * r2 * r))
        scale = (t * t + 2 * t, rho * t * (t + 1) / r, rho * t * (rho * r * (2 * t + 1) + t + 1) / (2 * r ** 3))
        for c in range(3):
            assert np.all(np.abs(got[c].astype(np.float64) - want[c]) <= 2.0 ** -48 * (8 + np.abs(rho * (1 - r))) * scale[c]), (rho, c)
        return
    with mpmath.workdps(50):
        for k, q in enumerate(r2):
            want = mt.radial_mp(float(q), rho)
            r = mpmath.sqrt(mpmath.mpf(float(q)))
            t = mpmath.exp(rho * (1 - r))
            scale = [t * t + 2 * t, rho * t * (t + 1) / r, rho * t * (rho * r * (2 * t + 1) + t + 1) / (2 * r ** 3)]
            for c in range(3):
                hi = float(got[c][k])
                value = mpmath.mpf(hi) + mpmath.mpf(float(got[c][k] - LD(hi)))
                assert abs(value - want[c]) <= mpmath.mpf(2) ** -62 * (8 + abs(rho * (1 - r))) * scale[c], (rho, q, c, value, want[c])


@pytest.mark.parametrize("rho", RHOS)
def test_first_and_second_are_the_derivatives(rho):
    """Central differences with h = 1e-20 at 80 digits: truncation 1e-40, rounding 1e-60.  Without mpmath: longdouble with
    h = 2^-21, truncation 2e-13 of the third derivative's scale and rounding 2^-64 / h = 1e-13."""
    if mpmath is None:
        h = LD(2.0) ** -21
        for r2 in (0.6, 0.9, 1.0, 1.3, 2.5, 9.0):
            up, down, here = mt.radial(LD(r2) + h, rho), mt.radial(LD(r2) - h, rho), mt.radial(LD(r2), rho)
            for k in (0, 1):
                want = (up[k] - down[k]) / (2 * h)
                assert abs(here[k + 1] - want) <= 1e-9 * (1 + abs(want)) * rho ** 2, (rho, r2, k)
        return
    with mpmath.workdps(80):
        h = mpmath.mpf(10) ** -20
        for r2 in (0.6, 0.9, 1.0, 1.3, 2.5, 9.0):
            q = mpmath.mpf(r2)
            up, down = mt.radial_mp(q + h, rho, 80), mt.radial_mp(q - h, rho, 80)
            _, f, s = mt.radial_mp(q, rho, 80)
            for got, k in ((f, 0), (s, 1)):
                want = (up[k] - down[k]) / (2 * h)
                assert abs(got - want) <= mpmath.mpf(10) ** -30 * (1 + abs(want)), (rho, r2, k, got, want)


@pytest.mark.parametrize("rho", RHOS)
def test_gradient_and_hvp_are_derivatives_of_the_sums(rho):
    x, y, z = lj.lattice(9, seed=3, spacing=1.0, jitter=0.08)
    u, v, w = np.random.default_rng(4).normal(size=(3, 9))
    g = mt.gradient(x, y, z, rho)
    p = mt.hvp(x, y, z, u, v, w, rho)
    h = LD(2.0) ** -20
    ep, em = mt.energy(x + h * u, y + h * v, z + h * w, rho), mt.energy(x - h * u, y - h * v, z - h * w, rho)
    assert abs((ep - em) / (2 * h) - (g[0] @ u + g[1] @ v + g[2] @ w)) <= 1e-9 * np.abs(g).sum()
    gp, gm = mt.gradient(x + h * u, y + h * v, z + h * w, rho), mt.gradient(x - h * u, y - h * v, z - h * w, rho)
    assert np.abs((gp - gm) / (2 * h) - p).max() <= 1e-9 * np.abs(p).max()
    hess = mt.hessian(x, y, z, rho)
    assert np.abs(hess @ np.concatenate([u, v, w]).astype(LD) - p.ravel()).max() <= 1e-15 * np.abs(p).max()


@pytest.mark.parametrize("rho", RHOS)
def test_hessian_is_symmetric_and_annihilates_translations(rho):
    x, y, z = lj.lattice(20, seed=5, spacing=1.0, jitter=0.08)
    h = mt.hessian(x, y, z, rho)
    assert np.array_equal(h, h.T)
    scale = np.abs(h).sum(axis=1).max()
    for c in range(3):
        shift = np.zeros(60, dtype=LD); shift[20 * c:20 * (c + 1)] = 1
        assert np.abs(h @ shift).max() <= 1e-17 * scale


def test_energy_delta_is_the_difference_of_energies():
    x, y, z = lj.lattice(12, seed=6, spacing=1.0, jitter=0.05)
    x2 = x.copy(); x2[5] += 0.1
    d = mt.energy_delta(x, y, z, 5, x2[5], y[5] - 0.05, z[5], 6)
    y2 = y.copy(); y2[5] -= 0.05
    assert abs(d - (mt.energy(x2, y2, z, 6) - mt.energy(x, y, z, 6))) <= 1e-17


@pytest.mark.parametrize("rho", RHOS)
def test_relaxed_icosahedron_is_a_minimum_with_six_zero_modes(rho):
    """The literature energy of the rho = 6 icosahedron is -42.439863 (Cambridge Cluster Database); the twin gives
    -42.4398631... and agrees to the printed precision.  The rho = 14 value is the twin's own (pinned in the GPU tests)."""
    p, e = mt.relaxed_icosahedron(rho)
    p = np.array(p)
    x, y, z = p[:13], p[13:26], p[26:]
    g = mt.gradient(x, y, z, rho)
    assert np.abs(g).max() <= 1e-13
    lam = np.linalg.eigvalsh(mt.hessian(x, y, z, rho).astype(np.float64))
    assert np.abs(lam[:6]).max() <= 1e-9 * lam[-1] and lam[6] > 1e-3 * lam[-1], lam[:8]
    if rho == 6:
        assert abs(e - mt.MORSE13_RHO6) <= 5e-7, e
    print(f"Morse rho = {rho}: icosahedron energy {e:.9f}, lowest vibration {lam[6]:.6f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bound_is_positive_small_and_carries_the_floor(dtype):
    """Sanity of the bound itself: a few hundred roundings of the row's scale at most, and the fp32 floor only where t underflows."""
    x, y, z = (np.asarray(a, dtype=dtype).astype(np.float64) for a in lj.lattice(65, seed=65))
    for rho in RHOS:
        S = np.abs(mt._pairs(x, y, z, rho)[5]).sum(axis=1)
        b = mt.bound("rows", dtype, x, y, z, rho)
        assert np.all(b > 0) and np.all(b <= 400 * mt.EPS[np.dtype(dtype)] * S)
    far = np.array([0.0, 40.0])
    zero = np.zeros(2)
    b32, b64 = mt.bound("energy", np.float32, far, zero, zero, 14), mt.bound("energy", np.float64, far, zero, zero, 14)
    assert b32 >= 2 * mt.TINY[np.dtype(np.float32)] / mt.EPS[np.dtype(np.float32)] and b64 < 1e-200
