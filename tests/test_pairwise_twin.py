"""The CPU twin of the pairwise Lennard-Jones functions (tests/pairwise_twin.py) against things it does not depend on:
closed-form values of the radial functions, finite differences, the definition of energy_delta, and the two
literature minima (Cambridge Cluster Database) reached with scipy from the jittered generators."""
import math
from fractions import Fraction

import numpy as np
import pytest

import pairwise_twin as tw

LD = np.longdouble


def test_exact_fma_rounds_once():
    # a * b + c where the product needs more than 53 bits: two roundings give a different answer
    a, b = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30
    c = -(1.0 + 2.0 ** -29)
    assert tw.fma(a, b, c, np.float64) == 2.0 ** -60
    assert a * b + c == 0.0
    # fp32: against exact rational arithmetic rounded by numpy from a value that fits a double exactly
    rng = np.random.default_rng(1)
    for _ in range(200):
        x, y, z = (np.float32(v) for v in rng.normal(size=3))
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        got = tw.fma(x, y, z, np.float32)
        assert got.dtype == np.float32
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        assert abs(Fraction(float(got)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


def test_radial_functions_at_the_minimum():
    r2 = 2.0 ** (1.0 / 3.0)                     # r = 2^(1/6): e = -1, e' = 0
    assert abs(tw.lj_energy(r2) + 1.0) <= 1e-14
    assert abs(tw.lj_first_derivative(r2)) <= 1e-13
    assert tw.lj_energy(1.0) == 0.0             # r = sigma
    # derivatives with respect to r2 against central differences of the function below them
    for r2 in (0.8, 1.0, 1.3, 2.5, 7.0):
        h = 1e-6 * r2
        d1 = (tw.lj_energy(r2 + h) - tw.lj_energy(r2 - h)) / (2 * h)
        d2 = (tw.lj_first_derivative(r2 + h) - tw.lj_first_derivative(r2 - h)) / (2 * h)
        assert abs(d1 - tw.lj_first_derivative(r2)) <= 1e-7 * max(1.0, abs(d1))
        assert abs(d2 - tw.lj_second_derivative(r2)) <= 1e-7 * max(1.0, abs(d2))


def test_generators():
    x, y, z = tw.icosahedron13()
    r = np.sqrt(x * x + y * y + z * z)
    assert r[0] == 0 and np.allclose(r[1:], 1.08, rtol=0, atol=1e-14)
    x, y, z = tw.octahedron38()
    p = np.stack([x, y, z], axis=1)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)) + 10 * np.eye(38)
    assert abs(d.min() - 1.09) <= 1e-14
    x, y, z = tw.lattice(1000, seed=3)
    assert len(x) == 1000 and np.array_equal(x, tw.lattice(1000, seed=3)[0])


@pytest.mark.parametrize("n", [13, 38, 65])
def test_gradient_is_the_derivative_of_the_energy(n):
    x, y, z = tw.jittered(tw.cluster(n), seed=5)
    g = tw.gradient(x, y, z)[0]
    h = 1e-5
    rng = np.random.default_rng(n)
    for _ in range(12):
        c, i = int(rng.integers(3)), int(rng.integers(n))
        arrs = [x.copy(), y.copy(), z.copy()]
        arrs[c][i] += h; ep = tw.energy(*arrs)[0]
        arrs[c][i] -= 2 * h; em = tw.energy(*arrs)[0]
        fd = float((ep - em) / (2 * h))
        assert abs(fd - float(g[c, i])) <= 1e-7 * max(1.0, abs(fd)), (c, i, fd, float(g[c, i]))
    # and the fp64 form scipy minimises
    assert np.allclose(tw.gradient_f64(np.concatenate([x, y, z])), np.concatenate([g[0], g[1], g[2]]).astype(np.float64), rtol=1e-11, atol=1e-11)
    assert abs(tw.energy_f64(np.concatenate([x, y, z])) - float(tw.energy(x, y, z)[0])) <= 1e-11 * n


@pytest.mark.parametrize("n", [13, 38])
def test_hvp_is_the_derivative_of_the_gradient(n):
    x, y, z = tw.jittered(tw.cluster(n), seed=7)
    rng = np.random.default_rng(2 * n)
    u, v, w = rng.normal(size=(3, n))
    p, S, Sc = tw.hvp(x, y, z, u, v, w)
    h = 1e-6
    gp = tw.gradient(x + h * u, y + h * v, z + h * w)[0]
    gm = tw.gradient(x - h * u, y - h * v, z - h * w)[0]
    fd = ((gp - gm) / (2 * h)).astype(np.float64)
    assert np.all(np.abs(fd - p.astype(np.float64)) <= 1e-6 * np.maximum(1.0, np.abs(fd)))
    assert np.all(Sc >= np.abs(p)) and np.all(S[None, :] >= Sc)


def test_energy_delta_is_the_difference_of_two_energies():
    x, y, z = tw.jittered(tw.octahedron38(), seed=11)
    rng = np.random.default_rng(4)
    for _ in range(10):
        i = int(rng.integers(38))
        new = (x[i] + rng.uniform(-0.2, 0.2), y[i] + rng.uniform(-0.2, 0.2), z[i] + rng.uniform(-0.2, 0.2))
        d, s = tw.energy_delta(x, y, z, i, *new)
        x2, y2, z2 = x.copy(), y.copy(), z.copy()
        x2[i], y2[i], z2[i] = new
        want = tw.energy(x2, y2, z2)[0] - tw.energy(x, y, z)[0]
        assert abs(float(d - want)) <= 1e-15 * float(s) * 38


def test_blockwise_energy_agrees():
    x, y, z = tw.lattice(700, seed=2)
    e, s = tw.energy(x, y, z)
    eb, sb = tw.energy_blockwise_f64(x, y, z, block=128)
    assert abs(eb - float(e)) <= 700 * 2.0 ** -53 * float(s)
    assert abs(sb - float(s)) <= 1e-12 * float(s)


def test_pair_forms_agree_with_the_sums():
    rng = np.random.default_rng(9)
    for _ in range(20):
        p0, p1 = rng.normal(size=3), rng.normal(size=3) + 1.0
        u0, u1 = rng.normal(size=3), rng.normal(size=3)
        xyz = [np.array([p0[c], p1[c]]) for c in range(3)]
        uvw = [np.array([u0[c], u1[c]]) for c in range(3)]
        e, s = tw.energy(*xyz)
        assert abs(tw.pair_energy(p0, p1) - float(e)) <= 40 * 2.0 ** -53 * float(s)
        g, _, S = tw.gradient(*xyz)
        assert np.all(np.abs(np.array(tw.pair_gradient(p0, p1)).T - g.astype(np.float64)) <= 40 * 2.0 ** -53 * S.astype(np.float64))
        p, _, S = tw.hvp(*xyz, *uvw)
        assert np.all(np.abs(np.array(tw.pair_hvp(p0, p1, u0, u1)).T - p.astype(np.float64)) <= 40 * 2.0 ** -53 * S.astype(np.float64))
        # fp32 single pairs are within fp32 rounding of the fp64 ones
        g32 = np.array(tw.pair_gradient(p0, p1, np.float32), dtype=np.float64)
        assert g32.dtype == np.float64 and np.allclose(g32, np.array(tw.pair_gradient(p0, p1)), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name,want,lit", [("icosahedron13", -44.326801419534, tw.LJ13), ("octahedron38", -173.928426590629, tw.LJ38)])
def test_literature_minima(name, want, lit):
    from scipy.optimize import minimize
    base = getattr(tw, name)()
    for seed in range(5):
        p0 = np.concatenate(tw.jittered(base, seed))
        r = minimize(tw.energy_f64, p0, jac=tw.gradient_f64, method="L-BFGS-B", options={"maxiter": 5000, "ftol": 1e-15, "gtol": 1e-10})
        assert abs(r.fun - want) <= 1e-10, (seed, r.fun)
        assert abs(r.fun - lit) <= 5e-7, (seed, r.fun)
