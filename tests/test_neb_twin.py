"""The CPU twin of the nudged elastic band (tests/neb_twin.py) alone: its pieces do what include/dzo.h says, checked against
things the twin does not depend on, and the rule reaches the saddle that joins the two ends of a band.  No device here.

The bands are strung between the two minima below a saddle of LJ7 (``neb_twin.end_pairs``: a saddle found by
``hybridef_twin.run``, its two sides relaxed by ``modefollow_twin.run``), five images each."""
import functools

import numpy as np
import pytest

import hessian_twin as ht
import neb_twin as nb
import pairwise_twin as tw

LJ7_SEEDS = (1, 2, 3)
ZERO_TOL = 1e-4
DTYPES = [np.float32, np.float64, np.longdouble]


def _toy(e_prev, e, e_next, dtype):
    """Three one-particle images on no particular path and the tangent of the middle one for the energies given."""
    t = np.dtype(dtype).type
    x_prev, x, x_next = (np.array(v, dtype=dtype) for v in ([0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [1.5, 2.5, 0.75]))
    return (x_next - x, x - x_prev) + nb.tangent(x_prev, x, x_next, t(e_prev), t(e), t(e_next), dtype)[:1] + \
        (nb.tangent(x_prev, x, x_next, t(e_prev), t(e), t(e_next), dtype)[3],)


@pytest.mark.parametrize("dtype", DTYPES)
def test_each_tangent_branch_gives_the_hand_computed_tangent(dtype):
    eps = float(np.finfo(dtype).eps)
    unit = lambda v: np.asarray(v, dtype=np.longdouble) / np.sqrt((np.asarray(v, dtype=np.longdouble) ** 2).sum())
    # uphill to the right: d+; uphill to the left: d-
    dp, dm, tau, branch = _toy(1.0, 2.0, 4.0, dtype)
    assert branch == 0 and np.abs(tau - unit([0.5, 2.0, 0.5])).max() <= 4 * eps
    dp, dm, tau, branch = _toy(4.0, 2.0, 1.0, dtype)
    assert branch == 1 and np.abs(tau - unit([1.0, 0.5, 0.25])).max() <= 4 * eps
    # a maximum whose right neighbour is the higher one: a = max(|1.5 - 3|, |1 - 3|) = 2 on d+, b = 1.5 on d-
    dp, dm, tau, branch = _toy(1.0, 3.0, 1.5, dtype)
    assert branch == 2 and np.abs(tau - unit(2.0 * np.array([0.5, 2.0, 0.5]) + 1.5 * np.array([1.0, 0.5, 0.25]))).max() <= 4 * eps
    # a minimum whose left neighbour is the higher one: b = 1 on d+, a = 4 on d-
    dp, dm, tau, branch = _toy(5.0, 1.0, 2.0, dtype)
    assert branch == 3 and np.abs(tau - unit(1.0 * np.array([0.5, 2.0, 0.5]) + 4.0 * np.array([1.0, 0.5, 0.25]))).max() <= 4 * eps
    assert abs(float((tau.astype(np.longdouble) ** 2).sum()) - 1.0) <= 8 * eps


def _lattice_band(n, m, seed, dtype):
    return np.stack([np.concatenate(tw.lattice(n, seed=seed + i)) for i in range(m)]).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_force_is_orthogonal_to_the_tangent_apart_from_the_spring_and_the_climbing_force_keeps_the_length(dtype):
    n, m = 6, 5
    band = _lattice_band(n, m, 11, dtype)
    eps, L = float(np.finfo(dtype).eps), np.longdouble
    for spring in (1.0, 7.0):
        plain = nb.iterate(band, np.zeros_like(band), spring=spring, climb=False, dtype=dtype)
        climb = nb.iterate(band, np.zeros_like(band), spring=spring, climb=True, dtype=dtype)
        assert plain["climbing"] == -1 and climb["climbing"] == climb["highest"] == int(np.argmax(climb["E"][1:-1])) + 1
        for k in range(1, m - 1):
            g, tau, F = (plain[key][k].astype(L) for key in ("g", "tau", "F"))
            scale = float(np.abs(g).max())
            dp, dm = (band[k + 1] - band[k]).astype(L), (band[k] - band[k - 1]).astype(L)
            along = spring * (np.sqrt((dp * dp).sum()) - np.sqrt((dm * dm).sum()))
            assert abs(float((F * tau).sum() - along)) <= 64 * n * eps * scale, k
            # the part of F orthogonal to tau is the part of -g orthogonal to tau
            assert np.abs((F - (F * tau).sum() * tau) + (g - (g * tau).sum() * tau)).max() <= 64 * n * eps * scale, k
        k = climb["climbing"]
        g, F = climb["g"][k].astype(L), climb["F"][k].astype(L)
        assert abs(float(np.sqrt((F * F).sum()) - np.sqrt((g * g).sum()))) <= 64 * n * eps * float(np.abs(g).max())
        for j in range(1, m - 1):
            if j != k:
                assert np.array_equal(climb["F"][j], plain["F"][j])
        assert np.all(plain["F"][[0, -1]] == 0) and np.all(plain["tau"][[0, -1]] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_move_is_projected_velocity_verlet_with_a_cap(dtype):
    n, m = 5, 4
    band = _lattice_band(n, m, 21, dtype)
    t = np.dtype(dtype).type
    rest = nb.iterate(band, np.zeros_like(band), max_move=10.0, dtype=dtype)
    assert rest["hit"] >= {"p<=0", "uncapped"} and "p>0" not in rest["hit"]
    for k in range(1, m - 1):                                # from rest: v = dt F, x += dt v
        assert np.array_equal(rest["velocities"][k], t(0.02) * rest["F"][k])
        assert np.array_equal(rest["band"][k], band[k] + t(0.02) * rest["velocities"][k])
    along = nb.iterate(band, rest["F"], max_move=1e-3, dtype=dtype)              # v parallel to F: kept whole, then capped
    assert along["hit"] >= {"p>0", "capped"}
    for k in range(1, m - 1):
        s = (along["band"][k] - band[k]).astype(np.longdouble)
        assert abs(float(np.sqrt((s * s).sum())) - 1e-3) <= 1e-3 * 64 * float(np.finfo(dtype).eps) * np.abs(band).max() / 1e-3
        want = rest["F"][k].astype(np.longdouble) * (1 + np.longdouble(t(0.02)))
        assert np.abs(along["velocities"][k] - want).max() <= 16 * float(np.finfo(dtype).eps) * np.abs(want).max()
    against = nb.iterate(band, -rest["F"], max_move=10.0, dtype=dtype)           # v against F: dropped
    assert "p>0" not in against["hit"] and np.array_equal(against["velocities"], rest["velocities"])
    assert np.array_equal(rest["band"][[0, -1]], band[[0, -1]])
    frozen = nb.iterate(band, rest["F"], force_tol=1e9, dtype=dtype)
    assert frozen["status"] == nb.CONVERGED and np.array_equal(frozen["band"], band) and np.array_equal(frozen["velocities"], rest["F"])
    bad = band.copy()
    bad[1, 0] = np.nan
    failed = nb.iterate(bad, np.zeros_like(band), dtype=dtype)
    assert failed["status"] == nb.FAILED and np.array_equal(failed["band"][2:], bad[2:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [3, 5, 32])
def test_interpolation_reproduces_the_ends_bit_for_bit(m, dtype):
    a, b = (np.concatenate(tw.lattice(7, seed=s)).astype(dtype) for s in (1, 2))
    band = nb.interpolate(a, b, m, dtype)
    assert band.dtype == np.dtype(dtype) and band.shape == (m, 21)
    assert np.array_equal(band[0], a) and np.array_equal(band[-1], b)
    L = np.longdouble
    for k in range(m):
        want = a.astype(L) + L(np.float64(k) / np.float64(m - 1)) * (b.astype(L) - a.astype(L))   # the quotient is fp64's
        assert np.abs(band[k] - want).max() <= 4 * float(np.finfo(dtype).eps) * np.abs(want).max()


def test_energy_and_gradient_have_the_values_of_the_fp64_twin():
    for n in (7, 70):
        p = np.concatenate(tw.lattice(n, seed=3))
        E, g = nb.energy_gradient(p, np.float64)
        assert abs(E - tw.energy_f64(p)) <= 1e-13 * abs(E) and np.abs(g - tw.gradient_f64(p)).max() <= 1e-12 * np.abs(g).max()
        E32, g32 = nb.energy_gradient(p, np.float32)
        assert E32.dtype == np.float32 and abs(E32 - E) <= 4e-6 * abs(E) and np.abs(g32 - g).max() <= 1e-5 * np.abs(g).max()


@functools.lru_cache(maxsize=None)
def _lj7_runs():
    a, b, saddles, _ = nb.end_pairs(7, LJ7_SEEDS)
    return [nb.run(nb.interpolate(a[k], b[k], 5, np.float64), force_tol=1e-6, max_iterations=2000) for k in range(3)], saddles


def test_lj7_bands_converge_on_the_saddle_between_their_ends():
    """Measured: the three bands converge in 520 to 880 iterations; the climbing image has the energy of the independently
    found saddle to 2e-15.  The bound is the second-order one of tests/test_gpu_neb.py."""
    runs, saddles = _lj7_runs()
    n, force_tol = 7, 1e-6
    for k, r in enumerate(runs):
        assert r["status"] == nb.CONVERGED and 50 < r["iterations"] <= 2000 and r["climbing"] == r["highest"]
        top = r["band"][r["climbing"]]
        g = tw.gradient_f64(top)
        lam = ht.spectrum_of(saddles[k])
        assert (lam < -ZERO_TOL).sum() == 1 and np.sqrt((g * g).sum() / (3 * n)) <= force_tol
        nonzero = np.abs(lam)[np.abs(lam) > ZERO_TOL]
        # one rounding term per energy compared, each 4 x the distance of the fp64 energy twin from the longdouble one there
        rounding = lambda p: 4.0 * abs(float(np.longdouble(nb.energy_gradient(p, np.float64)[0]) - nb.energy_gradient(p, np.longdouble)[0]))
        bound = 0.5 * 3 * n * force_tol ** 2 / nonzero.min() + rounding(top) + rounding(saddles[k])
        e_saddle = nb.energy_gradient(saddles[k], np.float64)[0]
        print("band", k, "iterations", r["iterations"], "E - E*", r["E"][r["climbing"]] - e_saddle, "bound", bound)
        assert abs(r["E"][r["climbing"]] - e_saddle) <= bound
        assert r["E"][r["climbing"]] > r["E"][0] and r["E"][r["climbing"]] > r["E"][-1]


def test_fp32_twin_converges_at_the_tolerance_the_device_is_held_to():
    """The first force_tol of 1e-5, 3e-5, 1e-4, ... at which the float32 twin converges on all three bands within 2000
    iterations.  A run with force_tol = t converges iff the residual of some iteration is <= t, and it moves like the run with
    force_tol = 0 until then: so one run per band with force_tol = 0 and the smallest residual it passes through decide it."""
    a, b, _, _ = nb.end_pairs(7, LJ7_SEEDS)
    floors = []
    for k in range(3):
        x = nb.interpolate(a[k].astype(np.float32), b[k].astype(np.float32), 5, np.float32)
        v = np.zeros_like(x)
        ends = [nb.energy_gradient(x[0], np.float32)[0], nb.energy_gradient(x[-1], np.float32)[0]]
        floor = np.inf
        for it in range(2001):
            r = nb.iterate(x, v, force_tol=0.0, climb=it >= 50, end_energies=ends, dtype=np.float32)
            floor = min(floor, r["residual"])
            if r["status"] != nb.ACTIVE:
                break
            x, v = r["band"], r["velocities"]
        floors.append(floor)
    candidates = [1e-5, 3e-5, 1e-4, 3e-4, 1e-3]
    first = next(t for t in candidates if max(floors) <= t)
    print("float32 residual floors", floors, "first tolerance", first)
    assert first == nb.FP32_FORCE_TOL
