"""The CPU twin of hybrid eigenvector following (tests/hybridef_twin.py) alone: the rule reaches transition states, and its
pieces do what include/dzo.h says.  No device here.

The searches start from the 16 asymmetric LJ13 minima of tests/test_gpu_modefollow.py (the same seeds, built the same way),
kicked by 0.05 along a non-zero mode, and count as found when they end CONVERGED on a point whose fp64 spectrum
(``hessian_twin.spectrum_of``) has one negative eigenvalue and six zeros, within 200 steps."""
import functools

import numpy as np
import pytest

import hessian_twin as ht
import hybridef_twin as hy
import lowmode_twin as lt
import modefollow_twin as mt
import pairwise_twin as tw

ZERO_TOL = 1e-4
SADDLE_SEEDS = [1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 14, 16, 17, 18, 19, 20]


@functools.lru_cache(maxsize=None)
def _asymmetric_minima():
    out = []
    for seed in SADDLE_SEEDS:
        r = mt.run(mt.random_start(13, seed), max_steps=400)
        assert r["status"] == mt.CONVERGED and r["index"] == 0 and r["zeros"] == 6
        out.append(r["point"].copy())
    return np.stack(out)


def _found(start_mode):
    found, steps, products, evaluations = 0, [], [], []
    for p in _asymmetric_minima():
        x, v = mt.kicked(p, start_mode, 0.05, ZERO_TOL)
        r = hy.run(x, v, max_steps=200)
        lam = ht.spectrum_of(r["point"])
        ok = r["status"] == hy.CONVERGED and (lam < -ZERO_TOL).sum() == 1 and (np.abs(lam) <= ZERO_TOL).sum() == 6 and r["steps"] <= 200
        found += bool(ok)
        if r["status"] == hy.CONVERGED:
            g = tw.gradient_f64(r["point"])
            assert np.sqrt((g * g).sum() / 39) <= 2e-10 and float(r["lam"]) < -ZERO_TOL
        steps.append(r["steps"]); products.append(r["products"]); evaluations.append(r["evaluations"])
    print("mode", start_mode, "found", found, "steps", steps, "products", products, "evaluations", evaluations)
    return found


def test_twin_finds_transition_states_along_the_lowest_mode():
    """Measured: 16 of 16, in 11 to 87 steps, 68 to 752 products and 102 to 921 gradient evaluations each."""
    found = _found(0)
    assert found >= 14 and found == hy.TWIN_FOUND[0]


def test_twin_finds_transition_states_along_the_second_mode():
    """Measured: 14 of 16; the other two end CONVERGED on saddles of index 2, which the method is known to do."""
    found = _found(1)
    assert found >= 12 and found == hy.TWIN_FOUND[1]


# ------------------------------------------------------------------------------ the step rule
def _point_and_mode(n=7, seed=3):
    x = np.concatenate(tw.lattice(n, seed=seed))
    ev, H, Pm = lt.dense_truth(x, np.float64)
    w, V = np.linalg.eigh(Pm @ H @ Pm)
    k = int(np.argmin(np.abs(w - ev[0])))
    return x, V[:, k].copy(), abs(float(w[k]))               # |lam|: the step then takes the convex count, whatever the lattice's sign


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.longdouble])
def test_uphill_step_is_capped_and_zero_for_a_zero_mode(dtype):
    t = np.dtype(dtype).type
    h, a, raw = hy.uphill(t(0.3), t(-2.0), ZERO_TOL, 0.1, dtype)
    q = t(0.6) / t(2.0)
    assert raw == q / (t(1) + np.sqrt(t(1) + q * q)) and abs(raw) > 0.1 and h == t(0.1) and a == t(2.0)
    assert hy.uphill(t(-0.3), t(-2.0), ZERO_TOL, 0.1, dtype)[0] == -t(0.1)
    assert hy.uphill(t(0.3), t(2.0), ZERO_TOL, 0.1, dtype)[0] == t(0.1)          # |lam|: the sign of lam does not enter
    h, _, raw = hy.uphill(t(0.01), t(-2.0), ZERO_TOL, 0.1, dtype)
    assert h == raw and 0 < h < 0.1                                              # below the cap: untouched
    assert hy.uphill(t(0.3), t(ZERO_TOL), ZERO_TOL, 0.1, dtype)[0] == 0          # a <= zero_tol
    assert hy.uphill(t(0.3), t(0.0), ZERO_TOL, 0.1, dtype)[0] == 0
    assert hy.uphill(t(0.3), t(2 * ZERO_TOL), ZERO_TOL, 0.1, dtype)[0] == t(0.1)
    assert abs(hy.uphill(t(1e30), t(1e-3), 0.0, 10.0, dtype)[0]) <= 1            # bounded by 1 for any a


def test_step_is_invariant_to_the_sign_of_the_mode():
    x, u, lam = _point_and_mode()
    a, b = hy.step(x, u, lam, tangent_steps=3, tangent_steps_convex=3), hy.step(x, -u, lam, tangent_steps=3, tangent_steps_convex=3)
    assert a["status"] == b["status"] == hy.ACTIVE and a["tangent"] == b["tangent"] == 3
    assert a["F"] == -b["F"] and a["h"] == -b["h"] and a["F"] != 0
    assert np.array_equal(a["point"], b["point"])


def test_records_are_those_of_the_point_before_the_move_and_frozen_instances_do_not_move():
    x, u, lam = _point_and_mode()
    r = hy.step(x, u, lam)
    E, g = mt.energy_gradient(x, np.float64)
    assert r["E"] == E and np.array_equal(r["g"], g) and not np.array_equal(r["point"], x)
    assert r["evaluations"] == 1 + 2 and r["tangent"] == 2                       # lam > 0: the convex count
    assert hy.step(x, u, -abs(lam))["tangent"] == 10
    done = hy.step(x, u, lam, grad_tol=1e9)
    assert done["status"] == hy.CONVERGED and np.array_equal(done["point"], x) and done["h"] == 0 and done["tangent"] == 0
    bad = x.copy()
    bad[4] = np.nan
    for r in (hy.step(bad, u, lam), hy.step(x, u, np.nan), hy.step(x, u, lam, mode_failed=True)):
        assert r["status"] == hy.FAILED and r["tangent"] == 0
    assert np.array_equal(hy.step(x, u, np.inf)["point"], x)


def test_tangent_steps_stay_orthogonal_to_the_mode_and_lower_the_energy():
    x, u, lam = _point_and_mode()
    none, some = hy.step(x, u, lam, tangent_steps_convex=0), hy.step(x, u, lam, tangent_steps_convex=6)
    assert none["tangent"] == 0 and none["evaluations"] == 1 and some["tangent"] == 6
    assert np.allclose(none["point"], x + float(none["h"]) * u, rtol=0, atol=1e-15)
    moved = some["point"] - none["point"]
    assert abs(moved @ u) <= 1e-14 * np.linalg.norm(moved) and np.linalg.norm(moved) > 1e-4
    assert tw.energy_f64(some["point"]) < tw.energy_f64(none["point"])


def test_tangent_cap_scales_the_step():
    x, u, lam = _point_and_mode()
    free = hy.step(x, u, lam, tangent_steps_convex=1, tangent_cap=1e3, tangent_first=0.01)
    capped = hy.step(x, u, lam, tangent_steps_convex=1, tangent_cap=1e-3, tangent_first=0.01)
    start = hy.step(x, u, lam, tangent_steps_convex=0)["point"]
    dn = dict((k, v) for k, v, _ in free["branches"])["dn"]
    assert dn > 1e-3 and np.linalg.norm(free["point"] - start) == pytest.approx(dn, rel=1e-9)
    assert np.linalg.norm(capped["point"] - start) == pytest.approx(1e-3, rel=1e-9)
    d0, d1 = free["point"] - start, capped["point"] - start
    assert np.allclose(d1 / np.linalg.norm(d1), d0 / np.linalg.norm(d0), rtol=0, atol=1e-9)


def test_a_non_positive_sy_falls_back_to_tangent_first():
    """Next to a transition state, displaced along its downhill mode, with the HIGHEST mode as u: the tangent space holds the
    negative curvature, the projected gradient lies along it, and a step s down it meets y = H s = lam_0 s: s.y < 0."""
    x0, v0 = mt.kicked(_asymmetric_minima()[0], 0, 0.05, ZERO_TOL)
    saddle = hy.run(x0, v0, max_steps=200)
    assert saddle["status"] == hy.CONVERGED
    lam, V = mt.modes(saddle["point"])
    assert lam[0] < -1.0
    x = saddle["point"] + 0.01 * V[:, 0]
    r = hy.step(x, V[:, -1], lam[-1], tangent_steps_convex=2, tangent_first=0.01, tangent_cap=1e3)
    sy = [v for k, v, _ in r["branches"] if k == "sy"]
    dn = [v for k, v, _ in r["branches"] if k == "dn"]
    prms = [v for k, v, _ in r["branches"] if k == "prms"]
    assert r["tangent"] == 2 and len(sy) == 1 and sy[0] < 0
    assert dn[1] == pytest.approx(0.01 * prms[1] * np.sqrt(len(x)), rel=1e-12)   # alpha = tangent_first again
    assert prms[1] > prms[0]                                                     # (downhill from a saddle the slope grows)
