"""The CPU twin of the eigenvector-following step (tests/modefollow_twin.py) against things it does not depend on: its polish
reaches true minima from asymmetric random starts, its step is the pseudo-inverse Newton step to first order, the closed-form
mode step stays bounded however small the curvature, and a frozen instance does not move.  The last test ties the twin to the
library's Python layer, so that this file fails where the feature is missing."""
import inspect

import numpy as np
import pytest

import hessian_twin as ht
import modefollow_twin as mt
import pairwise_twin as tw
from dzo_loader import dzo


@pytest.mark.parametrize("n,seed", [(5, 1), (13, 1), (38, 1)])
def test_index_0_run_reaches_a_minimum_from_an_asymmetric_random_start(n, seed):
    r = mt.run(mt.random_start(n, seed), target_index=0, max_step=0.2, zero_tol=1e-4, grad_tol=1e-10, max_steps=400)
    print(n, seed, r["steps"], r["grms"], r["index"], r["zeros"], float(r["E"]))
    assert r["status"] == mt.CONVERGED and r["grms"] <= 1e-10 and r["index"] == 0 and r["zeros"] == 6
    # independent of the twin's own evaluation: the vectorised fp64 gradient and spectrum of the other twins
    g = tw.gradient_f64(r["point"])
    assert np.sqrt((g * g).sum() / len(g)) <= 2e-10
    lam = ht.spectrum_of(r["point"])
    assert (lam < -1e-4).sum() == 0 and (np.abs(lam) <= 1e-4).sum() == 6


def test_step_is_the_pseudo_inverse_newton_step_to_first_order():
    """All curvatures positive, max_step large: h = -q / (1 + sqrt(1 + q^2)) = -F / a (1 + O(q^2)) with q = 2 F / a, so the move
    differs from -V diag(1 / lam) V^T g over the non-zero modes by at most q_max^2 / 4 of its own length."""
    p0 = np.array(ht.polished_minimum(tw.icosahedron13))
    rng = np.random.default_rng(3)
    p = p0 + 1e-7 * rng.normal(size=p0.shape)       # small: the rigid-body eigenvalues stay within zero_tol
    lam, V = mt.modes(p)
    r = mt.step(p, lam, V, target_index=0, max_step=1e6, zero_tol=1e-4, grad_tol=0.0)
    assert r["status"] == mt.ACTIVE and r["index"] == 0 and r["zeros"] == 6 and r["followed"] == -1
    keep = np.abs(lam) > 1e-4
    g = tw.gradient_f64(p)
    newton = -V[:, keep] @ ((V[:, keep].T @ g) / lam[keep])
    q = 2.0 * np.abs(V[:, keep].T @ g) / lam[keep]
    moved = r["point"] - p
    err = np.linalg.norm(moved - newton) / np.linalg.norm(newton)
    print("q_max", q.max(), "relative difference", err)
    assert q.max() < 1e-2 and err <= q.max() ** 2 / 4 + 1e-9
    assert r["step_length"] == pytest.approx(np.linalg.norm(newton), rel=1e-4)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_mode_step_is_bounded_as_the_curvature_vanishes(dtype):
    """|h| = q / (1 + sqrt(1 + q^2)) < 1 for every finite q, and 1 - |h| ~ 1 / q: the element type can tell |h| from 1 while
    1 / q > eps, so the strict bound is asserted for q < 1 / (4 eps) and |h| <= 1 (1 exactly after rounding, or 0 once q * q
    overflows) beyond, down to the smallest normal curvature.  F <= 1 keeps q = 2 F / a itself finite there."""
    dt = np.dtype(dtype)
    tiny, big, eps = np.finfo(dt).tiny, np.finfo(dt).max, np.finfo(dt).eps
    lam = np.array([1.0, 1e-3, 1e-8, 1e-20, 1e-30, tiny, -1e-30, -1.0, 2.0], dtype=dt)
    for fval in (1e-8, 1e-3, 0.25, 1.0):
        F = np.full(len(lam), fval, dtype=dt)
        h = mt.mode_steps(F, lam, 0.0, followed=7, dtype=dt)
        print(dt, fval, h)
        q = 2.0 * F.astype(np.float64) / np.abs(lam.astype(np.float64))
        assert np.all(np.isfinite(h)) and np.all(np.abs(h) <= 1)
        assert np.all(np.abs(h)[q < 0.25 / eps] < 1)
        assert h[7] > 0 and np.all(h[:7] <= 0) and h[8] < 0            # uphill on the followed mode only
    # an overflowing q * q gives h = 0 by itself
    h = mt.mode_steps(np.array([np.sqrt(big)], dtype=dt), np.array([0.5], dtype=dt), 0.0, -1, dt)
    assert h[0] == 0
    # a zero mode does not move
    assert mt.mode_steps(np.array([3.0], dtype=dt), np.array([1e-6], dtype=dt), 1e-4, -1, dt)[0] == 0


def test_a_frozen_instance_does_not_move():
    p0 = np.array(ht.polished_minimum(tw.icosahedron13))
    lam, V = mt.modes(p0)
    r = mt.step(p0, lam, V, grad_tol=1e-8)
    assert r["status"] == mt.CONVERGED and np.array_equal(r["point"], p0) and r["step_length"] == 0.0 and r["followed"] == -1
    bad = p0.copy()
    bad[4] = np.nan
    r = mt.step(bad, lam, V)
    assert r["status"] == mt.FAILED and np.array_equal(r["point"], bad, equal_nan=True)
    r = mt.step(p0 + 1e-3, lam, V, sweeps=-1)
    assert r["status"] == mt.FAILED
    # fewer non-zero modes than start_mode
    r = mt.step(p0 + 1e-3 * np.arange(39), lam, V, target_index=1, start_mode=33)
    assert r["status"] == mt.FAILED and np.array_equal(r["point"], p0 + 1e-3 * np.arange(39))


def test_the_followed_mode_is_kept_by_overlap_and_stored_with_its_sign():
    p, v = mt.kicked(np.array(ht.polished_minimum(tw.icosahedron13)) + 0.0, 0, 0.05)
    lam, V = mt.modes(p)
    r = mt.step(p, lam, V, w=-v, w_set=True, target_index=1, max_step=0.1)
    i = r["followed"]
    assert i >= 0 and r["w_set"] and np.array_equal(r["w"], V[:, i])
    assert r["overlaps"][i] == max(r["overlaps"][np.abs(lam) > 1e-4])
    assert r["h"][i] * (V[:, i] @ tw.gradient_f64(p)) > 0                 # uphill along the followed mode
    assert r["step_length"] <= 0.1


def test_python_layer_names_the_twins_statuses_and_defaults():
    assert (dzo.MODEFOLLOW_ACTIVE, dzo.MODEFOLLOW_CONVERGED, dzo.MODEFOLLOW_FAILED) == (mt.ACTIVE, mt.CONVERGED, mt.FAILED)
    sig = inspect.signature(dzo.find_saddles).parameters
    assert sig["kick"].default == 0.05 and sig["start_mode"].default == 0
    assert list(inspect.signature(dzo.polish_minima).parameters)[:2] == ["points", "n_particles"]
