"""The alignment twin (tests/align_twin.py) checked against things it does not depend on: the brute-force minimum over all
permutations, scipy's assignment solver where scipy imports, the monotone decrease of the alternation, and the recovery of
planted rotations, translations, relabellings and inversions.  CPU only; the kernel is compared with the twin in
tests/test_gpu_align.py."""
import itertools

import numpy as np
import pytest

import align_twin as at


def _brute(c):
    n = len(c)
    return min(sum(c[i, p[i]] for i in range(n)) for p in itertools.permutations(range(n)))


@pytest.mark.parametrize("n", range(1, 8))
def test_assignment_cost_is_the_brute_force_minimum(n):
    rng = np.random.default_rng(100 + n)
    for _ in range(3):
        a, b = at.ball_points(rng, n), at.ball_points(rng, n)
        perm, cost = at.assign(a, b)
        assert sorted(perm) == list(range(n))
        best = _brute(at.cost_matrix(a, b))
        assert abs(cost - best) <= 1e-14 * max(1.0, best), (n, cost, best)
    for _ in range(3):                                       # lattice points: many equal costs, every sum exact
        a = rng.integers(0, 3, (n, 3)).astype(np.float64)
        b = rng.integers(0, 3, (n, 3)).astype(np.float64)
        perm, cost = at.assign(a, b)
        assert sorted(perm) == list(range(n))
        assert cost == _brute(at.cost_matrix(a, b)), (n, cost)


def test_ties_go_to_the_lowest_column():
    a = np.zeros((3, 3))
    perm, cost = at.assign(a, a.copy())                      # every cost is zero: row i meets column i first
    assert list(perm) == [0, 1, 2] and cost == 0.0


@pytest.mark.parametrize("n", [13, 38, 64, 65, 200])
def test_assignment_cost_matches_scipy(n):
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(n)
    a, b = at.ball_points(rng, n), at.ball_points(rng, n)
    c = at.cost_matrix(a, b)
    perm, cost = at.assign(a, b)
    rows, cols = optimize.linear_sum_assignment(c)
    ref = c[rows, cols].sum()
    assert abs(cost - ref) <= 1e-13 * ref, (n, cost, ref)
    assert np.array_equal(perm, cols)                        # random points: the optimum is unique


def test_cost_matrix_is_the_stated_fma_chain():
    rng = np.random.default_rng(7)
    a, b = at.ball_points(rng, 9), at.ball_points(rng, 9)
    c = at.cost_matrix(a, b)
    exact = ((a[:, None, :].astype(np.longdouble) - b[None, :, :].astype(np.longdouble)) ** 2).sum(axis=2)
    assert np.abs(c - exact).max() <= 4 * 2.0 ** -53 * exact.max()


def test_the_distance_never_increases_from_cycle_to_cycle():
    rng = np.random.default_rng(11)
    for n in (5, 13, 38):
        a, b = at.ball_points(rng, n), at.ball_points(rng, n)
        r = at.align(at.join(a), at.join(b), n, random_trials=4, seed=3)
        assert len(r.histories) == 9
        for h in r.histories:
            assert all(h[k + 1] <= h[k] * (1 + 1e-12) for k in range(len(h) - 1)), h
        assert r.distance == min(r.trial_distances) and r.best_trial == int(np.argmin(r.trial_distances))


def test_jacobi_and_horn_against_numpy():
    rng = np.random.default_rng(5)
    m = rng.standard_normal((4, 4))
    m = m + m.T
    e, v = at.jacobi(m)
    v = np.array(v)
    assert np.allclose(sorted(e), np.linalg.eigvalsh(m), atol=1e-13)
    assert np.allclose(v @ np.diag(e) @ v.T, m, atol=1e-13) and np.allclose(v.T @ v, np.eye(4), atol=1e-14)
    assert at.jacobi(np.zeros((3, 3)))[1] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    a = at.ball_points(rng, 20)
    rot = at.proper_rotation(rng)
    got = at.horn(a @ rot.T, a)                              # brings a onto R a
    assert np.allclose(got, rot, atol=1e-13) and abs(np.linalg.det(got) - 1) < 1e-13


def test_random_rotations_are_proper_and_follow_the_stream():
    for r in (0, 7, 63):
        rot = at.random_rotation(12345, r)
        assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(rot) - 1) < 1e-14
    assert not np.allclose(at.random_rotation(1, 0), at.random_rotation(1, 1))
    assert not np.allclose(at.random_rotation(1, 0), at.random_rotation(2, 0))
    # the jump-ahead is the stream: trial 1 starts four draws after trial 0
    state = at.pcg_state(9)
    _, after = at.pcg_raw(state, 4)
    assert at._jump(state, 4) == after and at._jump(state, 0) == state


@pytest.mark.parametrize("case", at.recovery_cases(), ids=lambda c: "n%d%s" % (c[0], "inv" if c[1] else ""))
def test_principal_starts_recover_a_planted_motion(case):
    """The permutation and the sign of the determinant are asked for where they are unique (``align_twin.two_answers``)."""
    n, inverted, a, b, planted = case
    r = at.align(a, b, n, trials=at.TRIAL_PRINCIPAL, random_trials=0, allow_inversion=inverted)
    scale = np.linalg.norm(a)
    assert r.distance <= 1e-13 * scale, (n, r.distance)
    perm_free, sign_free = at.two_answers(n, inverted)
    if not perm_free:
        assert np.array_equal(planted[r.perm], np.arange(n))
    if not sign_free:
        assert abs(np.linalg.det(r.rotation) - (-1.0 if inverted else 1.0)) < 1e-12
    assert abs(abs(np.linalg.det(r.rotation)) - 1.0) < 1e-12 and sorted(r.perm) == list(range(n))
    assert np.abs(r.aligned - a).max() <= 1e-13 * scale
    assert r.status == at.CONVERGED and r.cycles <= 5


def test_small_and_degenerate_sizes_give_finite_answers():
    for n in (1, 2):
        rng = np.random.default_rng(n)
        a, b = at.ball_points(rng, n), at.ball_points(rng, n)
        r = at.align(at.join(a), at.join(b), n, random_trials=2, allow_inversion=True)
        assert np.isfinite(r.distance) and np.isfinite(r.rotation).all() and np.isfinite(r.aligned).all()
    r = at.align(at.join(a), at.join(a), 2)
    assert r.distance <= 1e-15
    bad = at.join(a).copy()
    bad[0] = np.nan
    r = at.align(bad, at.join(b), 2)
    assert r.status == at.FAILED and np.isnan(r.distance) and list(r.perm) == [0, 1]


def test_the_icosahedron_needs_the_random_starts_and_the_committed_seed_serves():
    """Every second-moment eigenvalue of the icosahedron is the same, so its principal frame is arbitrary: the four principal
    starts alone are not enough in general, eight random ones with the committed seed recover every case."""
    for k, (a, b, planted) in enumerate(at.icosahedron_cases()):
        r = at.align(a, b, 13, random_trials=8, seed=at.ICOSAHEDRON_SEED)
        assert r.distance <= 1e-13 * np.linalg.norm(a), (k, r.distance, r.trial_distances)
        # the icosahedron maps onto itself in 60 ways: the permutation found is one of them, not necessarily the planted one
        assert np.abs(r.aligned - a).max() <= 1e-13 * np.linalg.norm(a)
