"""The alignment twin (tests/align_twin.py) checked against things it does not depend on: the brute-force minimum over all
permutations, scipy's assignment solver where scipy imports, the monotone decrease of the alternation, and the recovery of
planted rotations, translations, relabellings and inversions.  CPU only; the kernel is compared with the twin in
tests/test_gpu_align.py."""
import itertools
import math

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


# ------------------------------------------------------------------------------ exact assignment cases: integer coordinates
# Conditions on the inputs tests/test_gpu_align.py runs on the device: the optimum is known without the twin (closed form, scipy
# on an integer matrix, brute force), the twin finds it with ``==``, and the inputs do to the search what they are there for
# (the longest paths, ties at most scans, ties inside a lane and across lanes).
LINE_SIZES = (13, 64, 65, 256, 257)                          # 1024 (524 800 scans) is too slow for the suite; run once by hand: the reversal, no tie
EXACT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257)


def _exact(kind, n):
    a, b = at.exact_case(kind, n)
    assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)) and max(np.abs(a).max(), np.abs(b).max()) <= 1024
    assert np.array_equal(a.astype(np.float32), a) and np.array_equal(b.astype(np.float32), b)
    c = at.cost_matrix(a, b)
    assert np.array_equal(c, ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))
    return a, b, c


@pytest.mark.parametrize("n", LINE_SIZES)
def test_line_has_the_closed_form_and_the_longest_paths(n):
    _, _, c = _exact("line", n)
    perm, u, v, seen = at.assign_costs(c, count=True)
    assert np.array_equal(perm, np.arange(n)[::-1])
    for order in ("index", "device"):
        assert at.matched_cost(c, perm, order) == at.line_cost(n) == n * (n + 1) ** 2
    assert np.array_equal(seen["scans"], np.arange(1, n + 1)) and seen["longest"] == n and seen["total"] == n * (n + 1) // 2
    assert seen["tied"] == 0
    assert np.array_equal(u, np.rint(u)) and np.array_equal(v, np.rint(v)) and max(np.abs(u).max(), np.abs(v).max()) < 2.0 ** 53
    optimize = pytest.importorskip("scipy.optimize")
    rows, cols = optimize.linear_sum_assignment(c)
    assert np.array_equal(cols, perm) and c[rows, cols].sum() == at.line_cost(n)


@pytest.mark.parametrize("n", EXACT_SIZES + (1024,))
def test_lattice_cost_is_scipys_and_most_scans_tie(n):
    _, _, c = _exact("lattice", n)
    perm, _, _, seen = at.assign_costs(c, count=True)
    assert sorted(perm) == list(range(n))
    if n >= 64:                                              # a floor on the input, not a measurement: 0.81 at 64, 0.87 at 256, 0.96 at 1024
        assert seen["tied"] >= 0.5 * seen["total"], seen
        assert seen["longest"] >= n // 2, seen
    optimize = pytest.importorskip("scipy.optimize")
    rows, cols = optimize.linear_sum_assignment(c)
    for order in ("index", "device"):
        assert at.matched_cost(c, perm, order) == c[rows, cols].sum(), (n, order)


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_all_tie_gives_the_identity_and_every_scan_ties(n):
    a, b, c = _exact("all_tie", n)
    assert (b == b[0]).all()
    perm, _, _, seen = at.assign_costs(c, count=True)
    assert np.array_equal(perm, np.arange(n))
    assert seen["total"] == n * (n + 1) // 2 and seen["longest"] == n
    assert seen["tied"] == seen["total"] - 1                 # all but the last scan, where one column is left
    for order in ("index", "device"):
        assert at.matched_cost(c, perm, order) == ((a - b) ** 2).sum()


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_lane_tie_cost_is_scipys_and_columns_of_one_lane_tie(n):
    _, b, c = _exact("lane_tie", n)
    if n > 64:
        assert np.array_equal(b[64:], b[:-64]) and np.array_equal(c[:, 64:], c[:, :-64])      # l and l + 64 q: one point
    m = min(n, 64)
    assert n <= 7 or np.array_equal(b[7:m, 0], b[:m - 7, 0])                                 # lanes l and l + 7 likewise
    perm, _, _, seen = at.assign_costs(c, count=True)
    assert sorted(perm) == list(range(n))
    if n >= 63:
        assert seen["tied"] >= 0.5 * seen["total"], seen
    optimize = pytest.importorskip("scipy.optimize")
    rows, cols = optimize.linear_sum_assignment(c)
    for order in ("index", "device"):
        assert at.matched_cost(c, perm, order) == c[rows, cols].sum(), (n, order)


@pytest.mark.parametrize("kind", at.EXACT_KINDS)
@pytest.mark.parametrize("n", range(1, 8))
def test_exact_cases_are_the_brute_force_minimum(n, kind):
    _, _, c = _exact(kind, n)
    perm, _, _ = at.assign_costs(c)
    assert at.matched_cost(c, perm) == at.matched_cost(c, perm, "device") == _brute(c), (kind, n)


# ------------------------------------------------------------------------------ the device's order of the sums
def _wave_sum_by_the_rule(terms):
    """the header's rule in python floats, written without the twin's helpers"""
    lanes = [0.0] * 64
    for j, t in enumerate(terms):                            # ascending j: a lane meets l, l + 64, ... in that order
        lanes[j % 64] = lanes[j % 64] + float(t)
    for offset in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ offset] for l in range(64)]
    assert len(set(lanes)) == 1
    return lanes[0]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 257, 1024])
def test_wave_sum_is_the_headers_order_and_differs_from_the_index_order(n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    got = at.wave_sum(v)
    assert got == at.particle_sum(v, "device") == _wave_sum_by_the_rule(v)
    assert abs(got - math.fsum(v)) <= n * 2.0 ** -53 * np.abs(v).sum()
    assert at.particle_sum(v, "index") == at.seq_sum(v)
    if n >= 4:                                               # told apart: lanes 1 and 3 meet before they meet lane 0
        w = np.zeros(n)
        w[0], w[1], w[3] = 1.0, 2.0 ** -53, 2.0 ** -53
        assert at.seq_sum(w) == 1.0 and at.wave_sum(w) == 1.0 + 2.0 ** -52
    if n >= 129:                                             # ... and a lane adds its own columns first
        w = np.zeros(n)
        w[0], w[64], w[128] = 2.0 ** -53, 2.0 ** -53, 1.0
        assert at.wave_sum(w) == 1.0 + 2.0 ** -52
        w[0], w[128] = 1.0, 2.0 ** -53
        assert at.wave_sum(w) == 1.0
    with pytest.raises(AssertionError):
        at.particle_sum(v, "lane")


def test_device_order_changes_the_sums_and_nothing_else():
    """order="device" permutes the terms of every sum: the same permutations, statuses and cycle counts as "index" on
    unrelated pairs, every distance within rounding, and not the same bits (or the option would do nothing)."""
    rng = np.random.default_rng(21)
    different = 0
    for n in (13, 65, 130):
        a, b = at.join(at.ball_points(rng, n)), at.join(at.ball_points(rng, n))
        options = dict(random_trials=2, seed=n, allow_inversion=True, max_cycles=20)
        ri, rd = at.align(a, b, n, **options), at.align(a, b, n, order="device", **options)
        assert np.array_equal(ri.perm, rd.perm) and (ri.best_trial, ri.cycles, ri.status) == (rd.best_trial, rd.cycles, rd.status)
        assert np.abs(ri.trial_distances - rd.trial_distances).max() <= 1e-13 * ri.distance
        assert np.abs(ri.rotation - rd.rotation).max() <= 1e-13 and np.abs(ri.aligned - rd.aligned).max() <= 1e-13
        different += int(not np.array_equal(ri.trial_distances, rd.trial_distances))
        pa, pb = at.split(a, n), at.split(b, n)
        perm, cost = at.assign(pa, pb)
        perm_d, cost_d = at.assign(pa, pb, "device")
        assert np.array_equal(perm, perm_d) and abs(cost - cost_d) <= 1e-13 * cost
        c = at.cost_matrix(pa, pb)
        assert cost_d == _wave_sum_by_the_rule(c[at.inverse(perm), np.arange(n)])           # the term of column j is c(rowof[j], j)
    assert different == 3


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
