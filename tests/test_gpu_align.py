"""The alignment unit on the device (csrc/dzo_align.hip) against its CPU twin (tests/align_twin.py) and against properties that
need no twin.

Tolerances.  Every comparison is allowed ``FACTOR * RATIO[T] * eps_T * |A|_F`` (|A|_F the Frobenius norm of the pair's first
point, eps_T the spacing of T at 1).  RATIO[T] is not taken from the kernel: it is the largest error, in units of
eps_T |A|_F, that the TWIN shows on this file's own inputs where the truth is known (the planted motions of the recovery cases:
its distance from zero and its aligned point from ``a``; the assignment cost against the same matched costs summed in
longdouble), found by ``measure_twin_ratios()`` on the CPU and recorded next to the constants.  FACTOR = 8 because the
kernel's sums run lane by lane and up the wave tree, the twin's in index order.

MEASURED on an MI355X (every test prints its figures with ``-s``): every permutation, winning start, cycle count and status
equals the twin's.  Assignment costs differ from the twin's by at most 1.2e-14 (0.12 of what is allowed).  Planted motions: the
distance is at most 5.2e-15 in float64 and 1.1e-06 in float32 (0.12 of the allowed), the aligned point within 0.06 of the allowed,
two cycles everywhere; the icosahedron within 0.09.  Unrelated pairs: distances, trial distances and rotation elements within
1.3e-15 of the twin's in both element types (0.03 of the allowed in float64), 2 to 11 cycles.
The frame-and-labels property and the consumer hold at the plain bound: the two distances differ by at most 0.009 of the
allowed in float64 and 0.012 in float32 (the twin itself, on the same inputs: 0.81 and 0.076 in units of eps_T |A|_F, below
RATIO), the consumer's by at most 0.015.  Energies and fingerprints of the aligned point: the rounding bound, read as how far
the point may move and carried to an energy through its gradient, is wide in that role: seen / allowed is at most 0.0025 (E),
0.003 (e_i) and 0.008 (d_i).  The sharp check of "a rigid motion and a relabelling" is the direct one next to it: the aligned
point against the returned rotation applied to the returned permutation of b, within the arithmetic's own rounding
(seen / allowed 0.0085 in float64, 0.59 in float32, where the one rounding to T is nearly all of it), the rotation orthogonal
with determinant 1 to 16 eps.

No tolerance at all in the second half of the file.  The exact assignment cases have integer coordinates, so the optimum cost is
a known integer and the device returns it with ``==``.  The replays (deterministic starts, the cycle limit, the ten fixed starts
among all 138) compare every float as a bit pattern with the twin run with ``order="device"``: the header states every sum order,
fma and tie rule, the library is built without contraction, and only the random starts call functions (log, cospi, sinpi) that no
header pins, so those are compared device against device.  MEASURED: every one of them holds as written; with the lower-column
rule of the wave argmin flipped the exact cases fail from N = 2 on (``all_tie``, then ``lattice``) while every test of the first
half still passes, and with Horn's nine sums taken in another association the replays fail from N = 3 on while, again, every
test of the first half passes.

Where a planted motion has two exact answers (``align_twin.two_answers``: a pair of points is swapped by a half turn; up to three
points are inverted by one) the permutation or the sign of the determinant is not asked for; everything else is.
"""
import functools
import subprocess
import time

import numpy as np
import pytest

import align_twin as at
import neb_twin as nb
import pairwise_twin as tw
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
EPS = {np.dtype(np.float64): 2.0 ** -52, np.dtype(np.float32): 2.0 ** -23}
FACTOR = 8.0
# measure_twin_ratios() on the CPU: the twin's largest error / (eps_T |A|_F) over the recovery cases below (distance and aligned
# point; in float32 the inputs themselves are rounded, which is what the figure shows) and over the assignment cases (cost)
RATIO = {np.dtype(np.float64): 5.89, np.dtype(np.float32): 0.78}                # measured: 5.885 (fp64), 0.7775 (fp32)
# ... and of the assignment cost, whose arithmetic is fp64 whatever T is (so the float32 figure is tiny: 4.4 in units of 2^-52)
COST_RATIO = {np.dtype(np.float64): 4.73, np.dtype(np.float32): 8.2e-9}         # measured: 4.723 (fp64), 8.196e-09 (fp32)
ASSIGN_SIZES = (1, 2, 3, 13, 63, 64, 65, 255, 256, 257, 300)
RECOVERY_SIZES = at.RECOVERY_SIZES + (64, 256, 257)
UNRELATED_SIZES = (13, 38, 65)
UNRELATED_BATCH = 8
PRINCIPAL = at.TRIAL_PRINCIPAL


def _bound(dtype, a, ratio=RATIO):
    return FACTOR * ratio[np.dtype(dtype)] * EPS[np.dtype(dtype)] * float(np.linalg.norm(np.asarray(a, dtype=np.float64)))


def _dev(x, dtype):
    return dzo.DeviceArray.from_host(np.ascontiguousarray(x, dtype=dtype))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


# ------------------------------------------------------------------------------ inputs and the twin on them, computed once
@functools.lru_cache(maxsize=None)
def _assign_inputs(n, dtype):
    rng = np.random.default_rng(7000 + n)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(5)]).astype(dtype)
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(5)]).astype(dtype)
    twin = [at.assign(at.split(a[k], n), at.split(b[k], n)) for k in range(5)]
    return a, b, twin


@functools.lru_cache(maxsize=None)
def _recovery_inputs(dtype):
    """[(n, inverted, a, b, planted)] rounded to dtype"""
    return [(n, inv, a.astype(dtype), b.astype(dtype), planted) for n, inv, a, b, planted in at.recovery_cases(RECOVERY_SIZES)]


@functools.lru_cache(maxsize=None)
def _unrelated_inputs(n, dtype):
    rng = np.random.default_rng(4242 + n)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(UNRELATED_BATCH)]).astype(dtype)
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(UNRELATED_BATCH)]).astype(dtype)
    twin = [at.align(a[k], b[k], n, random_trials=8, seed=n) for k in range(UNRELATED_BATCH)]
    return a, b, twin


def _close_seconds(twin):
    """the twin's two best starts lie within 1e-9 relative of each other: which one wins is then a matter of rounding"""
    d = np.sort(twin.trial_distances)
    return len(d) > 1 and d[1] - d[0] <= 1e-9 * d[1]


def measure_twin_ratios():
    """What RATIO records; CPU only.  Returns {dtype name: (recovery ratio, assignment ratio)}."""
    out = {}
    for dtype in DTYPES:
        dt = np.dtype(dtype)
        worst = 0.0
        for n, inv, a, b, planted in _recovery_inputs(dtype):
            r = at.align(a, b, n, trials=PRINCIPAL, random_trials=0, allow_inversion=inv)
            scale = EPS[dt] * np.linalg.norm(a.astype(np.float64))
            worst = max(worst, r.distance / scale, np.abs(r.aligned - a.astype(np.float64)).max() / scale)
        for a, b, planted in at.icosahedron_cases():
            a, b = a.astype(dtype), b.astype(dtype)
            r = at.align(a, b, 13, random_trials=8, seed=at.ICOSAHEDRON_SEED)
            scale = EPS[dt] * np.linalg.norm(a.astype(np.float64))
            worst = max(worst, r.distance / scale, np.abs(r.aligned - a.astype(np.float64)).max() / scale)
        cost = 0.0
        for n in ASSIGN_SIZES:
            a, b, twin = _assign_inputs(n, dtype)
            for k in range(5):
                pa, pb = at.split(a[k], n).astype(np.longdouble), at.split(b[k], n).astype(np.longdouble)
                exact = ((pa - pb[twin[k][0]]) ** 2).sum()
                cost = max(cost, float(abs(twin[k][1] - exact)) / (EPS[dt] * np.linalg.norm(a[k].astype(np.float64))))
        out[dt.name] = (worst, cost)
    return out


# ------------------------------------------------------------------------------ assign
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ASSIGN_SIZES)
def test_assignment_equals_the_twin(n, dtype):
    a, b, twin = _assign_inputs(n, dtype)
    perm, cost = dzo.assign_particles(_dev(a, dtype), _dev(b, dtype), n)
    assert perm.shape == (5, n) and perm.dtype == np.int32 and cost.dtype == np.float64
    for k in range(5):
        assert np.array_equal(perm[k], twin[k][0]), (n, k)
        allowed = _bound(dtype, a[k], COST_RATIO)
        print(n, k, "cost", cost[k], "twin", twin[k][1], "seen", abs(cost[k] - twin[k][1]), "allowed", allowed)
        assert abs(cost[k] - twin[k][1]) <= allowed, (n, k, cost[k], twin[k][1])


# ------------------------------------------------------------------------------ recovery of planted motions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(2 * len(RECOVERY_SIZES)))
def test_a_planted_motion_is_recovered(index, dtype):
    n, inverted, a, b, planted = _recovery_inputs(dtype)[index]
    r = dzo.align_pairs(_dev(a[None], dtype), _dev(b[None], dtype), n, trials=PRINCIPAL, random_trials=0, allow_inversion=inverted)
    allowed = _bound(dtype, a)
    aligned = r.aligned.to_host()[0]
    print(n, inverted, "distance", r.distances[0], "aligned", np.abs(aligned.astype(np.float64) - a).max(), "allowed", allowed, "cycles", r.cycles[0])
    assert r.status[0] == dzo.ALIGN_CONVERGED
    assert r.distances[0] <= allowed
    # one more rounding to T in the aligned point
    assert np.abs(aligned.astype(np.float64) - a.astype(np.float64)).max() <= allowed + EPS[np.dtype(dtype)] * np.abs(a).max()
    det = np.linalg.det(r.rotations[0])
    perm_free, sign_free = at.two_answers(n, inverted)       # where a planted motion has two exact answers
    if not perm_free:
        assert np.array_equal(planted[r.permutations[0]], np.arange(n))
    if not sign_free:
        assert abs(det - (-1.0 if inverted else 1.0)) < 1e-9
    assert abs(abs(det) - 1.0) < 1e-9 and sorted(r.permutations[0]) == list(range(n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_icosahedron_is_recovered_with_the_committed_seed(dtype):
    cases = at.icosahedron_cases()
    a = np.stack([c[0] for c in cases]).astype(dtype)
    b = np.stack([c[1] for c in cases]).astype(dtype)
    r = dzo.align_pairs(_dev(a, dtype), _dev(b, dtype), 13, random_trials=8, seed=at.ICOSAHEDRON_SEED, want_trials=True)
    aligned = r.aligned.to_host()
    for k in range(len(cases)):
        allowed = _bound(dtype, a[k])
        print(k, "distance", r.distances[k], "allowed", allowed, "best", r.best_trials[k], "trials", r.trial_distances[k])
        assert r.distances[k] <= allowed
        assert np.abs(aligned[k].astype(np.float64) - a[k]).max() <= allowed + EPS[np.dtype(dtype)] * np.abs(a[k]).max()


def test_large_n_planted_permutation():
    """N = 1024, the cheap path of the largest instantiation: B is a rotated, shifted, relabelled copy of A plus noise 1e-3."""
    n = 1024
    rng = np.random.default_rng(1024)
    a, b, plants = [], [], []
    for _ in range(2):
        p = at.ball_points(rng, n)
        q, planted = at.scramble(p, rng)
        a.append(at.join(p)); b.append(at.join(q + 1e-3 * rng.standard_normal(q.shape))); plants.append(planted)
    r = dzo.align_pairs(_dev(np.stack(a), np.float64), _dev(np.stack(b), np.float64), n, trials=PRINCIPAL, random_trials=0)
    print("distances", r.distances, "cycles", r.cycles, "best", r.best_trials)
    for k in range(2):
        assert np.array_equal(plants[k][r.permutations[k]], np.arange(n)), k
        assert r.status[k] == dzo.ALIGN_CONVERGED and r.distances[k] < 2e-3 * np.sqrt(3 * n) * 3


# ------------------------------------------------------------------------------ unrelated pairs against the twin
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", UNRELATED_SIZES)
def test_unrelated_pairs_against_the_twin(n, dtype):
    a, b, twin = _unrelated_inputs(n, dtype)
    r = dzo.align_pairs(_dev(a, dtype), _dev(b, dtype), n, random_trials=8, seed=n, want_trials=True)
    for k in range(UNRELATED_BATCH):
        t, allowed = twin[k], _bound(dtype, a[k])
        seen = max(abs(r.distances[k] - t.distance), np.abs(r.trial_distances[k] - t.trial_distances).max(), np.abs(r.rotations[k] - t.rotation).max())
        print(n, k, "distance", r.distances[k], "twin", t.distance, "seen", seen, "allowed", allowed, "cycles", r.cycles[k], "best", r.best_trials[k])
        assert abs(r.distances[k] - t.distance) <= allowed, (n, k)
        if _close_seconds(t):
            continue
        assert (r.best_trials[k], r.cycles[k], r.status[k]) == (t.best_trial, t.cycles, t.status), (n, k)
        assert np.array_equal(r.permutations[k], t.perm), (n, k)
        assert np.abs(r.trial_distances[k] - t.trial_distances).max() <= allowed, (n, k)
        assert np.abs(r.rotations[k] - t.rotation).max() <= allowed, (n, k)


def test_few_unrelated_pairs_fall_under_the_exemption():
    """CPU arithmetic only (it sits here because it is about this file's inputs): at most 5 % of the pairs above have two best
    starts within 1e-9 relative of each other."""
    cases = [t for dtype in DTYPES for n in UNRELATED_SIZES for t in _unrelated_inputs(n, dtype)[2]]
    exempt = sum(_close_seconds(t) for t in cases)
    assert exempt <= 0.05 * len(cases), (exempt, len(cases))


# ------------------------------------------------------------------------------ properties that need no twin
def _energy_allowed(x, n, dtype, move):
    """How far the energy E and a per-particle energy e_i of the point x may change when the whole point moves by at most
    `move` in the 2-norm and both energies are evaluated in T.  First order in the move: |dE| <= |g|_2 |dx|_2, and
    |de_i| <= sum_j |phi'(r_ij)| |dr_ij| with |dr_ij| <= |dx_i| + |dx_j| <= sqrt(2) |dx|_2.  The rounding of an energy is the
    project's derived bound of tests/test_gpu_pairwise.py, (N + 32) u S with S the sum of the absolute pair terms, once for
    each of the two energies compared.  Returns (allowed for E, allowed for e_i)."""
    p = at.split(x, n)
    d = p[:, None, :] - p[None, :, :]
    off = 1 - np.eye(n)
    r2 = (d * d).sum(axis=2) + np.eye(n)
    i6 = 1.0 / r2 ** 3
    slope = (-48.0 * i6 * i6 + 24.0 * i6) / r2 * off         # phi'(r) / r
    g2 = np.linalg.norm((slope[:, :, None] * d).sum(axis=1))
    steepest = (np.abs(slope) * np.sqrt(r2)).sum(axis=1).max()
    mag = 4.0 * (i6 * i6 + i6) * off
    u = 0.5 * EPS[np.dtype(dtype)]
    return g2 * move + 2 * (n + 32) * u * 0.5 * mag.sum(), np.sqrt(2.0) * steepest * move + 2 * (n + 32) * u * mag.sum(axis=1).max()


@pytest.mark.parametrize("dtype", DTYPES)
def test_properties_that_need_no_twin(dtype):
    n, batch = 38, 6
    dt = np.dtype(dtype)
    a = np.stack([np.concatenate(tw.lattice(n, seed=300 + k)) for k in range(batch)]).astype(dtype)
    b = np.stack([np.concatenate(tw.lattice(n, seed=400 + k)) for k in range(batch)]).astype(dtype)
    da, db = _dev(a, dtype), _dev(b, dtype)
    r = dzo.align_pairs(da, db, n, random_trials=4, seed=1, want_trials=True)
    assert r.trial_distances.shape == (batch, 9)
    for k in range(batch):
        assert r.distances[k] == r.trial_distances[k].min() and r.best_trials[k] == int(np.argmin(r.trial_distances[k]))
        pa, pb = at.split(a[k], n), at.split(b[k], n)
        raw = np.sqrt((((pa - pa.mean(axis=0)) - (pb - pb.mean(axis=0))) ** 2).sum())
        assert r.distances[k] <= raw + _bound(dtype, a[k]), (k, r.distances[k], raw)
        assert r.trial_distances[k, 0] <= raw + _bound(dtype, a[k])     # the identity start: its first assignment cannot be worse
    # the outputs belong together: aligned IS the rotation applied to the relabelled, centred b, moved to a's centroid.  The bound
    # is the arithmetic's own: three products and three sums in fp64 per coordinate on values up to |b| + |c_B| and |c_A|, the
    # centroids N-term fp64 sums in another order than numpy's, and one rounding to T
    aligned = r.aligned.to_host().astype(np.float64)
    for k in range(batch):
        pa, pb = at.split(a[k], n), at.split(b[k], n)
        rot, perm = r.rotations[k], r.permutations[k]
        assert sorted(perm) == list(range(n)) and np.abs(rot @ rot.T - np.eye(3)).max() <= 16 * EPS[np.dtype(np.float64)]
        assert abs(np.linalg.det(rot) - 1.0) <= 16 * EPS[np.dtype(np.float64)]
        image = (pb[perm] - pb.mean(axis=0)) @ rot.T + pa.mean(axis=0)
        size = 2 * np.abs(pb).max() + np.abs(pa).max()
        allowed_x = (n + 8) * EPS[np.dtype(np.float64)] * size + 0.5 * EPS[dt] * np.abs(image).max()
        seen_x = np.abs(at.split(aligned[k], n) - image).max()
        print(k, "aligned against its own rotation and permutation: seen / allowed %.3g" % (seen_x / allowed_x), "allowed", allowed_x)
        assert seen_x <= allowed_x, (k, seen_x, allowed_x)
    # a rigid motion and a relabelling change neither the energy nor the fingerprint beyond rounding
    fp_b, e_b = dzo.structure_fingerprints(db, n)
    fp_x, e_x = dzo.structure_fingerprints(r.aligned, n)
    e_x2 = dzo.pairwise_batch_energy_gradient(r.aligned, n)
    fp_b, fp_x = fp_b.to_host().astype(np.float64), fp_x.to_host().astype(np.float64)
    for k in range(batch):
        # the aligned point may sit the rounding bound away from the exact image of b (2-norm), and is rounded to T once more
        move = _bound(dtype, b[k]) + EPS[dt] * max(np.linalg.norm(a[k].astype(np.float64)), np.linalg.norm(b[k].astype(np.float64)))
        allowed_e, allowed_ei = _energy_allowed(b[k], n, dtype, move)
        pb = at.split(b[k], n)
        radius = np.linalg.norm(pb - pb.mean(axis=0), axis=1).max()
        # d_i = |x_i - c|^2: particle and centroid move by at most `move` each; three squares and two sums in T
        allowed_d = 4 * (radius + move) * move + 8 * EPS[dt] * radius ** 2
        seen = (abs(float(e_x[k]) - float(e_b[k])), np.abs(fp_x[k, :n] - fp_b[k, :n]).max(), np.abs(fp_x[k, n:] - fp_b[k, n:]).max())
        print(k, "seen / allowed: E %.3g" % (seen[0] / allowed_e), "e_i %.3g" % (seen[1] / allowed_ei), "d_i %.3g" % (seen[2] / allowed_d),
              "allowed", allowed_e, allowed_ei, allowed_d)
        assert seen[0] <= allowed_e and float(e_x2[k]) == float(e_x[k])
        assert seen[1] <= allowed_ei
        assert seen[2] <= allowed_d


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_distance_does_not_depend_on_the_frame_and_labels_of_b(dtype):
    """trials = PRINCIPAL alone: align(A, B) and align(A, R B[p] + t) give the same distance, for inputs whose moment
    eigenvalues are separated (asserted here on the twin's frames)."""
    n, batch = 38, 5
    rng = np.random.default_rng(99)
    a, b, b2 = [], [], []
    for _ in range(batch):
        pa, pb = at.ball_points(rng, n), at.ball_points(rng, n)
        for p in (pa, pb):
            e = at.principal_frame(p - p.mean(axis=0))[1]
            assert min(e[1] - e[0], e[2] - e[1]) > 1e-2 * e[2]
        q, _ = at.scramble(pb, rng)
        a.append(at.join(pa)); b.append(at.join(pb)); b2.append(at.join(q))
    a, b, b2 = (np.stack(v).astype(dtype) for v in (a, b, b2))
    da = _dev(a, dtype)
    r1 = dzo.align_pairs(da, _dev(b, dtype), n, trials=PRINCIPAL, random_trials=0)
    r2 = dzo.align_pairs(da, _dev(b2, dtype), n, trials=PRINCIPAL, random_trials=0)
    for k in range(batch):
        allowed = _bound(dtype, a[k])
        print(k, r1.distances[k], r2.distances[k], "seen / allowed %.3g" % (abs(r1.distances[k] - r2.distances[k]) / allowed), "allowed", allowed)
        assert abs(r1.distances[k] - r2.distances[k]) <= allowed, k


# ------------------------------------------------------------------------------ batch independence, refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_pair_computes_the_same_bits_alone_and_in_a_batch(dtype):
    n, batch = 38, 37
    rng = np.random.default_rng(37)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)]).astype(dtype)
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)]).astype(dtype)
    options = dict(random_trials=3, seed=5, allow_inversion=True, want_trials=True)
    whole = dzo.align_pairs(_dev(a, dtype), _dev(b, dtype), n, **options)
    whole_x = whole.aligned.to_host()
    whole_p, whole_c = dzo.assign_particles(_dev(a, dtype), _dev(b, dtype), n)
    for k in (0, 17, 36):
        one = dzo.align_pairs(_dev(a[k:k + 1], dtype), _dev(b[k:k + 1], dtype), n, **options)
        assert np.array_equal(_bits(one.aligned.to_host()[0]), _bits(whole_x[k]))
        assert np.array_equal(one.permutations[0], whole.permutations[k])
        for name in ("rotations", "distances", "trial_distances"):
            assert np.array_equal(_bits(getattr(one, name)[0]), _bits(getattr(whole, name)[k])), (k, name)
        assert (one.best_trials[0], one.cycles[0], one.status[0]) == (whole.best_trials[k], whole.cycles[k], whole.status[k])
        p, c = dzo.assign_particles(_dev(a[k:k + 1], dtype), _dev(b[k:k + 1], dtype), n)
        assert np.array_equal(p[0], whole_p[k]) and np.array_equal(_bits(c), _bits(whole_c[k:k + 1]))


def test_refusals():
    n, batch = 13, 4
    rng = np.random.default_rng(3)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)])
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)])
    good = dzo.align_pairs(_dev(a, np.float64), _dev(b, np.float64), n, want_trials=True)
    bad = b.copy()
    bad[2, 5] = np.nan
    r = dzo.align_pairs(_dev(a, np.float64), _dev(bad, np.float64), n, want_trials=True)
    assert r.status[2] == dzo.ALIGN_FAILED and np.isnan(r.distances[2]) and np.isnan(r.trial_distances[2]).all()
    assert r.permutations[2].tolist() == list(range(n)) and r.cycles[2] == 0 and r.best_trials[2] == 0
    assert np.array_equal(_bits(r.aligned.to_host()[2]), _bits(bad[2])) and np.array_equal(r.rotations[2], np.eye(3))
    good_x, r_x = good.aligned.to_host(), r.aligned.to_host()
    for k in (0, 1, 3):                                      # the neighbours are untouched
        assert np.array_equal(_bits(r_x[k]), _bits(good_x[k])) and np.array_equal(r.permutations[k], good.permutations[k])
        assert np.array_equal(_bits(r.distances[k:k + 1]), _bits(good.distances[k:k + 1])) and r.status[k] == good.status[k]
    inf = a.copy()
    inf[1, 0] = np.inf
    p, c = dzo.assign_particles(_dev(inf, np.float64), _dev(b, np.float64), n)
    assert p[1].tolist() == list(range(n)) and np.isnan(c[1]) and np.isfinite(c[[0, 2, 3]]).all()
    L = dzo.lib()
    da, db = _dev(a, np.float64), _dev(b, np.float64)
    out = [dzo.DeviceArray(batch * 3 * n, np.float64) for _ in range(7)]

    def call(n_particles=n, dtype=dzo.F64, trials=3, random_trials=8, max_cycles=20, a_ptr=da.ptr):
        return L.dzo_align_batch_pairs(n_particles, 1, dtype, a_ptr, db.ptr, trials, random_trials, max_cycles, 0, 0, *[o.ptr for o in out], None)

    assert call() == 0
    assert call(n_particles=1025) == 5 and call(random_trials=65) == 5 and call(max_cycles=65) == 5      # DZO_ERR_UNSUPPORTED
    assert call(trials=0, random_trials=0) == 1 and call(n_particles=0) == 1 and call(dtype=9) == 1       # DZO_ERR_INVALID
    assert call(trials=4) == 1 and call(max_cycles=0) == 1 and call(a_ptr=None) == 1
    assert L.dzo_align_batch_assign(1025, 1, dzo.F64, da.ptr, db.ptr, out[0].ptr, out[1].ptr) == 5
    assert L.dzo_align_batch_assign(n, 0, dzo.F64, da.ptr, db.ptr, out[0].ptr, out[1].ptr) == 1
    host = np.zeros(3 * n)
    assert call(a_ptr=host.ctypes.data) == 3                                                           # DZO_ERR_ASSERT
    with pytest.raises(AssertionError, match="must hold 3 \\* n_particles \\* batch elements"):
        dzo.align_pairs(da, dzo.DeviceArray(3 * n, np.float64), n)


# ------------------------------------------------------------------------------ exact assignment cases: known integer costs, no tolerance
EXACT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
TWIN_LIMIT = 257                                             # above it the twin runs only the kinds whose answer has no closed form


@functools.lru_cache(maxsize=None)
def _exact_inputs(n):
    """(a, b, [(kind, permutation, cost)]) of the four exact kinds at one size, fp64; exact in fp32 too.  The cost is the known
    integer: the closed form of ``line``, sum |a_i - b_0|^2 of ``all_tie``, the twin's for the other two (scipy's, asserted in
    tests/test_align_twin.py up to 257 and for ``lattice`` at 1024, and again here where scipy imports).  The permutation is the
    twin's.  ``line`` and ``all_tie`` take n (n + 1) / 2 scans, half a million at 1024 and many seconds each in the twin, so above TWIN_LIMIT their
    permutation is the closed form that tests/test_align_twin.py shows the twin to return (the reversal: the optimum is
    unique; the identity: the lowest-column rule on equal slacks)."""
    cases, a, b = [], [], []
    for kind in at.EXACT_KINDS:
        pa, pb = at.exact_case(kind, n)
        c = at.cost_matrix(pa, pb)
        closed = {"line": np.arange(n)[::-1], "all_tie": np.arange(n)}.get(kind)
        perm = closed if closed is not None and n > TWIN_LIMIT else at.assign_costs(c)[0]
        if closed is not None:
            assert np.array_equal(perm, closed), (kind, n)
        cost = at.matched_cost(c, perm, "device")
        assert cost == float(c[np.arange(n), perm].astype(np.int64).sum()) and (kind != "line" or cost == at.line_cost(n))
        try:
            from scipy import optimize
            rows, cols = optimize.linear_sum_assignment(c)
            assert cost == c[rows, cols].sum(), (kind, n)
        except ImportError:
            pass
        cases.append((kind, perm, cost))
        a.append(at.join(pa)); b.append(at.join(pb))
    return np.stack(a), np.stack(b), cases


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_assignment_cases(n, dtype):
    """Integer coordinates: every cost, potential and slack is an exact integer, so the optimum cost is one too and the device
    returns it with ``==`` in both element types; the permutation is the twin's, tie rules included.  One batch of
    (line, lattice, all_tie, lane_tie) per size.  ``line`` and ``all_tie`` put the loops ``step <= N`` and ``k <= N`` at their
    bound (row i scans i + 1 times: 524 800 scans at 1024 by one wave of the Q = 16 form), ``all_tie`` ties all unvisited columns
    at every scan, ``lane_tie`` ties the columns l + 64 q of a lane and seven classes of lanes, ``lattice`` ties at four scans
    in five on paths nearly N long.
    MEASURED on an MI355X (wall clock round the call, printed with ``-s``; the ``align_assign`` timer of ``dzo.profile_table``
    agrees to the millisecond): the batch of four takes 1.35 s at N = 1024 and at 1023 in either element type, 0.07 s at 257,
    0.04 s at 256, 0.003 s at 65.  Alone at N = 1024: ``line`` 1.37 s in float64 and 1.34 s in float32 (2.6 us a scan),
    ``all_tie`` 1.31 s, ``lane_tie`` 0.66 s (231 204 scans), ``lattice`` 0.06 s (19 964 scans).  So ``line`` stays at every size
    in both element types.  The first case of a size also pays the twin once for both types: 2.5 s at 1023 and at 1024."""
    a, b, cases = _exact_inputs(n)
    assert np.array_equal(a.astype(dtype), a) and np.array_equal(b.astype(dtype), b)
    da, db = _dev(a, dtype), _dev(b, dtype)
    start = time.perf_counter()
    perm, cost = dzo.assign_particles(da, db, n)
    seconds = time.perf_counter() - start
    print(n, np.dtype(dtype).name, "assign_particles of the four exact kinds: %.3f s" % seconds)
    for k, (kind, want_perm, want_cost) in enumerate(cases):
        print(" ", kind, "cost", cost[k], "exact", want_cost)
        assert np.array_equal(perm[k], want_perm), (kind, n)
        assert cost[k] == want_cost, (kind, n, cost[k], want_cost)


# ------------------------------------------------------------------------------ bit-for-bit replay of the deterministic starts
REPLAY_SIZES = (1, 2, 3, 13, 63, 64, 65, 255, 256, 257)
REPLAY_INVERTED = (13, 65, 257)
DETERMINISTIC = at.TRIAL_IDENTITY | at.TRIAL_PRINCIPAL


def _same_as_twin(r, k, t, dtype, trial_slots=None):
    """pair k of the Alignment r against the device-order twin t: floats as bit patterns, the rest as integers"""
    what = {}
    if r.trial_distances is not None:
        seen = r.trial_distances[k] if trial_slots is None else r.trial_distances[k][trial_slots]
        what["trial_distances"] = (seen, t.trial_distances)
    what["distances"] = (r.distances[k:k + 1], np.array([t.distance]))
    what["rotations"] = (r.rotations[k], np.asarray(t.rotation, dtype=np.float64))
    what["aligned"] = (r.aligned.to_host()[k], t.aligned.astype(dtype))      # the twin's fp64 value rounded once to T
    for name, (seen, want) in what.items():
        assert seen.dtype == want.dtype and np.array_equal(_bits(seen), _bits(want)), (name, k, seen, want)
    assert np.array_equal(r.permutations[k], t.perm), k
    if trial_slots is None:
        assert (r.best_trials[k], r.cycles[k], r.status[k]) == (t.best_trial, t.cycles, t.status), k


@functools.lru_cache(maxsize=None)
def _replay_inputs(n, dtype, batch=3, **options):
    rng = np.random.default_rng(5000 + n)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)]).astype(dtype)
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)]).astype(dtype)
    twin = [at.align(a[k], b[k], n, order="device", **options) for k in range(batch)]
    return a, b, twin


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", REPLAY_SIZES)
def test_deterministic_starts_replay_bit_for_bit(n, dtype):
    """The identity and the four principal starts use +, -, *, /, sqrt and the stated fma only, in a stated order: every
    output has the twin's bits (sums in the device's order).  No tolerance, and no exemption for close seconds: the best start
    of a bit-exact list is decided."""
    options = dict(trials=DETERMINISTIC, random_trials=0, max_cycles=20, allow_inversion=n in REPLAY_INVERTED)
    a, b, twin = _replay_inputs(n, dtype, **options)
    r = dzo.align_pairs(_dev(a, dtype), _dev(b, dtype), n, want_trials=True, **options)
    assert r.trial_distances.shape == (3, 10 if options["allow_inversion"] else 5)
    print(n, np.dtype(dtype).name, "cycles", r.cycles, "best", r.best_trials, "status", r.status)
    for k in range(3):
        _same_as_twin(r, k, twin[k], dtype)


@functools.lru_cache(maxsize=None)
def _largest_inputs(dtype):
    """one pair of N = 1024 that needs six cycles from the identity start (in the twin), so three end in CYCLE_LIMIT"""
    n = 1024
    rng = np.random.default_rng(1025)
    a = at.join(at.ball_points(rng, n)).astype(dtype)[None]
    b = at.join(at.ball_points(rng, n)).astype(dtype)[None]
    return a, b, [at.align(a[0], b[0], n, trials=at.TRIAL_IDENTITY, random_trials=0, max_cycles=3, order="device")]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_widest_form_replays_bit_for_bit_at_the_cycle_limit(dtype):
    """N = 1024, one unrelated pair, the identity start, three cycles: all sixteen columns of every lane and the 38 920-byte
    LDS layout run the full cycle (three dense assignments, three rotations), and the start ends in CYCLE_LIMIT with the
    rotation computed after the last assignment.
    MEASURED on an MI355X: 0.18 s in either element type (the ``align_starts`` timer: 180 ms; ``align_finish`` 0.01 ms); the
    twin takes 0.8 s.  Every field has the twin's bits."""
    n = 1024
    options = dict(trials=at.TRIAL_IDENTITY, random_trials=0, max_cycles=3)
    a, b, twin = _largest_inputs(dtype)
    da, db = _dev(a, dtype), _dev(b, dtype)
    start = time.perf_counter()
    r = dzo.align_pairs(da, db, n, want_trials=True, **options)
    print(np.dtype(dtype).name, "align_pairs at N = 1024, three cycles: %.3f s" % (time.perf_counter() - start))
    assert twin[0].status == at.CYCLE_LIMIT and r.status[0] == dzo.ALIGN_CYCLE_LIMIT and r.cycles[0] == 3
    _same_as_twin(r, 0, twin[0], dtype)


# ------------------------------------------------------------------------------ the cycle limit
CYCLE_LIMITS = (1, 2, 3, 64)


@functools.lru_cache(maxsize=None)
def _cycle_inputs(n, dtype):
    rng = np.random.default_rng(6100 + n)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(4)]).astype(dtype)
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(4)]).astype(dtype)
    twin = {m: [at.align(a[k], b[k], n, trials=at.TRIAL_IDENTITY, random_trials=0, max_cycles=m, order="device") for k in range(4)]
            for m in CYCLE_LIMITS}
    return a, b, twin


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [13, 65])
def test_the_cycle_limit_reports_the_last_assignment_and_the_rotation_after_it(n, dtype):
    """Four unrelated pairs, the identity start, max_cycles = 1, 2, 3 and 64.  In the twin the pairs of N = 13 converge in
    2, 4, 5, 3 cycles and those of N = 65 in 3, 5, 8, 3 (both element types): one pair of N = 13 converges in two, two of N = 65
    stay in CYCLE_LIMIT through three, and max_cycles = 3 produces both statuses in one batch at either size.  At the limit the permutation is the last cycle's and the rotation and
    the distance are computed after it, as the header states: all bit-equal to the device-order twin."""
    a, b, twin = _cycle_inputs(n, dtype)
    da, db = _dev(a, dtype), _dev(b, dtype)
    statuses = set()
    for m in CYCLE_LIMITS:
        r = dzo.align_pairs(da, db, n, trials=at.TRIAL_IDENTITY, random_trials=0, max_cycles=m, want_trials=True)
        print(n, np.dtype(dtype).name, "max_cycles", m, "cycles", r.cycles, "status", r.status)
        for k in range(4):
            t = twin[m][k]
            assert t.status == (at.CONVERGED if twin[64][k].cycles <= m else at.CYCLE_LIMIT) and t.cycles == min(m, twin[64][k].cycles)
            _same_as_twin(r, k, t, dtype)
            statuses.add((m, int(r.status[k])))
    assert {s for m, s in statuses if m == 1} == {dzo.ALIGN_CYCLE_LIMIT}              # one cycle has no previous permutation
    assert {s for m, s in statuses if m == 64} == {dzo.ALIGN_CONVERGED}
    assert (3, dzo.ALIGN_CYCLE_LIMIT) in statuses and (3, dzo.ALIGN_CONVERGED) in statuses


# ------------------------------------------------------------------------------ all 138 starts, and the stream rule
def test_all_138_starts_and_the_stream_rule():
    """The largest start count, 2 (1 + 4 + 64).  The ten deterministic starts (0 to 4, and 69 to 73 inverted) have the twin's
    bits; the winner is the first smallest of the device's own list; random trial r draws the same numbers with another trial
    count and for a pair alone (device against device: log, cospi and sinpi are pinned by no header); a call repeats itself."""
    n, batch, dtype = 13, 3, np.float64
    options = dict(trials=DETERMINISTIC, allow_inversion=True, max_cycles=20)
    a, b, twin = _replay_inputs(n, dtype, random_trials=0, **options)
    da, db = _dev(a, dtype), _dev(b, dtype)
    r = dzo.align_pairs(da, db, n, random_trials=64, seed=138, want_trials=True, **options)
    assert r.trial_distances.shape == (3, 138)
    fixed = np.r_[0:5, 69:74]
    x = r.aligned.to_host()
    for k in range(batch):
        assert np.array_equal(_bits(r.trial_distances[k][fixed]), _bits(twin[k].trial_distances)), k
        best = int(np.argmin(r.trial_distances[k]))          # the first index of the minimum
        assert r.best_trials[k] == best and _bits(r.distances[k:k + 1])[0] == _bits(r.trial_distances[k, best:best + 1])[0]
        if best in fixed:
            _same_as_twin(r, k, twin[k], dtype, trial_slots=fixed)
    assert len({tuple(_bits(r.trial_distances[k, 5:69])) for k in range(batch)}) == batch      # the random starts did run
    few = dzo.align_pairs(da, db, n, random_trials=3, seed=138, want_trials=True, **options)
    assert few.trial_distances.shape == (3, 16)
    for k in range(batch):
        for rr in range(3):                                  # orientation 5 + r, and its inverted copy
            assert _bits(few.trial_distances[k, 5 + rr:6 + rr])[0] == _bits(r.trial_distances[k, 5 + rr:6 + rr])[0], (k, rr)
            assert _bits(few.trial_distances[k, 13 + rr:14 + rr])[0] == _bits(r.trial_distances[k, 74 + rr:75 + rr])[0], (k, rr)
        assert np.array_equal(_bits(few.trial_distances[k][np.r_[0:5, 8:13]]), _bits(twin[k].trial_distances))
    other = dzo.align_pairs(da, db, n, random_trials=3, seed=139, want_trials=True, **options)
    assert not np.array_equal(_bits(other.trial_distances[:, 5:8]), _bits(few.trial_distances[:, 5:8]))   # the seed selects the stream
    for k in range(batch):
        one = dzo.align_pairs(_dev(a[k:k + 1], dtype), _dev(b[k:k + 1], dtype), n, random_trials=64, seed=138, want_trials=True, **options)
        assert np.array_equal(_bits(one.trial_distances[0]), _bits(r.trial_distances[k])), k
        assert np.array_equal(_bits(one.aligned.to_host()[0]), _bits(x[k])) and one.best_trials[0] == r.best_trials[k]
    again = dzo.align_pairs(da, db, n, random_trials=64, seed=138, want_trials=True, **options)
    for name in ("trial_distances", "distances", "rotations", "permutations", "best_trials", "cycles", "status"):
        assert np.array_equal(_bits(getattr(again, name)), _bits(getattr(r, name))), name
    assert np.array_equal(_bits(again.aligned.to_host()), _bits(x))


# ------------------------------------------------------------------------------ guard bands, untouched inputs
CANARY = 12345.0
GUARD = 64


def _guarded(shape, np_dtype):
    size = int(np.prod(shape))
    buf = dzo.DeviceArray.from_host(np.full(size + 2 * GUARD, CANARY, dtype=np_dtype))
    return buf, buf.view(GUARD, shape)


def _guards_hold(buffers):
    for name, (buf, window) in buffers.items():
        h = buf.to_host()
        assert np.all(h[:GUARD] == h.dtype.type(CANARY)) and np.all(h[-GUARD:] == h.dtype.type(CANARY)), name + ": wrote outside its output"
        assert not np.any(window.to_host() == h.dtype.type(CANARY)), name + ": an element of the output was not written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("want_trials", [True, False])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_outputs_stay_inside_their_windows_and_inputs_are_untouched(n, want_trials, dtype):
    """The C entry points with every output a window inside a larger array of canaries: no element outside a window changes,
    every element inside one is written, and a and b come back bit-identical ("neither is changed")."""
    batch, n_starts = 2, 2 * (1 + 4 + 2)
    rng = np.random.default_rng(8000 + n)
    a = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)]).astype(dtype)
    b = np.stack([at.join(at.ball_points(rng, n)) for _ in range(batch)]).astype(dtype)
    da, db = _dev(a, dtype), _dev(b, dtype)
    L = dzo.lib()
    out = {"aligned": _guarded((batch, 3 * n), dtype), "perm": _guarded((batch, n), np.int32), "rotation": _guarded((batch, 3, 3), np.float64),
           "distance": _guarded((batch,), np.float64), "best_trial": _guarded((batch,), np.int32), "cycles": _guarded((batch,), np.int32),
           "status": _guarded((batch,), np.int32)}
    trial = {"trial_distances": _guarded((batch, n_starts), np.float64)}
    order = ("aligned", "perm", "rotation", "distance", "best_trial", "cycles", "status")
    assert L.dzo_align_batch_pairs(n, batch, dzo.F64 if dtype is np.float64 else dzo.F32, da.ptr, db.ptr, DETERMINISTIC, 2, 20, 1, 7,
                                   *[out[name][1].ptr for name in order], trial["trial_distances"][1].ptr if want_trials else None) == 0
    _guards_hold(out)
    if want_trials:
        _guards_hold(trial)
    else:
        assert np.all(trial["trial_distances"][0].to_host() == CANARY)
    assert np.array_equal(_bits(da.to_host()), _bits(a)) and np.array_equal(_bits(db.to_host()), _bits(b))
    # the windows hold what the binding returns from plain arrays
    plain = dzo.align_pairs(da, db, n, trials=DETERMINISTIC, random_trials=2, max_cycles=20, allow_inversion=True, seed=7, want_trials=True)
    assert np.array_equal(_bits(out["aligned"][1].to_host()), _bits(plain.aligned.to_host()))
    assert np.array_equal(out["perm"][1].to_host(), plain.permutations) and np.array_equal(out["status"][1].to_host(), plain.status)
    assert np.array_equal(_bits(out["distance"][1].to_host()), _bits(plain.distances))
    if want_trials:
        assert np.array_equal(_bits(trial["trial_distances"][1].to_host()), _bits(plain.trial_distances))
    if want_trials:                                          # the assignment alone, once per size and element type
        assign = {"perm": _guarded((batch, n), np.int32), "cost": _guarded((batch,), np.float64)}
        assert L.dzo_align_batch_assign(n, batch, dzo.F64 if dtype is np.float64 else dzo.F32, da.ptr, db.ptr, assign["perm"][1].ptr,
                                        assign["cost"][1].ptr) == 0
        _guards_hold(assign)
        assert np.array_equal(_bits(da.to_host()), _bits(a)) and np.array_equal(_bits(db.to_host()), _bits(b))
        p, c = dzo.assign_particles(da, db, n)
        assert np.array_equal(assign["perm"][1].to_host(), p) and np.array_equal(_bits(assign["cost"][1].to_host()), _bits(c))


# ------------------------------------------------------------------------------ the consumer
def test_connect_minima_aligns_scrambled_ends():
    """The 13-atom end pairs of tests/test_gpu_neb.py with b rotated, shifted and relabelled: connect_minima(align=True) finds
    the distance align_pairs finds on the unscrambled ends, and the band's two ends have the energies of a and b.  How many
    bands converge is not asserted (tools/bench_align.py reports it)."""
    n, m = 13, 9
    a, b, _, _ = nb.end_pairs(n, (4, 5, 11, 12))
    rng = np.random.default_rng(13)
    scrambled = np.stack([at.join(at.scramble(at.split(x, n), rng)[0]) for x in b])
    da, db, ds = (_dev(v, np.float64) for v in (a, b, scrambled))
    options = dict(trials=PRINCIPAL, random_trials=0)
    plain = dzo.align_pairs(da, db, n, **options)
    c = dzo.connect_minima(da, ds, n, m, force_tol=1e-6, max_iterations=200, align=options)
    assert isinstance(c.alignment, dzo.Alignment) and c.band.shape == (4, m, 3 * n)
    e_a, e_b = dzo.pairwise_batch_energy_gradient(da, n), dzo.pairwise_batch_energy_gradient(db, n)
    band = c.band.to_host()
    aligned = c.alignment.aligned.to_host()
    for k in range(4):
        allowed = _bound(np.float64, a[k])
        seen = abs(c.alignment.distances[k] - plain.distances[k])
        print(k, "distance", c.alignment.distances[k], "plain", plain.distances[k], "seen / allowed %.3g" % (seen / allowed), "status", c.status[k])
        assert seen <= allowed
        assert np.array_equal(band[k, 0], a[k]) and np.array_equal(band[k, -1], aligned[k])
        move = _bound(np.float64, b[k]) + EPS[np.dtype(np.float64)] * max(np.linalg.norm(a[k]), np.linalg.norm(b[k]))
        allowed_e = _energy_allowed(b[k], n, np.float64, move)[0]
        print(k, "energy of the last image: seen / allowed %.3g" % (abs(c.energies[k, -1] - e_b[k]) / allowed_e))
        assert c.energies[k, 0] == e_a[k]
        assert abs(c.energies[k, -1] - e_b[k]) <= allowed_e
    assert not hasattr(dzo.connect_minima(da, db, n, m, force_tol=1e-6, max_iterations=1), "alignment")


def test_lj_align_example_prints_ok(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_align")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK" in r.stdout and "aligned distance" in r.stdout and "FAILED" not in r.stdout, r.stderr
