"""The CPU twin of the parallel-tempering Monte Carlo (tests/tempering_twin.py) against things it does not depend on, and the
proof that the inputs of the GPU trajectory test -- not the kernel -- keep that test honest.  No GPU."""
import math

import numpy as np
import pytest

import pairwise_twin as pw
import tempering_twin as tt
from oracle import oracle as orc

LD = np.longdouble


def test_pcg_stream_is_the_oracles():
    for seed in (0, 1, 4242, 2 ** 40 + 3):
        raw, state = tt.pcg_raw(tt.pcg_state(seed), 50)
        assert np.array_equal(raw, orc.pcg_raw(50, seed))
        more, _ = tt.pcg_raw(state, 10)
        assert np.array_equal(more, orc.pcg_raw(60, seed)[50:])


def test_draws_follow_the_rule():
    raw = np.array([[0, 0, 0, 2 ** 32 - 1, 2 ** 31, 2 ** 32 - 1], [2 ** 32 - 1, 2 ** 31, 2 ** 30, 5, 7, 0]], dtype=np.uint32)
    j, normals, u, r = tt.step_draws(raw, 38, np.float64)
    assert j.tolist() == [0, 37]
    assert u[0] == (2.0 ** 32 - 1) / 2.0 ** 32 and u[1] == 0.0
    assert tt.step_draws(raw, 38, np.float32)[2][0] == np.float32(1.0)           # rounds up to 1 in fp32
    r0 = math.sqrt(-2.0 * math.log(0.5 * 2.0 ** -32))
    assert abs(normals[0, 0] - r0) <= 1e-14 * r0                                  # angle 2 pi 2^-33: cos = 1 - 1e-19
    assert abs(normals[1, 1] - math.sqrt(-2.0 * math.log((2 ** 31 + 0.5) / 2 ** 32))) <= 1e-9     # angle ~ pi / 2: the sine
    z = tt.own_draws(5, 4000, 13, np.float64)[1].ravel()
    assert abs(z.mean()) <= 5 / math.sqrt(z.size) and abs(z.var() - 1) <= 5 * math.sqrt(2 / z.size)


def test_fac_is_the_1024th_root_of_two():
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-3)):
        f = tt.fac(dtype)
        assert f.dtype == dtype
        assert abs(float(LD(f) ** 1024) - 2.0) <= tol
    t = np.float64
    assert tt.adapt_radius(0.5, 10, 31, t) == t(0.5) / tt.fac(t)
    assert tt.adapt_radius(0.5, 10, 29, t) == t(0.5) * tt.fac(t)
    assert tt.adapt_radius(0.5, 10, 30, t) == 0.5
    assert tt.adapt_radius(0.9999, 10, 0, t) == 1.0


def test_against_a_plain_metropolis_loop_on_three_particles():
    """the twin's own decisions against a loop written out in plain fp64 numpy (pair energies by the textbook formula)"""
    def lj(r2):
        s6 = 1.0 / r2 ** 3
        return 4.0 * (s6 * s6 - s6)

    def total(p):
        return sum(lj(float(((p[:, a] - p[:, b]) ** 2).sum())) for a in range(3) for b in range(a + 1, 3))

    xyz0 = np.array([[0.0, 1.1, 0.5], [0.0, 0.0, 0.95], [0.0, 0.0, 0.1]])
    steps, beta, radius, R = 400, 3.0, 0.1, 1.6
    j, normals, u, _ = tt.own_draws(99, steps, 3, np.float64)
    tr = tt.simulate(xyz0, j, normals, u, radius, beta, R, np.float64)
    p = xyz0.copy()
    e = total(p)
    acc = 0
    for i in range(steps):
        q = p.copy()
        q[:, j[i]] = p[:, j[i]] + radius * normals[i]
        if (q[:, j[i]] ** 2).sum() < R * R:
            d = total(q) - e
            if d <= 0 or u[i] <= math.exp(-beta * d):
                p, e, acc = q, e + d, acc + 1
        assert abs(float(tr.energy[i]) - e) <= 1e-9 * max(1.0, abs(e)), i
    assert acc == tr.num_accept and 0 < acc < steps
    assert np.allclose(tr.final, p, rtol=0, atol=1e-12)
    assert tr.num_reject == steps - acc
    # replaying the twin's own decisions gives the same path, and no decision contradicts its class
    rp = tt.replay(xyz0, j, normals, u, tr.code, radius, beta, R, np.float64)
    assert np.array_equal(rp.final, tr.final)
    assert not np.any((rp.klass == tt.MUST_ACCEPT) & (tr.code != tt.CODE_ACCEPTED) & tr.inside)
    assert not np.any((rp.klass == tt.MUST_REJECT) & (tr.code != tt.CODE_REJECTED) & tr.inside)


def test_classify():
    t = np.float64
    assert tt.classify(-1.0, 1e-12, 0.99, 5.0, t) == tt.MUST_ACCEPT
    assert tt.classify(1.0, 1e-12, 0.5, 5.0, t) == tt.MUST_REJECT                # exp(-5) = 0.0067
    assert tt.classify(1.0, 1e-12, 0.001, 5.0, t) == tt.MUST_ACCEPT
    assert tt.classify(1.0, 1e-3, math.exp(-5.0), 5.0, t) == tt.UNDECIDED
    assert tt.classify(1e-13, 1e-12, 0.5, 5.0, t) == tt.UNDECIDED or tt.classify(1e-13, 1e-12, 0.5, 5.0, t) == tt.MUST_ACCEPT
    assert tt.classify(0.5, 1e-12, 0.999999, 0.0, t) == tt.MUST_ACCEPT           # beta = 0


def test_moments_and_heat_capacity():
    rng = np.random.default_rng(3)
    e = -170.0 + 2.0 * rng.standard_normal(5000)
    V1, V2, V3, A1, A2, A3 = tt.moments(e)
    el = e.astype(LD)
    assert abs(V1 - np.mean(el)) <= 1e-15 * A1 and abs(V2 - np.mean(el ** 2)) <= 1e-15 * A2 and abs(V3 - np.mean(el ** 3)) <= 1e-15 * A3
    cv, cvp = tt.heat_capacity(V1, V2, V3, 4.0, np.float64)
    var = float(np.var(el))
    assert abs(cv - 16.0 * var) <= 1e-9 * 16.0 * var
    cov = float(np.mean(el ** 3) - np.mean(el ** 2) * np.mean(el))
    assert abs(cvp - 256.0 * (cov - (float(V1) + 0.25) * 2 * var)) <= 1e-6 * abs(cvp) + 1e-3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", tt.TRAJECTORY_NS)
def test_trajectory_inputs_leave_few_steps_undecided(n, dtype):
    """The share of steps whose decision the twin cannot tell, for the inputs of the GPU trajectory test, from the twin alone: its
    own decisions on draws from numpy's Box-Muller over the oracle's PCG32.  At most 5 % in fp32, none in fp64."""
    reps, beta, radii, R = tt.trajectory_inputs(n, dtype)
    undecided = inside = accepted = 0
    for k in range(reps.shape[0]):
        raw = orc.pcg_raw(6 * tt.TRAJECTORY_STEPS, tt.TRAJECTORY_SEED + n + k).reshape(-1, 6)
        j, normals, u, _ = tt.step_draws(raw, n, dtype)
        tr = tt.simulate(reps[k], j, normals, u, np.dtype(dtype).type(radii[k]), np.dtype(dtype).type(beta[k]), R, dtype)
        undecided += int(np.sum(tr.inside & (tr.klass == tt.UNDECIDED)))
        inside += int(tr.inside.sum()); accepted += tr.num_accept
    total = tt.TRAJECTORY_STEPS * reps.shape[0]
    print(f"N={n} {np.dtype(dtype).name}: {inside} inside, {accepted} accepted, {undecided} undecided of {total}")
    assert inside > total // 2 and 0 < accepted < total                           # the inputs exercise both branches
    assert undecided / total <= tt.UNDECIDED_CAP[np.dtype(dtype)]
