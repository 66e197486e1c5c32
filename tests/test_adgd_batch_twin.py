"""The CPU twin of the batched AdGD optimizer (tests/adgd_batch_twin.py) pinned against things it does not depend on, and what
the GPU tests (tests/test_gpu_adgd_batch.py) assume about their inputs shown on the CPU:

* its step-size rule equals the oracle's AdGD (oracle/dzo_oracle_impl.h, step!() of src/DZOptimization.jl:274-312) on hand-fed
  (delta_point, delta_gradient, current, previous), bit for bit;
* it reaches the literature minima of LJ13 and LJ38 from the jittered icosahedron / octahedron;
* the GPU tests' inputs have NO undecided trial inside their windows: a trial is undecided when
  |E_trial - E_old| <= (N + 32) u (S_old + S_trial), the derived bound of tests/test_gpu_pairwise.py on both energies.
"""
import numpy as np
import pytest

import adgd_batch_twin as at
import pairwise_twin as tw
import quench_twin as qt
from oracle import oracle as orc

DTYPES = [np.float64, np.float32]


# ------------------------------------------------------------------------------ the rule against the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_step_size_rule_matches_the_oracle_bit_for_bit(dtype):
    """The oracle's AdGD runs on a quadratic; before each step its delta_point and delta_gradient are overwritten with hand-made
    vectors whose squares sum exactly in any order (small integers times a power of two), so that the order of the oracle's own
    norm does not enter.  The step sizes it holds before the step and the hand-made vectors go to the twin's rule; the oracle's
    new current_step_size must have the same bits.  The vectors are chosen so that both branches of the min are taken, and one
    delta_gradient is zero (:293)."""
    n = 12
    rng = np.random.default_rng(3)
    prob = orc.Problem(orc.QUADRATIC_CHAIN, n, dtype=dtype)
    opt = orc.AdGD(prob, rng.uniform(-1.0, 1.0, n).astype(dtype), 0.125)
    opt.step()                                                  # iteration_count 1: the rule is live from here on
    assert opt.iteration_count == 1 and not opt.is_stuck
    capped = grown_taken = zero_dg = 0
    for k in range(24):
        dx = (rng.integers(-7, 8, n) * 2.0 ** int(rng.integers(-12, -4))).astype(dtype)
        dg = (rng.integers(-7, 8, n) * 2.0 ** int(rng.integers(-14, 2))).astype(dtype)
        if k % 8 == 7:
            dg[:] = 0
        if not dx.any():
            dx[0] = dtype(2.0 ** -8)
        opt.delta_point[:] = dx
        opt.delta_gradient[:] = dg
        current, previous = dtype(opt.current_step_size), dtype(opt.previous_step_size)
        grown, cap = at.step_size_candidates(dx, dg, current, previous, dtype)
        want = at.next_step_size(dx, dg, current, previous, dtype)
        opt.step()
        if opt.is_stuck:
            break
        got = dtype(opt.current_step_size)
        assert got.tobytes() == dtype(want).tobytes(), (k, got, want)
        assert dtype(opt.previous_step_size).tobytes() == current.tobytes(), k      # :298
        zero_dg += cap is None
        capped += cap is not None and not grown < cap
        grown_taken += cap is not None and grown < cap
    assert capped >= 3 and grown_taken >= 3 and zero_dg >= 1, (capped, grown_taken, zero_dg)


@pytest.mark.parametrize("dtype", DTYPES)
def test_constructor_and_first_step(dtype):
    """:229-241 and the first step!(), which takes current_step_size as it is (:288)."""
    t = np.dtype(dtype).type
    q = at.AdGD(at.start(13, 0, dtype), 0.01, dtype)
    g = q.g.astype(np.float64)
    assert not q.is_stuck and q.iteration_count == 0 and q.df == 0 and not q.dx.any() and not q.dg.any()
    assert q.current_step_size == q.previous_step_size == t(0.01) / t(np.sqrt(np.dot(g, g)))
    x0, g0, s0 = q.x.copy(), q.g.copy(), q.current_step_size
    q.step()
    assert q.iteration_count == 1 and q.last_halvings == 0 and q.current_step_size == s0 and q.previous_step_size == s0
    assert np.array_equal(q.x, np.array([tw.fma(-s0, a, b, dtype) for a, b in zip(g0, x0)], dtype=dtype))
    assert np.array_equal(q.dx, q.x - x0) and np.array_equal(q.dg, q.g - g0) and q.f < qt.energy_gradient(x0, dtype)[0]
    one = at.AdGD(np.array([0.25, -1.0, 3.0], dtype=dtype), 0.01, dtype)     # one particle: no gradient
    assert one.is_stuck and one.current_step_size == 0 and one.previous_step_size == 0 and one.f == 0
    assert one.step().iteration_count == 0


def test_bounded_halvings_leave_the_documented_state():
    """Two coincident particles: energy and gradient are not finite, no trial is accepted, stuck after max_halvings rejected
    trials."""
    p = at.start(38, 1, np.float64)
    p[1] = p[0]; p[39] = p[38]; p[77] = p[76]
    q = at.AdGD(p, 0.01, np.float64, max_halvings=8)
    s0 = q.current_step_size
    g0, f0 = q.g.copy(), q.f
    q.step()
    assert q.is_stuck and q.last_halvings == 8 and q.iteration_count == 0 and len(q.trials) == 8
    assert np.array_equal(q.x, p) and np.array_equal(q.dx, p) and not q.dg.any()
    assert np.array_equal(q.g, g0, equal_nan=True) and (q.f == f0 or (np.isnan(q.f) and np.isnan(f0)))
    assert np.isnan(s0) and np.isnan(q.previous_step_size) and np.isnan(q.current_step_size)   # |g0| is not a number: 0.01 / |g0| neither


# ------------------------------------------------------------------------------ the literature minima
@pytest.mark.parametrize("name,n,lit", [("ico", 13, tw.LJ13), ("oct", 38, tw.LJ38)])
def test_twin_reaches_the_literature_minima(name, n, lit):
    for seed in range(3):
        q = at.AdGD(qt.start(name, seed), 0.01)
        steps = q.run(5000)
        print(f"{name} seed {seed}: stuck after {steps} steps at {q.f:.9f}")
        assert q.is_stuck and abs(q.f - lit) <= 5e-7, (name, seed, steps, q.f)


# ------------------------------------------------------------------------------ the GPU tests' inputs
# trials inside the windows over the starts ico (13), oct (38) and lattice(200), seeds 0-3: (step length, element type) ->
# (trials, rejected trials).  The halvings of the first step at length 1.0 are 3 (N = 13), 1-2 (38) and 0-1 (200).
COUNTS = {(0.01, at.F64): (247, 7), (0.01, at.F32): (60, 0), (1.0, at.F64): (142, 22), (1.0, at.F32): (81, 21)}
FIRST_HALVINGS = {13: {3}, 38: {1, 2}, 200: {0, 1}}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("step_length", [0.01, 1.0])
def test_no_undecided_trial_inside_the_windows(step_length, dtype):
    window = at.WINDOWS[step_length][np.dtype(dtype)]
    trials = rejected = 0
    for n in at.NS:
        for seed in at.SEEDS:
            tr, undecided, rj, first = at.count_undecided(at.start(n, seed, dtype), step_length, dtype, window)
            assert undecided == 0, (n, seed, step_length, undecided, tr)
            if step_length == 1.0:
                assert first in FIRST_HALVINGS[n], (n, seed, first)
            else:
                assert first == 0, (n, seed, first)
            trials += tr; rejected += rj
    print(f"step length {step_length} {np.dtype(dtype).name}: {trials} trials, {rejected} rejected in the first {window} steps")
    assert (trials, rejected) == COUNTS[(step_length, np.dtype(dtype))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", at.EDGE_NS)
def test_no_undecided_trial_at_the_shape_edges(n, dtype):
    for b, p in enumerate(at.edge_starts(n, dtype)):
        tr, undecided, _, _ = at.count_undecided(p, 0.01, dtype, at.EDGE_STEPS)
        assert tr == at.EDGE_STEPS and undecided == 0, (n, b, tr, undecided)
