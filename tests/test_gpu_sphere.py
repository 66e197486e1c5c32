"""The Thomson unit on the device (csrc/dzo_sphere.hip) against tests/sphere_twin.py, at every (N, m) of sphere_twin.CASES in both
element types: the wave kernel from N = 2, with dropped padding pairs inside the 4-unrolled trip (61, 63) and as a full wave
(64); the block kernel with one to four particles per thread; the last (N, m) whose ring fits the LDS and the first whose ring
goes to device memory, per element type; the largest.

a. sphere_project_ against the twin, bit for bit;
b. energy and gradients against the longdouble twin within the derived bounds, the raw fp64 gradient bit for bit the twin's
   in-order sum, and the stored objective and gradient those of the stored point;
c. after every step of (e): every particle on the sphere and every gradient tangent, within the bounds of one operation;
d. every direction against the oracle and the twin over m + 8 single steps, and the ring moving by one each step;
e. every step replayed: the point is project(fma(2^-h, d, x_old)) by the twin's project, every decision the longdouble twin's
   where its energies are apart (tests/test_sphere_twin.py: inside the windows they always are);
f. one launch of m + 5 steps against m + 5 launches of one step and against step(m) + step(5), bit for bit;
g. jittered closed forms and random starts run to their minima;
h. the plain-C example.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import quench_checks as qc
import sphere_twin as st
from build_checks import link_example
from dzo_loader import dzo

LD = np.longdouble
gpu = pytest.mark.gpu
cases = pytest.mark.parametrize("n,m", st.CASES)
dtypes = pytest.mark.parametrize("dtype", st.DTYPES)


@pytest.fixture(scope="module")
def device():
    dzo.init(0)


def make(points, n, m=10):
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(points).ravel())
    return dev, dzo.SphereLBFGS(dev, n, st.STEP, m)


def raw_gradients(opt, n):
    gdev = dzo.DeviceArray.zeros(opt.batch * 3 * n, opt.dtype)
    dzo.sphere_energy_gradient(opt.points, n, gdev, tangent=False)
    return gdev.to_host().reshape(opt.batch, 3 * n)


def consistent(opt, n, state, what):
    """The stored objective and gradient are those of the stored point, bit for bit."""
    gdev = dzo.DeviceArray.zeros(opt.batch * 3 * n, opt.dtype)
    e = dzo.sphere_energy_gradient(opt.points, n, gdev, tangent=True)
    assert qc.same(e, state["OBJECTIVES"]), (what, "objective")
    assert qc.same(gdev.to_host().reshape(opt.batch, 3 * n), state["GRADIENTS"]), (what, "gradient")


# ------------------------------------------------------------------------------ a. the projection
@gpu
@dtypes
@pytest.mark.parametrize("n", [1, 3, 64, 257, 1024])
def test_project_is_the_twin_bit_for_bit(device, n, dtype):
    rng = np.random.default_rng(n)
    raw = (rng.standard_normal((3, 3 * n)) * np.exp(rng.uniform(-6, 6, (3, 3 * n)))).astype(dtype)
    dev = dzo.DeviceArray.from_host(raw.ravel())
    assert dzo.sphere_project_(dev, n) is dev
    once = dev.to_host().reshape(3, 3 * n)
    want = np.stack([st.project(r, dtype) for r in raw])
    assert qc.same(once, want)
    # ... and on points that are already normalised: not the identity in floating point, and still the twin's
    dzo.sphere_project_(dev, n)
    twice = dev.to_host().reshape(3, 3 * n)
    assert qc.same(twice, np.stack([st.project(r, dtype) for r in want]))
    if n >= 64:
        assert not qc.same(twice, once)


@gpu
def test_arguments_are_checked(device):
    dev = dzo.DeviceArray.from_host(st.start(4, 0, np.float64))
    lib = dzo.lib()
    e = dzo.DeviceArray(1, np.float64)
    assert lib.dzo_sphere_batch_energy_gradient(1, 4, 1, 0, dev.ptr, e.ptr, None, 1) != 0           # an unknown energy
    assert lib.dzo_sphere_batch_energy_gradient(0, 4, 1, 0, dev.ptr, e.ptr, None, 2) != 0           # tangent is 0 or 1
    with pytest.raises(Exception):
        dzo.SphereLBFGS(dev, 4, st.STEP, 33)                                                        # DZO_LBFGS_BATCH_MAX_HISTORY
    with pytest.raises(Exception):
        dzo.SphereLBFGS(dev, 4, 0.0, 3)
    with pytest.raises(Exception):
        dzo.SphereLBFGS(dev, 4, st.STEP, 3, energy=1)


# ------------------------------------------------------------------------------ b. against the longdouble twin
@gpu
@dtypes
@cases
def test_objective_and_gradient_against_the_twin(device, n, m, dtype):
    starts = st.starts(n, dtype)
    dev, opt = make(starts, n, m)
    u_is_f64 = np.dtype(dtype) == st.F64
    for k in (0, st.steps_before_the_second_look(n)):
        if k:
            opt.step(k)
        state = qc.state(opt)
        if k == 0:                                              # the constructor stores what the device's projection computed
            assert qc.same(state["POINTS"], np.stack([st.project(r, dtype) for r in starts])), (n, m)
        consistent(opt, n, state, (n, m, k))
        assert qc.same(dzo.sphere_energy_gradient(opt.points, n), state["OBJECTIVES"]), (n, m, k, "energies without a gradient buffer")
        raw = raw_gradients(opt, n)
        worst_e = worst_g = worst_r = 0.0
        for b in range(opt.batch):
            p = state["POINTS"][b]
            E, S, g, Srow = st.exact(p)
            err, bound = abs(LD(state["OBJECTIVES"][b]) - E), st.bound_energy(n, dtype, S)
            worst_e = max(worst_e, float(err / bound))
            assert err <= bound, (n, m, k, b, float(err), float(bound))
            errg = np.abs(state["GRADIENTS"][b].reshape(3, n).astype(LD) - st.exact_tangent(p, g))
            boundg = st.bound_gradient(n, dtype, Srow)[None, :]
            worst_g = max(worst_g, float(np.max(errg / boundg)))
            assert np.all(errg <= boundg), (n, m, k, b, float(np.max(errg / boundg)))
            errr = np.abs(raw[b].reshape(3, n).astype(LD) - g)
            boundr = st.bound_gradient(n, dtype, Srow, constrained=False)[None, :]
            worst_r = max(worst_r, float(np.max(errr / boundr)))
            assert np.all(errr <= boundr), (n, m, k, b, float(np.max(errr / boundr)))
            if u_is_f64:                                        # the reference's order of summation: zeros compared by value
                _, g_twin = st.energy_gradient(p, dtype, constrained=False)
                assert np.array_equal(raw[b], g_twin), (n, m, k, b, "raw gradient, bit for bit")
                assert qc.same(state["GRADIENTS"][b] + 0.0, st.tangent(p, g_twin, dtype) + 0.0), (n, m, k, b, "tangent gradient, bit for bit")
        print(f"N={n} m={m} {np.dtype(dtype).name} after {k} steps: worst error / bound: energy {worst_e:.4f}, tangent gradient {worst_g:.4f}, "
              f"raw gradient {worst_r:.4f}")


# ------------------------------------------------------------------------------ d. directions and the ring across the wrap
@gpu
@dtypes
@cases
def test_direction_against_the_oracle_across_the_wrap(device, n, m, dtype):
    dev, opt = make(st.starts(n, dtype), n, m)
    worst = qc.check_directions_and_ring(opt, n, m, dtype, m + 8)
    print(f"N={n} m={m} {np.dtype(dtype).name}: worst direction error / tolerance {worst:.4f} (tolerance {qc.tol_direction(m, dtype):.1e})")


# ------------------------------------------------------------------------------ c, e. step replay and the invariants
@gpu
@dtypes
@cases
def test_step_replay_and_invariants(device, n, m, dtype):
    t = np.dtype(dtype).type
    window = st.window(n, dtype)
    dev, opt = make(st.starts(n, dtype), n, m)
    undecided = trials = 0
    worst_norm = worst_overlap = 0.0
    cur = qc.state(opt)
    for k in range(window + 4):                                  # the point is replayed on every step, decisions inside the window
        before = cur
        opt.step(1)
        cur = qc.state(opt)
        raw = raw_gradients(opt, n)
        for b in range(opt.batch):
            # c. the stored state: on the sphere, and tangent
            P, G, R = (a[b].reshape(3, n).astype(LD) for a in (cur["POINTS"], cur["GRADIENTS"], raw))
            off = np.max(np.abs((P * P).sum(axis=0) - 1) / st.bound_norm(dtype))
            over = np.max(np.abs((P * G).sum(axis=0)) / np.maximum(st.bound_overlap(dtype, np.sqrt((R * R).sum(axis=0))), LD(1e-300)))
            worst_norm, worst_overlap = max(worst_norm, float(off)), max(worst_overlap, float(over))
            assert off <= 1 and over <= 1, (n, m, k, b, float(off), float(over))
            if before["IS_STUCK"][b]:
                continue
            x_old, d, h = before["POINTS"][b], cur["DIRECTIONS"][b], int(cur["LAST_HALVINGS"][b])
            if cur["IS_STUCK"][b]:                              # a stuck step leaves point, gradient and history as they were
                for name in ("POINTS", "GRADIENTS", "OBJECTIVES", "S", "Y", "RHO", "HISTORY_COUNTS", "ITERATION_COUNTS"):
                    assert qc.same(cur[name][b], before[name][b]), (n, m, k, b, name)
            else:
                assert qc.same(cur["POINTS"][b], st.project(x_old + t(2.0 ** -h) * d, dtype)), (n, m, k, b, h)   # 2^-h d is exact
                assert np.array_equal(cur["DELTA_POINTS"][b], cur["POINTS"][b] - x_old), (n, m, k, b)
                assert np.array_equal(cur["DELTA_GRADIENTS"][b], cur["GRADIENTS"][b] - before["GRADIENTS"][b]), (n, m, k, b)
            if k >= window:
                continue
            last = h if not cur["IS_STUCK"][b] else h - 1
            old = st.exact_energy(x_old)
            for hh in range(last + 1):
                x_t = st.project(x_old + t(2.0 ** -hh) * d, dtype)
                diff, bound = st.decision_margin(x_old, x_t, dtype, old)
                trials += 1
                if abs(diff) <= bound:
                    undecided += 1
                    continue
                if hh == h and not cur["IS_STUCK"][b]:
                    assert diff <= bound, (n, m, k, b, hh, "accepted a trial that does not decrease", float(diff), float(bound))
                else:
                    assert diff >= -bound, (n, m, k, b, hh, "rejected a trial that decreases", float(diff), float(bound))
    print(f"N={n} m={m} {np.dtype(dtype).name}: {undecided} of {trials} trials undecided in the first {window} steps; worst | |p|^2 - 1 | / bound "
          f"{worst_norm:.3f}, p . g / bound {worst_overlap:.3f}")
    assert trials >= window * opt.batch and undecided == 0


# ------------------------------------------------------------------------------ f. one launch against many
@gpu
@dtypes
@cases
def test_one_launch_against_many(device, n, m, dtype):
    points, steps = st.starts(n, dtype), m + 5
    _, one = make(points, n, m)
    one.step(steps)
    a = qc.state(one)
    _, many = make(points, n, m)
    for _ in range(steps):
        many.step(1)
    qc.assert_same_state(qc.state(many), a, f"step({steps}) against {steps} x step(1)")
    _, two = make(points, n, m)
    two.step(m)
    assert np.all((two.history_counts == m) | two.is_stuck)
    two.step(steps - m)
    qc.assert_same_state(qc.state(two), a, f"step({steps}) against step({m}) + step({steps - m})")
    assert np.all((a["HISTORY_COUNTS"] == m) | (a["IS_STUCK"] != 0))
    # ... and an instance computes the same bits alone as in the batch
    _, alone = make(points[1:2], n, m)
    alone.step(steps)
    qc.assert_same_state(qc.state(alone), a, "alone against in the batch", rows_b=slice(1, 2))


# ------------------------------------------------------------------------------ g. minima
@gpu
@dtypes
@pytest.mark.parametrize("n", st.CLOSED_N)
def test_jittered_closed_forms_return(device, n, dtype):
    E = st.closed_form(n)[1]
    tol = st.tol_minimum(n, dtype, E, st.TWIN_WORST_CLOSED[(n, np.dtype(dtype))])
    dev, opt = make(np.stack([st.jittered(n, s, dtype) for s in range(16)]), n, 10)
    assert opt._run(500, 25) < 500 and opt.count_active() == 0
    state = qc.state(opt)
    worst = 0.0
    for b in range(16):
        worst = max(worst, float(abs(LD(state["OBJECTIVES"][b]) - E)), float(abs(st.exact_energy(state["POINTS"][b])[0] - E)))
    print(f"closed form N={n} {np.dtype(dtype).name}: worst |E - closed form| {worst:.3e}, tolerance {float(tol):.3e}, "
          f"steps {state['ITERATION_COUNTS'].min()}..{state['ITERATION_COUNTS'].max()}")
    assert worst <= tol


@gpu
@dtypes
@pytest.mark.parametrize("n", [12, 32])
def test_random_starts_reach_the_lowest_energy(device, n, dtype):
    lowest = st.E_ICOSAHEDRON if n == 12 else st.E_LOWEST_32
    tol = st.tol_minimum(n, dtype, lowest, st.TWIN_WORST_RANDOM[(n, np.dtype(dtype))])
    dev, opt = make(st.random_starts(n, 16, st.RANDOM_SEED, dtype), n, 10)
    assert opt._run(1000, 50) < 1000 and opt.count_active() == 0
    state = qc.state(opt)
    worst = 0.0
    for b in range(16):
        worst = max(worst, float(abs(LD(state["OBJECTIVES"][b]) - lowest)), float(abs(st.exact_energy(state["POINTS"][b])[0] - lowest)))
    print(f"random starts N={n} {np.dtype(dtype).name}: worst |E - lowest| {worst:.3e}, tolerance {float(tol):.3e}, "
          f"steps {state['ITERATION_COUNTS'].min()}..{state['ITERATION_COUNTS'].max()}")
    assert worst <= tol


# ------------------------------------------------------------------------------ h. the example
def example_starts():
    """The 64 x [x | y | z] starts of examples/thomson_quench.c: its generator restated."""
    state, out = 0x9E3779B97F4A7C16, np.empty(64 * 36)
    for k in range(out.size):
        state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out[k] = 2.0 * (((state >> 11) + 0.5) / 9007199254740992.0) - 1.0
    return out.reshape(64, 36)


@gpu
def test_thomson_example_runs_and_reaches_the_icosahedron(device, tmp_path):
    exe, _, _ = link_example(tmp_path, "thomson_quench")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    m = re.search(r"lowest energy ([\d.]+), highest energy ([\d.]+), (\d+) of 64 at the icosahedron, all at rest", r.stdout)
    assert m, r.stdout
    # the count the twin reaches on the example's own starts
    reached = 0
    for p in example_starts():
        q = st.SphereQuench(p, 0.01, 10, np.float64)
        q.run(5000)
        reached += int(abs(float(q.f) - 49.16525305763) <= 1e-9)
    print("the twin reaches the icosahedron from", reached, "of 64")
    assert int(m.group(3)) == reached
    assert abs(float(m.group(1)) - float(st.E_ICOSAHEDRON)) <= 1e-9
    if reached == 64:
        assert abs(float(m.group(2)) - float(st.E_ICOSAHEDRON)) <= 1e-9
