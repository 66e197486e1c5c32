"""GPU tests of the batched L-BFGS quench (dzo_lbfgs_batch_*, dzo_pairwise_batch_energy_gradient): the live LBFGSOptimizer of
src/DZOptimization.jl:321-509 over many small Lennard-Jones clusters in one launch.

1. the invariants of run_and_test! (legacy/DZOptimization.jl:998-1049), exact, after every one of 50 single steps;
2. objective and gradient against the longdouble twin with the DERIVED bound of tests/test_gpu_pairwise.py, (N + 32) u S;
3. the direction against the oracle's compute_lbfgs_step_direction! on the state read before the step;
4. a replay of every step: the point is fma(2^-h, d, x_old) exactly, and the twin's energies agree with every decision
   (trials inside the bound are undecided; tests/test_quench_twin.py shows the inputs have none inside the windows);
5. quenches to the literature minima, next to the one-at-a-time LBFGSOptimizer;
6. independence of batch and position, determinism, and launch splitting, bit for bit;
7. edges and error codes;  8. the tempering hand-over;  9. the plain-C example.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pairwise_twin as tw
import quench_checks as qc
import quench_twin as qt
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
LD = np.longdouble
U = qt.U
DTYPES = [np.float64, np.float32]
NS = [13, 38, 200]                                # WAVE, WAVE, BLOCK
TOL_DIRECTION = qc.TOL_DIRECTION                   # set at history_length 10
WINDOW = {np.dtype(np.float64): 20, np.dtype(np.float32): 5}
VECTORS = qc.VECTORS
_make, _same, _state, _assert_same_state, _consistent = qc.make, qc.same, qc.state, qc.assert_same_state, qc.consistent


@pytest.fixture(scope="module", autouse=True)
def _init():
    dzo.init(0)


def _start(n, seed, dtype):
    if n == 13:
        return qt.start("ico", seed, dtype)
    if n == 38:
        return qt.start("oct", seed, dtype)
    return np.asarray(np.concatenate(tw.lattice(n, seed=seed)), dtype=dtype)


def _starts(n, seeds, dtype):
    return np.stack([_start(n, s, dtype) for s in seeds])


# ------------------------------------------------------------------------------ 1. invariants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_run_and_test_invariants(n, dtype):
    dev, opt = _make(_starts(n, range(8), dtype), n)
    prev = _state(opt)
    _consistent(opt, n, prev, (n, 0))
    assert not prev["IS_STUCK"].any() and not prev["ITERATION_COUNTS"].any()
    for k in range(1, 51):
        opt.step(1)
        cur = _state(opt)
        _consistent(opt, n, cur, (n, k))
        for b in range(opt.batch):
            where = (n, np.dtype(dtype).name, k, b)
            if prev["IS_STUCK"][b] or cur["IS_STUCK"][b]:
                assert _same(cur["POINTS"][b], prev["POINTS"][b]) and _same(cur["GRADIENTS"][b], prev["GRADIENTS"][b]), where
                assert cur["ITERATION_COUNTS"][b] == prev["ITERATION_COUNTS"][b] and _same(cur["OBJECTIVES"][b], prev["OBJECTIVES"][b]), where
                if prev["IS_STUCK"][b]:
                    for name in VECTORS:
                        assert _same(cur[name][b], prev[name][b]), (where, name, "a stuck instance changed")
                continue
            assert np.array_equal(cur["DELTA_POINTS"][b], cur["POINTS"][b] - prev["POINTS"][b]), where
            assert np.array_equal(cur["DELTA_GRADIENTS"][b], cur["GRADIENTS"][b] - prev["GRADIENTS"][b]), where
            assert cur["OBJECTIVES"][b] < prev["OBJECTIVES"][b], where
            assert cur["DELTA_OBJECTIVES"][b] == cur["OBJECTIVES"][b] - prev["OBJECTIVES"][b], where
            assert cur["ITERATION_COUNTS"][b] == prev["ITERATION_COUNTS"][b] + 1, where
            assert cur["HISTORY_COUNTS"][b] == min(k, 10), where
            s, y = cur["DELTA_POINTS"][b].astype(np.float64), cur["DELTA_GRADIENTS"][b].astype(np.float64)
            assert _same(cur["S"][b, 0], cur["DELTA_POINTS"][b]) and _same(cur["Y"][b, 0], cur["DELTA_GRADIENTS"][b]), where
            assert abs(cur["RHO"][b, 0] - np.dot(s, y)) <= 1e-13 * np.sum(np.abs(s * y)), where
            if k > 1:                                        # the older pairs moved down by one
                keep = min(k, 10) - 1
                assert _same(cur["S"][b, 1:1 + keep], prev["S"][b, :keep]) and _same(cur["RHO"][b, 1:1 + keep], prev["RHO"][b, :keep]), where
        prev = cur


# ------------------------------------------------------------------------------ 2. against the longdouble twin
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_objective_and_gradient_against_the_twin(n, dtype):
    dev, opt = _make(_starts(n, range(4), dtype), n)
    u = U[np.dtype(dtype)]
    for k in (0, 10):
        if k:
            opt.step(k)
        st = _state(opt)
        worst_e = worst_g = 0.0
        for b in range(opt.batch):
            p = st["POINTS"][b].astype(np.float64)
            x, y, z = p[:n], p[n:2 * n], p[2 * n:]
            E, S = tw.energy(x, y, z)
            err = abs(LD(st["OBJECTIVES"][b]) - E)
            bound = LD(n + 32) * u * S
            worst_e = max(worst_e, float(err / bound))
            assert err <= bound, (n, k, b, float(err), float(bound))
            g, Srow, _ = tw.gradient(x, y, z)
            errg = np.abs(st["GRADIENTS"][b].reshape(3, n).astype(LD) - g)
            boundg = LD(n + 32) * u * Srow[None, :]
            worst_g = max(worst_g, float(np.max(errg / boundg)))
            assert np.all(errg <= boundg), (n, k, b)
        print(f"N={n} {np.dtype(dtype).name} after {k} steps: worst error / bound: energy {worst_e:.4f}, gradient {worst_g:.4f}")


# ------------------------------------------------------------------------------ 3. direction parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_direction_against_the_oracle(n, dtype):
    dev, opt = _make(_starts(n, range(4), dtype), n)
    opt.step(1)
    worst = 0.0
    for k in range(20):
        before = _state(opt)
        opt.step(1)
        d = opt.step_directions
        for b in range(opt.batch):
            if before["IS_STUCK"][b]:
                continue
            hc = int(before["HISTORY_COUNTS"][b])
            assert hc == min(k + 1, 10)
            d_ref, _ = orc.lbfgs_direction(before["GRADIENTS"][b].astype(np.float64), before["S"][b, :hc].astype(np.float64),
                                           before["Y"][b, :hc].astype(np.float64), before["RHO"][b, :hc])
            err = np.linalg.norm(d[b].astype(np.float64) - d_ref) / np.linalg.norm(d_ref)
            worst = max(worst, err)
            assert err <= TOL_DIRECTION[np.dtype(dtype)], (n, k, b, err)
    print(f"N={n} {np.dtype(dtype).name}: worst direction error {worst:.3e}")


# ------------------------------------------------------------------------------ 4. step replay
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_step_replay(n, dtype):
    t = np.dtype(dtype).type
    window = WINDOW[np.dtype(dtype)]
    dev, opt = _make(_starts(n, range(4), dtype), n)
    undecided = trials = 0
    for k in range(window + 10):                             # the point is replayed on every step, decisions inside the window
        before = _state(opt)
        opt.step(1)
        cur = _state(opt)
        for b in range(opt.batch):
            if before["IS_STUCK"][b]:
                continue
            x_old, d, h = before["POINTS"][b], cur["DIRECTIONS"][b], int(cur["LAST_HALVINGS"][b])
            if not cur["IS_STUCK"][b]:
                assert _same(cur["POINTS"][b], x_old + t(2.0 ** -h) * d), (n, k, b, h)     # 2^-h d is exact: the bits of the fma
            if k >= window:
                continue
            last = h if not cur["IS_STUCK"][b] else h - 1
            for hh in range(last + 1):
                x_t = x_old + t(2.0 ** -hh) * d
                diff, bound = qt.decision_margin(x_old, x_t, dtype)
                trials += 1
                if abs(diff) <= bound:
                    undecided += 1
                    continue
                if hh == h and not cur["IS_STUCK"][b]:
                    assert diff <= bound, (n, k, b, hh, "accepted a trial that does not decrease", float(diff), float(bound))
                else:
                    assert diff >= -bound, (n, k, b, hh, "rejected a trial that decreases", float(diff), float(bound))
    print(f"N={n} {np.dtype(dtype).name}: {undecided} of {trials} trials undecided in the first {window} steps")
    assert undecided == 0


# ------------------------------------------------------------------------------ 5. quench to the literature values
@pytest.mark.parametrize("name,n,lit", [("ico", 13, tw.LJ13), ("oct", 38, tw.LJ38)])
def test_quench_reaches_the_literature_minima(name, n, lit):
    starts = np.stack([qt.start(name, s) for s in range(10)])
    dev, opt = _make(starts, n)
    steps, done = 0, False
    while not done and steps < 2000:
        done = opt.step(50)
        steps += 50
    f = opt.current_objective_values
    print(f"{name}: f = {f.round(9).tolist()} after {opt.iteration_counts.tolist()} steps")
    assert done and opt.is_stuck.all() and opt.count_active() == 0
    assert np.all(np.abs(f - lit) <= 5e-7), f
    for s in range(10):
        prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n)
        one = dzo.LBFGSOptimizer(None, prob, None, dzo.DeviceArray.from_host(starts[s]), 0.01, 10)
        k = 0
        while k < 2000 and not one.is_stuck:
            one.step()
            k += 1
        assert one.is_stuck
        assert abs(one.current_objective_value - f[s]) <= 1e-9, (name, s, one.current_objective_value, f[s])


# ------------------------------------------------------------------------------ 6. independence and determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_independence_and_determinism(n, dtype):
    batch, pos = 256, 200
    starts = _starts(n, [s % 7 for s in range(batch)], dtype)
    starts[pos] = _start(n, 11, dtype)
    _, big = _make(starts, n)
    big.step(100)
    a = _state(big)
    _, alone = _make(starts[pos:pos + 1], n)
    alone.step(100)
    _assert_same_state(_state(alone), a, "alone against position 200 of 256", slice(0, 1), slice(pos, pos + 1))
    _, again = _make(starts, n)
    again.step(100)
    _assert_same_state(_state(again), a, "the same batch twice")
    _, split = _make(starts, n)
    split.step(50)
    split.step(50)
    _assert_same_state(_state(split), a, "step(100) against step(50) + step(50)")
    _, lazy = _make(starts, n)
    assert lazy.step(100, wait=False) is None
    dzo.synchronize()
    _assert_same_state(_state(lazy), a, "step(.., NULL) + dzo_synchronize against the blocking form")
    # instances that share a start share every bit, wherever they sit
    for b in range(7, batch):
        if b != pos:
            assert _same(a["POINTS"][b], a["POINTS"][b % 7]) and _same(a["OBJECTIVES"][b], a["OBJECTIVES"][b % 7]), b


# ------------------------------------------------------------------------------ 7. edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_particle_is_stuck_at_creation(dtype):
    dev, opt = _make(np.array([[0.25, -1.0, 3.0]] * 3, dtype=dtype), 1)
    st = _state(opt)
    assert st["IS_STUCK"].all() and opt.count_active() == 0
    assert not st["OBJECTIVES"].any() and not st["GRADIENTS"].any() and not st["DIRECTIONS"].any()
    assert opt.step(5) is True
    _assert_same_state(_state(opt), st, "N = 1 after step")


@pytest.mark.parametrize("n,m,dtype,halvings", [
    pytest.param(38, 10, np.float64, 64, id="38"), pytest.param(200, 10, np.float64, 64, id="200"),
    pytest.param(64, 3, np.float64, 8, id="64-3"), pytest.param(257, 1, np.float64, 8, id="257-1"),
    pytest.param(1024, 5, np.float32, 8, id="1024-5-float32")])
def test_coincident_particles_do_not_disturb_the_neighbours(n, m, dtype, halvings):
    """Two particles of instance 1 share a place: its energy is not finite, no trial is accepted, and it is stuck after
    max_halvings trials of its first step, in the state the header documents; its neighbours in the batch do not notice."""
    starts = _starts(n, range(3), dtype)
    clean = starts.copy()
    starts[1, 1] = starts[1, 0]; starts[1, n + 1] = starts[1, n]; starts[1, 2 * n + 1] = starts[1, 2 * n]   # particles 0 and 1 coincide
    _, bad = _make(starts, n, m)
    bad.set_max_halvings(halvings)
    _, ref = _make(clean, n, m)
    ref.set_max_halvings(halvings)
    history = ("HISTORY_COUNTS", "S", "Y", "RHO")
    first = {name: bad.read(getattr(dzo, "LBFGS_BATCH_" + name)) for name in VECTORS}        # S, Y and RHO as they are stored
    active = [bad.count_active()]
    for _ in range(4):
        bad.step(25); ref.step(25)
        active.append(bad.count_active())
    assert bad.is_stuck[1] and bad.last_halvings[1] == halvings and bad.iteration_counts[1] == 0
    assert all(x >= y for x, y in zip(active, active[1:])), active
    _assert_same_state(_state(bad), _state(ref), "neighbours of a singular instance", [0, 2], [0, 2])
    last = {name: bad.read(getattr(dzo, "LBFGS_BATCH_" + name)) for name in VECTORS}
    assert _same(last["POINTS"][1], starts[1]) and _same(last["DELTA_POINTS"][1], starts[1]), "delta_point holds the old point"
    assert _same(last["DELTA_GRADIENTS"][1], first["DELTA_GRADIENTS"][1]) and not last["DELTA_GRADIENTS"][1].any()
    assert last["HISTORY_COUNTS"][1] == 0
    for name in history + ("GRADIENTS", "OBJECTIVES", "DELTA_OBJECTIVES"):
        assert _same(last[name][1], first[name][1]), (name, "changed in the step that got stuck")


def test_count_active_falls_to_zero_and_the_handle_aliases_its_points():
    n = 13
    dev, opt = _make(_starts(n, range(6), np.float64), n)
    counts = [opt.count_active()]
    while counts[-1] > 0 and len(counts) < 400:
        opt.step(5)
        counts.append(opt.count_active())
    assert counts[0] == 6 and counts[-1] == 0 and all(x >= y for x, y in zip(counts, counts[1:])), counts
    assert opt.ptr(dzo.LBFGS_BATCH_POINTS) == dev.ptr
    e = dzo.pairwise_batch_energy_gradient(dev, n)            # the caller's array holds the minima
    assert _same(e, opt.current_objective_values) and np.all(np.abs(e - tw.LJ13) <= 5e-7)
    assert _same(dev.to_host().reshape(6, 3 * n), opt.current_points)


def test_error_codes():
    L = dzo.lib()
    n, batch = 13, 4
    x = dzo.DeviceArray.from_host(_starts(n, range(batch), np.float64).ravel())
    e, g = dzo.DeviceArray.zeros(batch), dzo.DeviceArray.zeros(batch * 3 * n)
    host = np.zeros(batch * 3 * n)
    h = C.c_void_p()
    LJ, F64 = dzo.RADIAL_LENNARD_JONES, dzo.F64
    INVALID, ASSERT, UNSUPPORTED = 1, 3, 5
    create = lambda radial, nn, bb, dt, p, step, m, out=C.byref(h): L.dzo_lbfgs_batch_create(radial, nn, bb, dt, p, step, m, out)
    assert create(7, n, batch, F64, x.ptr, 0.01, 10) == INVALID
    assert create(LJ, n, batch, 9, x.ptr, 0.01, 10) == INVALID
    assert create(LJ, 0, batch, F64, x.ptr, 0.01, 10) == INVALID
    assert create(LJ, n, 0, F64, x.ptr, 0.01, 10) == INVALID
    assert create(LJ, n, batch, F64, x.ptr, 0.01, 0) == INVALID
    assert create(LJ, n, batch, F64, None, 0.01, 10) == INVALID
    assert create(LJ, n, batch, F64, x.ptr, 0.01, 10, None) == INVALID
    assert create(LJ, 1025, batch, F64, x.ptr, 0.01, 10) == UNSUPPORTED
    assert create(LJ, n, batch, F64, x.ptr, 0.01, 33) == UNSUPPORTED
    assert create(LJ, n, batch, F64, host.ctypes.data, 0.01, 10) == ASSERT
    assert create(LJ, n, batch, F64, x.ptr, 0.0, 10) == ASSERT
    assert h.value is None
    assert create(LJ, n, batch, F64, x.ptr, 0.01, 32) == 0 and h.value
    assert L.dzo_lbfgs_batch_step(h, -1, None) == INVALID
    assert L.dzo_lbfgs_batch_step(None, 1, None) == INVALID
    assert L.dzo_lbfgs_batch_set_max_halvings(h, 0) == INVALID
    assert L.dzo_lbfgs_batch_count_active(h, None) == INVALID
    assert L.dzo_lbfgs_batch_read(h, 99, host.ctypes.data) == INVALID
    assert L.dzo_lbfgs_batch_read(h, dzo.LBFGS_BATCH_POINTS, None) == INVALID
    p = C.c_void_p()
    assert L.dzo_lbfgs_batch_get_ptr(h, 99, C.byref(p)) == INVALID and L.dzo_lbfgs_batch_get_ptr(h, dzo.LBFGS_BATCH_POINTS, None) == INVALID
    flag = C.c_int32(-1)
    assert L.dzo_lbfgs_batch_step(h, 0, C.byref(flag)) == 0 and flag.value == 0
    assert L.dzo_lbfgs_batch_step(h, 3, C.byref(flag)) == 0 and flag.value == 0      # history_length 32: the large LDS request
    assert L.dzo_lbfgs_batch_destroy(h) == 0 and L.dzo_lbfgs_batch_destroy(None) == 0
    ev = L.dzo_pairwise_batch_energy_gradient
    assert ev(LJ, n, batch, F64, x.ptr, e.ptr, g.ptr) == 0 and ev(LJ, n, batch, F64, x.ptr, e.ptr, None) == 0
    assert ev(7, n, batch, F64, x.ptr, e.ptr, g.ptr) == INVALID and ev(LJ, n, batch, 9, x.ptr, e.ptr, g.ptr) == INVALID
    assert ev(LJ, 0, batch, F64, x.ptr, e.ptr, g.ptr) == INVALID and ev(LJ, n, 0, F64, x.ptr, e.ptr, g.ptr) == INVALID
    assert ev(LJ, n, batch, F64, None, e.ptr, g.ptr) == INVALID and ev(LJ, n, batch, F64, x.ptr, None, g.ptr) == INVALID
    assert ev(LJ, 1025, batch, F64, x.ptr, e.ptr, g.ptr) == UNSUPPORTED
    assert ev(LJ, n, batch, F64, x.ptr, host.ctypes.data, g.ptr) == ASSERT and ev(LJ, n, batch, F64, host.ctypes.data, e.ptr, g.ptr) == ASSERT
    with pytest.raises(dzo.DzoError) as err:
        dzo.BatchedLBFGS(dzo.DeviceArray.zeros(3 * 1025), 1025, 0.01, 10)
    assert err.value.code == UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES)
def test_history_in_device_memory_matches_history_in_lds(dtype):
    """N = 1024 keeps the history ring in the handle's global slab from history_length 5 (fp32) / 1 (fp64) on.  The path follows
    from (N, m, T), so no instance runs on both; what the two have in common is the oracle and the single-step launches.  Over
    m + 3 steps, which turn the ring past its end: the invariants (consistency, deltas, decrease), every direction against the
    oracle and the twin on the state read before it with the ring shifting by one, and one launch of m + 3 steps against
    m + 3 launches of one and against step(m) + step(3), bit for bit.  tests/test_gpu_quench_shapes.py holds the shapes on either
    side of the LDS limit, (97, 32) | (98, 32) and others, to the same checks."""
    n, m = 1024, {np.dtype(np.float64): 1, np.dtype(np.float32): 5}[np.dtype(dtype)]
    assert qc.path(n, m, dtype) == qc.BLOCK_SLAB
    points = _starts(n, range(2), dtype)
    dev, opt = _make(points, n, m)
    prev = _state(opt)
    for k in range(1, 4):
        opt.step(1)
        cur = _state(opt)
        _consistent(opt, n, cur, (n, k))
        assert np.array_equal(cur["DELTA_POINTS"], cur["POINTS"] - prev["POINTS"]) and np.array_equal(cur["DELTA_GRADIENTS"], cur["GRADIENTS"] - prev["GRADIENTS"])
        assert np.all(cur["OBJECTIVES"] < prev["OBJECTIVES"]) and np.all(cur["ITERATION_COUNTS"] == k)
        assert _same(cur["S"][:, 0], cur["DELTA_POINTS"]) and (k == 1 or m == 1 or _same(cur["S"][:, 1], prev["S"][:, 0]))
        prev = cur
    _, opt = _make(points, n, m)
    worst = qc.check_directions_and_ring(opt, n, m, dtype, m + 3)
    print(f"N={n} m={m} {np.dtype(dtype).name}: worst direction error / tolerance {worst:.4f}")
    qc.check_one_launch_against_many(points, n, m, m + 3)


# ------------------------------------------------------------------------------ 8. tempering hand-over
@pytest.mark.parametrize("dtype", DTYPES)
def test_tempering_quench_leaves_the_chain_alone(dtype):
    n, replicas = 38, 16
    rdev = dzo.DeviceArray.from_host(_starts(n, range(replicas), dtype).ravel())
    beta = np.geomspace(20.0, 3.0, replicas)
    pt = dzo.ParallelTempering(rdev, n, beta, [0.05] * replicas, 3.0, base_seed=5)
    pt.run(200, 2)
    before = rdev.to_host()
    e_before = dzo.pairwise_batch_energy_gradient(rdev, n)
    energies, minima, opt = pt.quench(max_steps=2000 if dtype == np.float64 else 200)
    assert _same(rdev.to_host(), before), "the quench touched the Markov chain's replicas"
    assert minima.ptr != rdev.ptr and energies.shape == (replicas,)
    assert np.all(energies <= e_before), (energies, e_before)
    st = _state(opt)
    _consistent(opt, n, st, "quenched copy")
    assert _same(minima.to_host().reshape(replicas, 3 * n), st["POINTS"]) and _same(energies, st["OBJECTIVES"])
    if dtype == np.float64:
        assert opt.is_stuck.all()


# ------------------------------------------------------------------------------ 9. the plain-C example
def test_lj_quench_example_runs(tmp_path):
    dzo.build()
    exe = str(tmp_path / "lj_quench")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lj_quench.c"),
                    "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout and "instances not stuck: 0" in r.stdout
    lowest = float(re.search(r"lowest minimum: (-?[0-9.]+)", r.stdout).group(1))
    assert lowest >= tw.LJ38 - 5e-7
