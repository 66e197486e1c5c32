"""GPU tests of the batched AdGD optimizer (dzo_adgd_batch_*): the live AdGDOptimizer of src/DZOptimization.jl:179-312 over many
small Lennard-Jones clusters in one launch, held to the arithmetic include/dzo.h states for it.

1. the invariants of a step, exact, after every one of 50 single steps;
2. objective and gradient against the longdouble twin with the DERIVED bound of tests/test_gpu_pairwise.py, (N + 32) u S;
3. the step-size rule against the twin's on the state read before the step;
4. a replay of every step: the point is fma(-(s 2^-h), g_old, x_old) exactly, and the twin's energies agree with every decision
   (trials inside the bound are undecided; tests/test_adgd_batch_twin.py shows the inputs have none inside the windows);
5. runs to the literature minima, next to the one-at-a-time AdGDOptimizer;
6. independence of batch and position, determinism, and launch splitting, bit for bit;
7. the shape edges;  8. edges and error codes;  9. the tempering hand-over;  10. the plain-C example.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adgd_batch_twin as at
import pairwise_twin as tw
import quench_twin as qt
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
LD = np.longdouble
U = qt.U
DTYPES = [np.float64, np.float32]
NS = at.NS
VECTORS = ["POINTS", "GRADIENTS", "DELTA_POINTS", "DELTA_GRADIENTS", "OBJECTIVES", "DELTA_OBJECTIVES", "IS_STUCK", "ITERATION_COUNTS",
           "CURRENT_STEP_SIZES", "PREVIOUS_STEP_SIZES", "LAST_HALVINGS"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    dzo.init(0)


# ------------------------------------------------------------------------------ the handle's state, bit for bit
def _make(points, n, step=0.01):
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(points).ravel())
    return dev, dzo.BatchedAdGD(dev, n, step)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _state(opt):
    return {name: opt.read(getattr(dzo, "ADGD_BATCH_" + name)) for name in VECTORS}


def _assert_same_state(a, b, what, rows_a=slice(None), rows_b=slice(None)):
    for name in VECTORS:
        assert _same(a[name][rows_a], b[name][rows_b]), (what, name)


def _consistent(opt, n, st, what):
    """The stored objective and gradient are those of the stored point, bit for bit."""
    gdev = dzo.DeviceArray.zeros(opt.batch * 3 * n, opt.dtype)
    e = dzo.pairwise_batch_energy_gradient(opt.points, n, gdev)
    assert _same(e, st["OBJECTIVES"]), (what, "objective")
    assert _same(gdev.to_host().reshape(opt.batch, 3 * n), st["GRADIENTS"]), (what, "gradient")


def _check_step(prev, cur, b, where):
    """What one step!() may have done to instance b: nothing (it was stuck), found it stuck, or accepted a trial."""
    if prev["IS_STUCK"][b]:
        for name in VECTORS:
            assert _same(cur[name][b], prev[name][b]), (where, name, "a stuck instance changed")
        return
    assert _same(cur["PREVIOUS_STEP_SIZES"][b], prev["CURRENT_STEP_SIZES"][b]), (where, ":298")
    if cur["IS_STUCK"][b]:
        for name in ("POINTS", "GRADIENTS", "OBJECTIVES", "DELTA_OBJECTIVES", "DELTA_GRADIENTS", "ITERATION_COUNTS"):
            assert _same(cur[name][b], prev[name][b]), (where, name, "changed in the step that got stuck")
        assert _same(cur["DELTA_POINTS"][b], prev["POINTS"][b]), (where, "delta_point holds the old point")
        return
    assert np.array_equal(cur["DELTA_POINTS"][b], cur["POINTS"][b] - prev["POINTS"][b]), where
    assert np.array_equal(cur["DELTA_GRADIENTS"][b], cur["GRADIENTS"][b] - prev["GRADIENTS"][b]), where
    assert cur["OBJECTIVES"][b] < prev["OBJECTIVES"][b], where
    assert cur["DELTA_OBJECTIVES"][b] == cur["OBJECTIVES"][b] - prev["OBJECTIVES"][b], where
    assert cur["ITERATION_COUNTS"][b] == prev["ITERATION_COUNTS"][b] + 1, where


def _replay_step(prev, cur, b, n, dtype, decide, where):
    """The accepted point is the fused multiply-add of the header, bit for bit; with `decide`, every trial of the step against the
    longdouble energies.  Returns (trials, undecided)."""
    t = np.dtype(dtype).type
    if prev["IS_STUCK"][b]:
        return 0, 0
    x_old, g_old = prev["POINTS"][b], prev["GRADIENTS"][b]
    s, h, stuck = cur["CURRENT_STEP_SIZES"][b], int(cur["LAST_HALVINGS"][b]), bool(cur["IS_STUCK"][b])
    trial = lambda hh: at.fma(-(s * t(2.0 ** -hh)), g_old, x_old, dtype)
    if not stuck:
        assert _same(cur["POINTS"][b], trial(h)), (where, h, "the point is not fma(-(s 2^-h), g, x)")
    if not decide:
        return 0, 0
    trials = undecided = 0
    old = qt.exact_energy(x_old)
    for hh in range((h if not stuck else h - 1) + 1):
        diff, bound = qt.decision_margin(x_old, trial(hh), dtype, old)
        trials += 1
        if abs(diff) <= bound:
            undecided += 1
        elif hh == h and not stuck:
            assert diff <= bound, (where, hh, "accepted a trial that does not decrease", float(diff), float(bound))
        else:
            assert diff >= -bound, (where, hh, "rejected a trial that decreases", float(diff), float(bound))
    return trials, undecided


# ------------------------------------------------------------------------------ 1. invariants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_step_invariants(n, dtype):
    dev, opt = _make(at.starts(n, range(8), dtype), n)
    prev = _state(opt)
    _consistent(opt, n, prev, (n, 0))
    assert not prev["IS_STUCK"].any() and not prev["ITERATION_COUNTS"].any() and not prev["LAST_HALVINGS"].any()
    assert not prev["DELTA_POINTS"].any() and not prev["DELTA_GRADIENTS"].any() and not prev["DELTA_OBJECTIVES"].any()
    assert _same(prev["CURRENT_STEP_SIZES"], prev["PREVIOUS_STEP_SIZES"]) and np.all(prev["CURRENT_STEP_SIZES"] > 0)
    for k in range(1, 51):
        opt.step(1)
        cur = _state(opt)
        _consistent(opt, n, cur, (n, k))
        for b in range(opt.batch):
            _check_step(prev, cur, b, (n, np.dtype(dtype).name, k, b))
        prev = cur
    assert prev["ITERATION_COUNTS"].min() >= 5, prev["ITERATION_COUNTS"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_constructor_step_sizes(dtype):
    """:229-241: current = previous = T(initial_step_length) / T(sqrt(g0.g0)).  The device's fp64 sum of 3N non-negative terms
    and numpy's are each within (3N - 1) 2^-53 of the exact sum, relatively: after the root they differ by (3N - 1) 2^-53.  Two
    roundings of the root, to T and of the quotient follow on either side, at most 4 u_T together: relative (3N + 4) u_T."""
    t = np.dtype(dtype).type
    for n in NS:
        dev, opt = _make(at.starts(n, range(4), dtype), n, 0.25)
        g = opt.current_gradients.astype(np.float64)
        want = np.array([t(0.25) / t(np.sqrt(np.dot(r, r))) for r in g])
        got = opt.current_step_sizes
        tol = float((3 * n + 4) * U[np.dtype(dtype)])
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol * want), (n, got, want)
        assert _same(got, opt.previous_step_sizes)


# ------------------------------------------------------------------------------ 2. against the longdouble twin
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_objective_and_gradient_against_the_twin(n, dtype):
    dev, opt = _make(at.starts(n, range(4), dtype), n)
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


# ------------------------------------------------------------------------------ 3. the step-size rule
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_step_size_rule_against_the_twin(n, dtype):
    """Steps 1 .. 20.  Where sqrt(1 + theta) gives the smaller candidate the device's value has the twin's bits (no sum enters).
    Otherwise the two fp64 sums of 3N non-negative terms each may differ by 3N 2^-53 relatively between summation orders, and a
    handful of roundings in T follow: relative (6N + 8) u_T.  Where the two candidates are closer than that, either may win."""
    dev, opt = _make(at.starts(n, range(4), dtype), n)
    tol = float((6 * n + 8) * U[np.dtype(dtype)])
    exact = capped = 0
    worst = 0.0
    for k in range(1, 21):
        before = _state(opt)
        opt.step(1)
        cur = opt.current_step_sizes
        for b in range(opt.batch):
            if before["IS_STUCK"][b]:
                continue
            where = (n, np.dtype(dtype).name, k, b)
            c0, p0 = before["CURRENT_STEP_SIZES"][b], before["PREVIOUS_STEP_SIZES"][b]
            if before["ITERATION_COUNTS"][b] == 0:
                assert _same(cur[b], c0), (where, "the first step takes current_step_size as it is (:288)")
                continue
            grown, cap = at.step_size_candidates(before["DELTA_POINTS"][b], before["DELTA_GRADIENTS"][b], c0, p0, dtype)
            want = at.next_step_size(before["DELTA_POINTS"][b], before["DELTA_GRADIENTS"][b], c0, p0, dtype)
            if cap is None or float(grown) < float(cap) * (1.0 - tol):
                assert _same(cur[b], grown), (where, cur[b], grown)
                exact += 1
            else:
                err = abs(float(cur[b]) - float(want)) / float(want)
                worst = max(worst, err / tol)
                assert err <= tol, (where, cur[b], want, err, tol)
                capped += 1
    print(f"N={n} {np.dtype(dtype).name}: {exact} steps on the sqrt(1 + theta) branch, {capped} capped, worst error / tolerance {worst:.4f}")
    assert exact > 0 and capped > 0, "both candidates of the min must have been taken"


# ------------------------------------------------------------------------------ 4. step replay
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("step_length", [0.01, 1.0])
@pytest.mark.parametrize("n", NS)
def test_step_replay(n, step_length, dtype):
    window = at.WINDOWS[step_length][np.dtype(dtype)]
    dev, opt = _make(at.starts(n, at.SEEDS, dtype), n, step_length)
    undecided = trials = 0
    halvings = []
    prev = _state(opt)
    for k in range(window):
        opt.step(1)
        cur = _state(opt)
        for b in range(opt.batch):
            tr, un = _replay_step(prev, cur, b, n, dtype, True, (n, step_length, np.dtype(dtype).name, k, b))
            trials += tr; undecided += un
        if k == 0:
            halvings = cur["LAST_HALVINGS"].tolist()
        prev = cur
    print(f"N={n} step length {step_length} {np.dtype(dtype).name}: {undecided} of {trials} trials undecided in the first {window} steps; "
          f"halvings of the first step {halvings}")
    assert undecided == 0


# ------------------------------------------------------------------------------ 5. the literature minima
@pytest.mark.parametrize("name,n,lit", [("ico", 13, tw.LJ13), ("oct", 38, tw.LJ38)])
def test_reaches_the_literature_minima(name, n, lit):
    starts = np.stack([qt.start(name, s) for s in range(10)])
    dev, opt = _make(starts, n)
    steps, done = 0, False
    while not done and steps < 5000:
        done = opt.step(50)
        steps += 50
    f = opt.current_objective_values
    print(f"{name}: f = {f.round(9).tolist()} after {opt.iteration_counts.tolist()} steps")
    assert done and opt.is_stuck.all() and opt.count_active() == 0
    assert np.all(np.abs(f - lit) <= 5e-7), f
    for s in range(10):
        prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n)
        one = dzo.AdGDOptimizer(None, prob, None, dzo.DeviceArray.from_host(starts[s]), 0.01)
        k = 0
        while k < 5000 and not one.is_stuck:
            one.step()
            k += 1
        assert one.is_stuck
        assert abs(one.current_objective_value - f[s]) <= 1e-9, (name, s, one.current_objective_value, f[s])


# ------------------------------------------------------------------------------ 6. independence and determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_independence_and_determinism(n, dtype):
    batch, pos = 256, 200
    starts = at.starts(n, [s % 7 for s in range(batch)], dtype)
    starts[pos] = at.start(n, 11, dtype)
    _, big = _make(starts, n)
    big.step(60)
    a = _state(big)
    assert a["ITERATION_COUNTS"].min() >= 5
    _, alone = _make(starts[pos:pos + 1], n)
    alone.step(60)
    _assert_same_state(_state(alone), a, "alone against position 200 of 256", slice(0, 1), slice(pos, pos + 1))
    _, again = _make(starts, n)
    again.step(60)
    _assert_same_state(_state(again), a, "the same batch twice")
    _, split = _make(starts, n)
    split.step(30)
    split.step(30)
    _assert_same_state(_state(split), a, "step(60) against step(30) + step(30)")
    _, lazy = _make(starts, n)
    assert lazy.step(60, wait=False) is None
    dzo.synchronize()
    _assert_same_state(_state(lazy), a, "step(.., NULL) + dzo_synchronize against the blocking form")
    for b in range(7, batch):                                # instances that share a start share every bit, wherever they sit
        if b != pos:
            _assert_same_state(a, a, f"instance {b} against {b % 7}", slice(b, b + 1), slice(b % 7, b % 7 + 1))


# ------------------------------------------------------------------------------ 7. shape edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", at.EDGE_NS)
def test_shape_edges(n, dtype):
    points = at.edge_starts(n, dtype)
    dev, opt = _make(points, n)
    prev = _state(opt)
    _consistent(opt, n, prev, (n, 0))
    assert not prev["IS_STUCK"].any()
    trials = undecided = 0
    for k in range(1, at.EDGE_STEPS + 1):
        opt.step(1)
        cur = _state(opt)
        _consistent(opt, n, cur, (n, k))
        for b in range(opt.batch):
            where = (n, np.dtype(dtype).name, k, b)
            _check_step(prev, cur, b, where)
            tr, un = _replay_step(prev, cur, b, n, dtype, True, where)
            trials += tr; undecided += un
        prev = cur
    assert trials >= at.EDGE_STEPS * opt.batch and undecided == 0, (trials, undecided)
    assert np.all(prev["ITERATION_COUNTS"] == at.EDGE_STEPS), prev["ITERATION_COUNTS"]
    _, one = _make(points, n)
    one.step(at.EDGE_STEPS)
    _assert_same_state(_state(one), prev, f"step({at.EDGE_STEPS}) against {at.EDGE_STEPS} x step(1)")


# ------------------------------------------------------------------------------ 8. edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_particle_is_stuck_at_creation(dtype):
    dev, opt = _make(np.array([[0.25, -1.0, 3.0]] * 3, dtype=dtype), 1)
    st = _state(opt)
    assert st["IS_STUCK"].all() and opt.count_active() == 0
    assert not st["OBJECTIVES"].any() and not st["GRADIENTS"].any()
    assert not st["CURRENT_STEP_SIZES"].any() and not st["PREVIOUS_STEP_SIZES"].any()
    assert opt.step(5) is True
    _assert_same_state(_state(opt), st, "N = 1 after step")


@pytest.mark.parametrize("n", [38, 200])
def test_coincident_particles_do_not_disturb_the_neighbours(n):
    """Two particles of instance 1 share a place: its energy is not finite, no trial is accepted, and it is stuck after
    max_halvings trials of its first step, in the state the header documents; its neighbours in the batch do not notice."""
    halvings = 8
    starts = at.starts(n, range(3), np.float64)
    clean = starts.copy()
    starts[1, 1] = starts[1, 0]; starts[1, n + 1] = starts[1, n]; starts[1, 2 * n + 1] = starts[1, 2 * n]   # particles 0 and 1 coincide
    _, bad = _make(starts, n)
    bad.set_max_halvings(halvings)
    _, ref = _make(clean, n)
    ref.set_max_halvings(halvings)
    first = _state(bad)
    active = [bad.count_active()]
    for _ in range(4):
        bad.step(25); ref.step(25)
        active.append(bad.count_active())
    last = _state(bad)
    assert last["IS_STUCK"][1] and last["LAST_HALVINGS"][1] == halvings and last["ITERATION_COUNTS"][1] == 0
    assert all(x >= y for x, y in zip(active, active[1:])), active
    _assert_same_state(last, _state(ref), "neighbours of a singular instance", [0, 2], [0, 2])
    assert _same(last["POINTS"][1], starts[1]) and _same(last["DELTA_POINTS"][1], starts[1]), "delta_point holds the old point"
    assert not last["DELTA_GRADIENTS"][1].any()
    for name in ("GRADIENTS", "OBJECTIVES", "DELTA_OBJECTIVES", "DELTA_GRADIENTS"):
        assert _same(last[name][1], first[name][1]), (name, "changed in the step that got stuck")
    assert _same(last["PREVIOUS_STEP_SIZES"][1], first["CURRENT_STEP_SIZES"][1])


def test_count_active_falls_to_zero_and_the_handle_aliases_its_points():
    n = 13
    dev, opt = _make(at.starts(n, range(6), np.float64), n)
    counts = [opt.count_active()]
    while counts[-1] > 0 and len(counts) < 400:
        opt.step(5)
        counts.append(opt.count_active())
    assert counts[0] == 6 and counts[-1] == 0 and all(x >= y for x, y in zip(counts, counts[1:])), counts
    assert opt.ptr(dzo.ADGD_BATCH_POINTS) == dev.ptr
    e = dzo.pairwise_batch_energy_gradient(dev, n)            # the caller's array holds the minima
    assert _same(e, opt.current_objective_values) and np.all(np.abs(e - tw.LJ13) <= 5e-7)
    assert _same(dev.to_host().reshape(6, 3 * n), opt.current_points)
    opt.close()
    opt.close()


def test_error_codes():
    L = dzo.lib()
    n, batch = 13, 4
    x = dzo.DeviceArray.from_host(at.starts(n, range(batch), np.float64).ravel())
    host = np.zeros(batch * 3 * n)
    h = C.c_void_p()
    LJ, F64 = dzo.RADIAL_LENNARD_JONES, dzo.F64
    INVALID, ASSERT, UNSUPPORTED = 1, 3, 5
    create = lambda radial, nn, bb, dt, p, step, out=C.byref(h): L.dzo_adgd_batch_create(radial, nn, bb, dt, p, step, out)
    assert create(7, n, batch, F64, x.ptr, 0.01) == INVALID
    assert create(LJ, n, batch, 9, x.ptr, 0.01) == INVALID
    assert create(LJ, 0, batch, F64, x.ptr, 0.01) == INVALID
    assert create(LJ, n, 0, F64, x.ptr, 0.01) == INVALID
    assert create(LJ, n, batch, F64, None, 0.01) == INVALID
    assert create(LJ, n, batch, F64, x.ptr, 0.01, None) == INVALID
    assert create(LJ, 1025, batch, F64, x.ptr, 0.01) == UNSUPPORTED
    assert create(LJ, n, batch, F64, host.ctypes.data, 0.01) == ASSERT
    assert create(LJ, n, batch, F64, x.ptr, 0.0) == ASSERT
    assert create(LJ, n, batch, F64, x.ptr, -1.0) == ASSERT
    assert h.value is None
    assert create(LJ, n, batch, F64, x.ptr, 0.01) == 0 and h.value
    assert L.dzo_adgd_batch_step(h, -1, None) == INVALID
    assert L.dzo_adgd_batch_step(None, 1, None) == INVALID
    assert L.dzo_adgd_batch_set_max_halvings(h, 0) == INVALID and L.dzo_adgd_batch_set_max_halvings(None, 8) == INVALID
    assert L.dzo_adgd_batch_count_active(h, None) == INVALID
    assert L.dzo_adgd_batch_read(h, 11, host.ctypes.data) == INVALID and L.dzo_adgd_batch_read(h, -1, host.ctypes.data) == INVALID
    assert L.dzo_adgd_batch_read(h, dzo.ADGD_BATCH_POINTS, None) == INVALID
    p = C.c_void_p()
    assert L.dzo_adgd_batch_get_ptr(h, 99, C.byref(p)) == INVALID and L.dzo_adgd_batch_get_ptr(h, dzo.ADGD_BATCH_POINTS, None) == INVALID
    flag = C.c_int32(-1)
    assert L.dzo_adgd_batch_step(h, 0, C.byref(flag)) == 0 and flag.value == 0
    assert L.dzo_adgd_batch_step(h, 3, C.byref(flag)) == 0 and flag.value == 0
    assert L.dzo_adgd_batch_set_max_halvings(h, 1) == 0
    assert L.dzo_adgd_batch_destroy(h) == 0 and L.dzo_adgd_batch_destroy(None) == 0
    with pytest.raises(dzo.DzoError) as err:
        dzo.BatchedAdGD(dzo.DeviceArray.zeros(3 * 1025), 1025, 0.01)
    assert err.value.code == UNSUPPORTED


# ------------------------------------------------------------------------------ 9. tempering hand-over
@pytest.mark.parametrize("dtype", DTYPES)
def test_tempering_quench_with_adgd_leaves_the_chain_alone(dtype):
    n, replicas = 38, 16
    rdev = dzo.DeviceArray.from_host(at.starts(n, range(replicas), dtype).ravel())
    beta = np.geomspace(20.0, 3.0, replicas)
    pt = dzo.ParallelTempering(rdev, n, beta, [0.05] * replicas, 3.0, base_seed=5)
    pt.run(200, 2)
    before = rdev.to_host()
    e_before = dzo.pairwise_batch_energy_gradient(rdev, n)
    energies, minima, opt = pt.quench(max_steps=5000 if dtype == np.float64 else 200, optimizer="adgd")
    assert isinstance(opt, dzo.BatchedAdGD)
    assert _same(rdev.to_host(), before), "the quench touched the Markov chain's replicas"
    assert minima.ptr != rdev.ptr and energies.shape == (replicas,)
    assert np.all(energies <= e_before), (energies, e_before)
    st = _state(opt)
    _consistent(opt, n, st, "quenched copy")
    assert _same(minima.to_host().reshape(replicas, 3 * n), st["POINTS"]) and _same(energies, st["OBJECTIVES"])
    if dtype == np.float64:
        assert opt.is_stuck.all()
    _, _, default = pt.quench(max_steps=50)
    assert isinstance(default, dzo.BatchedLBFGS)
    assert _same(rdev.to_host(), before)


# ------------------------------------------------------------------------------ 10. the plain-C example
def test_lj_adgd_quench_example_runs(tmp_path):
    dzo.build()
    exe = str(tmp_path / "lj_adgd_quench")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lj_adgd_quench.c"),
                    "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout and "instances not stuck: 0" in r.stdout
    lowest = float(re.search(r"lowest minimum: (-?[0-9.]+)", r.stdout).group(1))
    assert lowest >= tw.LJ38 - 5e-7
