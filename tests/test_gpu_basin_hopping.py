"""The device's batched basin hopping (csrc/dzo_basin_hopping.hip) against the rule of include/dzo.h, on the GPU.

A Metropolis walk cannot be compared value by value with another implementation, so the device RECORDS each hop and the test
replays it (tests/basin_twin.py):

(a) the recorded normals are numpy's Box-Muller of the stated draws (particle i: draws 4i .. 4i+3 of the hop's 4N + 1) within
    the bound tests/test_gpu_tempering.py derives for REC_NORMALS; the uniform is draw 4N, bit for bit;
(b) the trial is rebuilt in numpy from the recorded normals, bit for bit (a product and a sum in T, the sphere test in T);
(c) ONE dzo.BatchedLBFGS over all walkers' trials, step(quench_steps), gives REC_TRIAL_ENERGY and REC_QUENCH_ITERATIONS bit
    for bit;
(d) delta = E_q - E is one subtraction of two values the replay holds bit for bit, so it is exact, and the decision must be
    the class of classify(delta, 0, u, beta).  A hop whose uniform lies within the few ulp of exp's rounding around the
    threshold is undecided; the cap on those is zero over the whole file (the seeds are fixed).

At the end POINTS, ENERGIES, BEST_*, RNG_STATES, the counters and RADII are the replay's bit for bit, and POINTS / ENERGIES
agree with dzo.pairwise_batch_energy_gradient.  Every case runs a handful of hops of 3 .. 5 walkers."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import basin_twin as bt
import pairwise_twin as pw
import quench_checks as qc
import tempering_twin as tt
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

LD = np.longdouble
U64 = LD(2.0) ** -53
DTYPES = [np.float64, np.float32]
LDS_MAX = 159 * 1024


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.int8}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _make(points, n, beta, radii, R, seed, m=10, quench_steps=400, record=0, max_halvings=None):
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(points).reshape(-1))
    bh = dzo.BasinHopping(dev, n, beta, radii, R, 0.01, m, quench_steps, seed)
    if max_halvings:
        bh.set_max_halvings(max_halvings)
    if record:
        bh.set_record(record)
    return dev, bh


def _quench(points, n, m, quench_steps, max_halvings=None):
    """dzo_lbfgs_batch_create + step(quench_steps) on a copy: (points, energies, iterations, stuck)"""
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(points).reshape(-1))
    opt = dzo.BatchedLBFGS(dev, n, 0.01, m)
    if max_halvings:
        opt.set_max_halvings(max_halvings)
    opt.step(quench_steps, wait=False)
    out = opt.current_points, opt.current_objective_values, opt.iteration_counts, opt.is_stuck
    opt.close()
    return out


STATE = ("POINTS", "ENERGIES", "BEST_POINTS", "BEST_ENERGIES", "RADII", "RNG_STATES", "NUM_ACCEPT", "NUM_REJECT", "HOP_COUNTS", "QUENCH_ITERATIONS",
         "QUENCH_UNFINISHED")


def _state(bh):
    return {name: bh.read(getattr(dzo, "BASIN_HOPPING_" + name)) for name in STATE}


def _assert_same_state(a, b, what, rows_a=slice(None), rows_b=slice(None), skip=()):
    for name in STATE:
        if name not in skip:
            assert _same(a[name][rows_a], b[name][rows_b]), (what, name)


def _replay(points, n, dtype, beta, radii, R, seed, m, quench_steps, hops, adapt=False, max_halvings=None, what=""):
    """Runs `hops` hops in one launch with recording on and replays them.  Returns (handle, its state, the replay's log)."""
    t = np.dtype(dtype).type
    points = np.ascontiguousarray(points, dtype=dtype)
    batch = points.shape[0]
    dev, bh = _make(points, n, beta, radii, R, seed, m, quench_steps, record=hops, max_halvings=max_halvings)
    created = _state(bh)
    x, e, _, _ = _quench(points, n, m, quench_steps)                 # create: no draws, always kept (default max_halvings)
    assert _same(created["POINTS"], x) and _same(created["ENERGIES"], e), (what, "create")
    assert _same(created["BEST_POINTS"], x) and _same(created["BEST_ENERGIES"], e), (what, "create")
    for name in ("NUM_ACCEPT", "NUM_REJECT", "HOP_COUNTS", "QUENCH_ITERATIONS", "QUENCH_UNFINISHED"):
        assert not created[name].any(), (what, name)
    states = [tt.pcg_state(seed + b) for b in range(batch)]
    assert [int(v) for v in created["RNG_STATES"]] == states
    assert _same(created["RADII"], np.asarray(radii, dtype=dtype)) and _same(bh.inverse_temperatures, np.asarray(beta, dtype=dtype))

    bh.hop(hops, adapt=adapt, hops_per_launch=hops)
    nrm, uni = bh.read(dzo.BASIN_HOPPING_REC_NORMALS), bh.read(dzo.BASIN_HOPPING_REC_UNIFORM)
    e_q, its, code = (bh.read(getattr(dzo, "BASIN_HOPPING_REC_" + s)) for s in ("TRIAL_ENERGY", "QUENCH_ITERATIONS", "CODE"))
    best_x, best_e = x.copy(), e.copy()
    acc, rej, total_its, unfinished = (np.zeros(batch, dtype=np.int64) for _ in range(4))
    log = dict(code=code, moved=[], worst_normal=0.0, delta=[])
    ut = tt.U[np.dtype(dtype)] if np.dtype(dtype) == np.float32 else LD(0)
    for i in range(hops):
        trials = np.empty_like(x)
        us = []
        for b in range(batch):
            normals, u, states[b], r = bt.hop_draws(states[b], n, np.float64, with_radii=True)
            bound = (13 * U64 + ut) * np.abs(normals).astype(LD) + 4 * LD(math.pi) * U64 * r.astype(LD)
            err = np.abs(nrm[b, i].astype(LD) - normals.astype(LD))
            log["worst_normal"] = max(log["worst_normal"], float((err / bound).max()))
            assert np.all(err <= bound), (what, "normals", i, b, float((err / bound).max()))                       # (a)
            assert _same(uni[b, i], t(u)), (what, "uniform", i, b)
            trials[b], moved = bt.trial(x[b], np.asarray(radii, dtype=dtype)[b], nrm[b, i], R, dtype)           # (b)
            log["moved"].append(moved)
            us.append(uni[b, i])
        xq, eq, itq, stuck = _quench(trials, n, m, quench_steps, max_halvings)                                  # (c)
        assert _same(e_q[:, i], eq), (what, "trial energy", i, e_q[:, i], eq)
        assert np.array_equal(its[:, i], itq.astype(np.int32)), (what, "iterations", i, its[:, i], itq)
        for b in range(batch):                                                                                   # (d)
            klass, own = bt.decide(eq[b], e[b], us[b], np.asarray(beta, dtype=dtype)[b], dtype)
            assert klass != tt.UNDECIDED, (what, "undecided hop: choose another seed", i, b)
            want = bt.CODE_NOT_FINITE if own == bt.CODE_NOT_FINITE else (bt.CODE_ACCEPTED if klass == tt.MUST_ACCEPT else bt.CODE_REJECTED)
            assert code[b, i] == want, (what, "decision", i, b, code[b, i], want)
            with np.errstate(all="ignore"):
                log["delta"].append(t(eq[b]) - t(e[b]))
            if want == bt.CODE_ACCEPTED:
                x[b], e[b] = xq[b], eq[b]
            if np.isfinite(eq[b]) and eq[b] < best_e[b]:
                best_x[b], best_e[b] = xq[b], eq[b]
            acc[b] += want == bt.CODE_ACCEPTED
            rej[b] += want != bt.CODE_ACCEPTED
        total_its += itq
        unfinished += ~stuck
    st = _state(bh)
    assert _same(st["POINTS"], x) and _same(st["ENERGIES"], e), (what, "final")
    assert _same(dev.to_host().reshape(batch, 3 * n), x), (what, "the caller's array holds the current minima")
    assert _same(st["BEST_POINTS"], best_x) and _same(st["BEST_ENERGIES"], best_e), (what, "best")
    assert [int(v) for v in st["RNG_STATES"]] == states, (what, "4N + 1 draws per hop")
    assert np.array_equal(st["NUM_ACCEPT"], acc) and np.array_equal(st["NUM_REJECT"], rej), what
    assert np.array_equal(st["HOP_COUNTS"], np.full(batch, hops)) and np.array_equal(st["QUENCH_ITERATIONS"], total_its), what
    assert np.array_equal(st["QUENCH_UNFINISHED"], unfinished), what
    want_radii = np.asarray(radii, dtype=dtype)
    if adapt:
        want_radii = np.array([tt.adapt_radius(want_radii[b], int(acc[b]), int(rej[b]), dtype) for b in range(batch)], dtype=dtype)
    assert _same(st["RADII"], want_radii), (what, "radii")
    if np.all(np.isfinite(e)):
        assert _same(dzo.pairwise_batch_energy_gradient(dev, n), e), (what, "ENERGIES is the energy of POINTS")
    log.update(its=its, unfinished=unfinished, acc=acc, rej=rej)
    return bh, st, log


def _inputs(n, dtype, batch=3):
    pts = np.stack([qc.start(n, s, dtype) for s in range(batch)])
    R = float(np.sqrt((pts.reshape(batch, 3, n).astype(np.float64) ** 2).sum(axis=1)).max() + 0.05)
    return pts, np.array([2.0, 6.0, 20.0, 1.0, 50.0][:batch]), np.full(batch, 0.05), R


def _fits(n, m, dtype):
    """the header's formula: (2 m + 6) 3N elements and the scalars (16 m + 64 bytes) within 159 KiB"""
    return (2 * m + 6) * 3 * n * np.dtype(dtype).itemsize + 16 * m + 64 <= LDS_MAX


def _ring_edges(dtype):
    """(last (N, m) whose ring fits LDS, first that does not): along N at m = 32 and along m at N = 1024 where there is one"""
    n = max(k for k in range(65, 1025) if _fits(k, 32, dtype))
    edges = [((n, 32), (n + 1, 32))]
    ms = [m for m in range(1, 33) if _fits(1024, m, dtype)]
    if ms:
        edges.append(((1024, max(ms)), (1024, max(ms) + 1)))
    return edges


def test_ring_edges_follow_the_stated_formula():
    assert _ring_edges(np.float64) == [((96, 32), (97, 32))]
    assert _ring_edges(np.float32) == [((193, 32), (194, 32)), ((1024, 3), (1024, 4))]
    assert not _fits(1024, 1, np.float64) and _fits(1024, 1, np.float32)


SHAPES = [(n, m) for n in (2, 13, 38, 64) for m in (1, 32)] + [(65, 10), (257, 10), (1024, 1)]
EDGES = sorted({case for dt in DTYPES for pair in _ring_edges(dt) for case in pair})


def _steps_of(n):
    return 400 if n <= 38 else 30 if n >= 257 else 60


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", SHAPES + [c for c in EDGES if c not in SHAPES])
def test_hops_replayed(n, m, dtype):
    """(a) .. (d) of the module's docstring and the final state, in every launch shape."""
    pts, beta, radii, R = _inputs(n, dtype)
    hops = 4
    bh, st, log = _replay(pts, n, dtype, beta, radii, R, 700 + n, m, _steps_of(n), hops, what=(n, m, np.dtype(dtype).name))
    moved = np.concatenate(log["moved"])
    print(f"basin N={n} m={m} {np.dtype(dtype).name}: codes {log['code'].tolist()}, iterations {log['its'].tolist()}, unfinished "
          f"{log['unfinished'].tolist()}, moved {int(moved.sum())}/{moved.size}, worst normal error / bound {log['worst_normal']:.3f}")
    assert moved.any()
    if n >= 257:
        assert log["unfinished"].sum() > 0, "quench_steps = 30 cuts quenches off"
    if 13 <= n <= 38:
        assert log["unfinished"].sum() == 0, "400 steps end stuck"


@pytest.fixture(scope="module")
def ico():
    """five 13-atom walkers from jittered icosahedra"""
    return np.stack([np.concatenate(pw.jittered(pw.icosahedron13(), 20 + k, 0.08)) for k in range(5)])


BETA5, RADII5 = np.array([1.25, 2.0, 4.0, 0.2, 8.0]), np.array([0.4, 0.3, 0.35, 0.45, 0.25])


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_decisions_and_the_adaptation(ico, dtype):
    """Large moves at temperature ~1: the walkers take both branches; adapt = 1 follows the rule on the counts read back."""
    bh, st, log = _replay(ico.astype(dtype), 13, dtype, BETA5, RADII5, 3.0, 31, 10, 400, 6, adapt=True, what="adapt")
    assert {0, 1} <= set(log["code"].ravel().tolist())
    uphill = [float(d) for d, c in zip(log["delta"], log["code"].T.ravel()) if c == 1 and d > 0]
    print(f"adapt {np.dtype(dtype).name}: codes {log['code'].tolist()}, accepted uphill hops {uphill}")
    acc, rej = bh.num_accept, bh.num_reject
    assert np.array_equal(acc + rej, np.full(5, 6))
    want = [tt.adapt_radius(np.dtype(dtype).type(RADII5[b]), int(acc[b]), int(rej[b]), dtype) for b in range(5)]
    assert _same(bh.perturbation_radii, np.array(want, dtype=dtype)) and not _same(bh.perturbation_radii, RADII5.astype(dtype))
    assert np.all(st["BEST_ENERGIES"] <= st["ENERGIES"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [13, 65])
def test_a_walker_alone_has_the_bits_it_has_in_a_batch(n, dtype):
    pts, beta, radii, R = _inputs(n, dtype, batch=4)
    _, all4 = _make(pts, n, beta, radii, R, 90, quench_steps=_steps_of(n))
    all4.hop(3, adapt=True)
    a = _state(all4)
    for b in (0, 3):
        _, one = _make(pts[b:b + 1], n, beta[b:b + 1], radii[b:b + 1], R, 90 + b, quench_steps=_steps_of(n))
        one.hop(3, adapt=True)
        _assert_same_state(_state(one), a, ("alone", n, b), rows_b=slice(b, b + 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [13, 65])
def test_two_calls_equal_one(n, dtype):
    """hop(2); hop(3) equals hop(5) with adapt = 0, by the C entry and by hops_per_launch."""
    pts, beta, radii, R = _inputs(n, dtype)
    _, one = _make(pts, n, beta, radii, R, 5, quench_steps=_steps_of(n))
    one.hop(5, adapt=False, hops_per_launch=5)
    a = _state(one)
    _, two = _make(pts, n, beta, radii, R, 5, quench_steps=_steps_of(n))
    two.hop(2, adapt=False)
    two.hop(3, adapt=False)
    _assert_same_state(_state(two), a, "hop(2); hop(3)", skip=("NUM_ACCEPT", "NUM_REJECT"))     # those are of the last call
    _, split = _make(pts, n, beta, radii, R, 5, quench_steps=_steps_of(n))
    split.hop(5, adapt=False, hops_per_launch=2)
    _assert_same_state(_state(split), a, "hops_per_launch = 2", skip=("NUM_ACCEPT", "NUM_REJECT"))
    assert np.array_equal(split.num_accept + split.num_reject, np.ones(3, dtype=np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_and_resume(ico, dtype):
    """A checkpoint is POINTS, RNG_STATES and RADII read back; a fresh handle at those points with the two arrays set goes on
    as the first handle did.  create quenches the points it is given: a walker continues identically where that quench leaves
    its point and energy as they are, which a minimum found in fp64 does (required here of every walker); in fp32 a stuck point
    can still move by a decrease at rounding level, and then the walker continues from where the rule puts it: the quench of
    the checkpointed point.  The streams do not depend on the points and are the first handle's in every case."""
    pts = ico[:3].astype(dtype)
    _, bh = _make(pts, 13, BETA5[:3], RADII5[:3], 3.0, 77)
    bh.hop(2, adapt=True)
    minima, energies, rng, radii = bh.current_points, bh.energies, bh.rng_states, bh.perturbation_radii
    bh.hop(3, adapt=True)
    a = _state(bh)
    _, fresh = _make(minima, 13, BETA5[:3], RADII5[:3], 3.0, 1234)
    fresh.rng_states = rng
    fresh.perturbation_radii = radii
    created = _state(fresh)
    x, e, _, _ = _quench(minima, 13, 10, 400)
    assert _same(created["POINTS"], x) and _same(created["ENERGIES"], e) and _same(created["RNG_STATES"], rng) and _same(created["RADII"], radii)
    fixed = [b for b in range(3) if _same(x[b], minima[b]) and _same(e[b], energies[b])]
    print(f"checkpoint {np.dtype(dtype).name}: walkers whose checkpointed point is a fixed point of the quench: {fixed}")
    if np.dtype(dtype) == np.float64:
        assert fixed == [0, 1, 2]
    fresh.hop(3, adapt=True)
    b_state = _state(fresh)
    assert _same(b_state["RNG_STATES"], a["RNG_STATES"])
    for b in fixed:
        # BEST_* and the totals belong to the handle's own history
        _assert_same_state(b_state, a, ("resume", b), rows_a=slice(b, b + 1), rows_b=slice(b, b + 1),
                           skip=("BEST_POINTS", "BEST_ENERGIES", "HOP_COUNTS", "QUENCH_ITERATIONS", "QUENCH_UNFINISHED"))
    _, again = _make(minima, 13, BETA5[:3], RADII5[:3], 3.0, 99)
    again.rng_states = rng
    again.perturbation_radii = radii
    again.hop(3, adapt=True)
    _assert_same_state(_state(again), b_state, "the same checkpoint twice")


@pytest.mark.parametrize("dtype", DTYPES)
def test_constraining_radius(ico, dtype):
    """An infinite radius moves every particle; a tiny one moves none: the trial is the minimum and the hop is accepted with
    delta <= 0."""
    pts = ico[:3].astype(dtype)
    bh, st, log = _replay(pts, 13, dtype, BETA5[:3], RADII5[:3], math.inf, 11, 10, 400, 4, what="infinite radius")
    assert np.concatenate(log["moved"]).all()
    bh, st, log = _replay(pts, 13, dtype, BETA5[:3], RADII5[:3], 1e-3, 11, 10, 400, 4, what="tiny radius")
    assert not np.concatenate(log["moved"]).any()
    assert np.all(log["code"] == 1) and all(d <= 0 for d in log["delta"])
    assert _same(st["ENERGIES"], st["BEST_ENERGIES"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_particles(ico, dtype):
    """Walker 1 starts with two particles at one place: its energy is not a number and stays; every hop of it is rejected (code
    0: the comparisons with NaN fail; or 2 where the quench itself ends at a non-finite energy) and BEST_* never changes.  The
    other walkers are not affected."""
    pts = ico[:3].astype(dtype).copy()
    pts[1].reshape(3, 13)[:, 5] = pts[1].reshape(3, 13)[:, 4]
    bh, st, log = _replay(pts, 13, dtype, BETA5[:3], RADII5[:3], 3.0, 3, 10, 400, 4, what="coincident")
    assert np.isnan(st["ENERGIES"][1]) and np.isnan(st["BEST_ENERGIES"][1])
    assert set(log["code"][1].tolist()) <= {0, 2} and log["acc"][1] == 0
    assert np.all(np.isfinite(st["ENERGIES"][[0, 2]])) and _same(st["POINTS"][1], _quench(pts, 13, 10, 400)[0][1])


def test_error_codes(ico):
    L = dzo.lib()
    n, batch = 13, 3
    x = dzo.DeviceArray.from_host(ico[:batch].ravel())
    host = np.zeros(batch * 3 * n)
    beta = (C.c_double * batch)(1.0, 2.0, 3.0)
    radii = (C.c_double * batch)(0.1, 0.1, 0.1)
    h = C.c_void_p()
    LJ, F64 = dzo.RADIAL_LENNARD_JONES, dzo.F64
    INVALID, ASSERT, UNSUPPORTED, STATE = 1, 3, 5, 6

    def create(radial=LJ, nn=n, bb=batch, dt=F64, p=x.ptr, be=beta, ra=radii, R=3.0, step=0.01, m=10, qs=50, out=C.byref(h)):
        return L.dzo_basin_hopping_create(radial, nn, bb, dt, p, be, ra, R, step, m, qs, 1, out)

    assert create(radial=7) == INVALID and create(dt=9) == INVALID
    assert create(nn=0) == INVALID and create(bb=0) == INVALID
    assert create(qs=0) == INVALID and create(m=0) == INVALID
    assert create(p=None) == INVALID and create(be=None) == INVALID and create(ra=None) == INVALID and create(out=None) == INVALID
    assert create(R=0.0) == INVALID and create(R=-1.0) == INVALID and create(R=math.nan) == INVALID
    assert create(nn=1025) == UNSUPPORTED and create(m=33) == UNSUPPORTED
    assert create(p=host.ctypes.data) == ASSERT and create(step=0.0) == ASSERT
    assert h.value is None
    assert create(R=math.inf, m=32) == 0 and h.value                                  # history_length 32: the large LDS request
    assert L.dzo_basin_hopping_hop(h, -1, 0) == INVALID and L.dzo_basin_hopping_hop(None, 1, 0) == INVALID
    assert L.dzo_basin_hopping_set_max_halvings(h, 0) == INVALID and L.dzo_basin_hopping_set_max_halvings(None, 5) == INVALID
    assert L.dzo_basin_hopping_read(h, 99, host.ctypes.data) == INVALID
    assert L.dzo_basin_hopping_read(h, dzo.BASIN_HOPPING_POINTS, None) == INVALID
    assert L.dzo_basin_hopping_read(h, dzo.BASIN_HOPPING_REC_CODE, host.ctypes.data) == STATE   # nothing is being recorded
    p = C.c_void_p()
    assert L.dzo_basin_hopping_get_ptr(h, 99, C.byref(p)) == INVALID and L.dzo_basin_hopping_get_ptr(h, dzo.BASIN_HOPPING_POINTS, None) == INVALID
    assert L.dzo_basin_hopping_get_ptr(h, dzo.BASIN_HOPPING_POINTS, C.byref(p)) == 0 and p.value == x.ptr
    assert L.dzo_basin_hopping_set(h, dzo.BASIN_HOPPING_POINTS, host.ctypes.data) == INVALID   # RADII and RNG_STATES only
    assert L.dzo_basin_hopping_set(h, dzo.BASIN_HOPPING_RADII, None) == INVALID
    assert L.dzo_basin_hopping_set_record(h, -1) == INVALID
    assert L.dzo_basin_hopping_set_record(h, 2) == 0
    assert L.dzo_basin_hopping_hop(h, 3, 0) == INVALID                                # does not fit the record
    assert L.dzo_basin_hopping_hop(h, 2, 0) == 0 and L.dzo_basin_hopping_hop(h, 0, 1) == 0
    counts = np.zeros(batch, dtype=np.int64)
    assert L.dzo_basin_hopping_read(h, dzo.BASIN_HOPPING_HOP_COUNTS, counts.ctypes.data) == 0 and counts.tolist() == [2, 2, 2]
    assert L.dzo_basin_hopping_set_record(h, 0) == 0 and L.dzo_basin_hopping_hop(h, 3, 0) == 0
    assert L.dzo_basin_hopping_destroy(h) == 0 and L.dzo_basin_hopping_destroy(None) == 0
    with pytest.raises(dzo.DzoError) as err:
        dzo.BasinHopping(dzo.DeviceArray.zeros(3 * 1025), 1025, [1.0], [0.1], 3.0)
    assert err.value.code == UNSUPPORTED


def test_example_reaches_the_icosahedron(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_basin_hopping")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "best energy: -44.32680" in r.stdout
