"""The device's parallel-tempering Monte Carlo (scripts/MonteCarlo.jl; csrc/dzo_tempering.hip) against its CPU twin
(tests/tempering_twin.py), on the GPU.

A Metropolis trajectory cannot be compared value by value with another implementation: one decision that falls the other way
changes everything after it.  So the device RECORDS its draws and decisions, and the twin replays them:

* the draws are checked against the stated rule by themselves (bit for bit where the rule is integer or exactly rounded
  arithmetic, within a derived bound for the normals);
* given the recorded decisions the coordinates are reproducible bit for bit, so the twin knows the exact energy difference of
  every step, and with the derived bound b = (N + 32) u (S_old + S_new) which decisions the device MUST have taken; only
  steps whose uniform lies inside the error bars of the threshold are undecided, and their share is capped (5 % in fp32,
  none in fp64; tests/test_tempering_twin.py shows that the inputs alone meet the cap).

Bound of the normals (test_draws_follow_the_stated_rule).  Device: n = fl(sqrt(-2 log u1) * cospi(2 u2)); u1, 2 u2 are exact.
ROCm documents log, sqrt, sinpi and cospi of double at 1, 1, 2 and 2 ulp (HIP math API, "double precision mathematical functions").
log contributes 1 ulp, halved by the square root (1/2), the root adds 1, cospi / sinpi 2, the product 1/2: 4 ulp
<= 4 * 2^-52 |n| = 8 u |n|.  numpy on the host: log 1 ulp (halved), sqrt 1/2, product 1/2, cos 1 ulp: at most 2.5 ulp <= 5 u |n|;
but its ARGUMENT 2 pi u2 is a rounded product of a rounded constant: an absolute error of up to 2 * 2^-53 * 2 pi = 4 pi u, which
moves cos / sin by as much, times r = sqrt(-2 log u1).  One rounding to T: u_T |n|.  Together
|n_dev - n_numpy| <= (13 u + [T = fp32] u_T) |n| + 4 pi u r.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pairwise_twin as pw
import tempering_twin as tt
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
LD = np.longdouble
U = tt.U
DTYPES = [np.float64, np.float32]
NS = tt.TRAJECTORY_NS
U64 = LD(2.0) ** -53


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.int8}[a.dtype.itemsize])


def _make(reps, beta, radii, R, seed, record=0):
    """reps: (replicas, 3, N) of the element type"""
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(reps).reshape(-1))
    pt = dzo.ParallelTempering(dev, reps.shape[2], beta, radii, R, seed)
    if record:
        pt.set_record(record)
    return dev, pt


def _record(pt):
    return (pt.read(dzo.TEMPERING_REC_INDEX), pt.read(dzo.TEMPERING_REC_NORMALS), pt.read(dzo.TEMPERING_REC_UNIFORM),
            pt.read(dzo.TEMPERING_REC_CODE))


def _trace(dev_energies, steps, replicas, ld=None):
    ld = steps if ld is None else ld
    return dev_energies.to_host().reshape(replicas, ld)[:, :steps]


# ------------------------------------------------------------------------------ 1. draws
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_draws_follow_the_stated_rule(n, dtype):
    reps, beta, radii, R = tt.trajectory_inputs(n, dtype)
    steps, seed = 200, 977 + n
    dev, pt = _make(reps, beta, radii, R, seed, record=steps)
    pt.temper(steps)
    idx, nrm, uni, code = _record(pt)
    worst = 0.0
    for k in range(reps.shape[0]):
        raw = orc.pcg_raw(6 * steps, seed + k).reshape(steps, 6)
        j, normals, u, r = tt.step_draws(raw, n, np.float64)
        assert np.array_equal(idx[k], j), (n, k)
        assert np.array_equal(_bits(uni[k]), _bits(u.astype(dtype))), (n, k)
        ut = U[np.dtype(dtype)] if np.dtype(dtype) == np.float32 else LD(0)
        bound = (13 * U64 + ut) * np.abs(normals).astype(LD) + 4 * LD(math.pi) * U64 * r.astype(LD)
        err = np.abs(nrm[k].astype(LD) - normals.astype(LD))
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (n, k, float((err / bound).max()))
    # the state the handle keeps is the stream after 6 * steps draws
    for k in range(reps.shape[0]):
        assert int(pt.rng_states[k]) == tt.pcg_raw(tt.pcg_state(seed + k), 6 * steps)[1]
    print(f"draws N={n} {np.dtype(dtype).name}: worst normal error / bound = {worst:.4f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_normals_are_normal(dtype):
    """Mean, variance and the Kolmogorov-Smirnov statistic of m = 115 200 recorded normals inside 5 sigma of their sampling
    distributions: |mean| <= 5 / sqrt(m); |var - 1| <= 5 sqrt(2 / (m - 1)); D <= sqrt(ln(2 / p) / (2 m)) with p = 5.7e-7, the
    two-sided 5-sigma tail (the asymptotic P(D > x) <= 2 exp(-2 m x^2))."""
    from scipy import stats
    n, replicas, steps = 38, 64, 600
    reps = np.repeat(np.stack(pw.octahedron38())[None], replicas, axis=0).astype(dtype)
    dev, pt = _make(reps, np.full(replicas, 5.0), np.full(replicas, 0.01), 3.0, 31337, record=steps)
    pt.temper(steps)
    z = pt.read(dzo.TEMPERING_REC_NORMALS).astype(np.float64).ravel()
    m = z.size
    assert m == 115200
    assert abs(z.mean()) <= 5.0 / math.sqrt(m), z.mean()
    assert abs(z.var(ddof=1) - 1.0) <= 5.0 * math.sqrt(2.0 / (m - 1)), z.var(ddof=1)
    D = stats.kstest(z, "norm").statistic
    assert D <= math.sqrt(math.log(2.0 / 5.7e-7) / (2.0 * m)), D
    u = pt.read(dzo.TEMPERING_REC_UNIFORM).astype(np.float64).ravel()
    assert abs(u.mean() - 0.5) <= 5.0 * math.sqrt(1.0 / 12.0 / u.size)
    print(f"normals {np.dtype(dtype).name}: mean {z.mean():.2e}, var {z.var(ddof=1):.5f}, KS D {D:.5f}")


# ------------------------------------------------------------------------------ 2. trajectory
def _check_trajectory(n, dtype, reps, beta, radii, R, seed, steps, cap):
    dev, pt = _make(reps, beta, radii, R, seed, record=steps)
    energies = dzo.DeviceArray.zeros(steps * reps.shape[0], dtype)
    pt.temper(steps, energies)
    idx, nrm, uni, code = _record(pt)
    trace = _trace(energies, steps, reps.shape[0])
    final, new_radii, acc, rej = pt.coordinates, pt.perturbation_radii, pt.num_accept, pt.num_reject
    undecided = 0
    for k in range(reps.shape[0]):
        tr = tt.replay(reps[k], idx[k], nrm[k], uni[k], code[k], np.dtype(dtype).type(radii[k]), np.dtype(dtype).type(beta[k]), R, dtype)
        assert np.array_equal(code[k] != tt.CODE_OUTSIDE, tr.inside), (n, k, "sphere flags")
        ins = tr.inside
        bad_acc = ins & (tr.klass == tt.MUST_ACCEPT) & (code[k] != tt.CODE_ACCEPTED)
        bad_rej = ins & (tr.klass == tt.MUST_REJECT) & (code[k] != tt.CODE_REJECTED)
        assert not bad_acc.any() and not bad_rej.any(), (n, k, np.flatnonzero(bad_acc)[:5], np.flatnonzero(bad_rej)[:5])
        assert np.array_equal(_bits(final[k]), _bits(tr.final)), (n, k, "final coordinates")
        err = np.abs(trace[k].astype(LD) - tr.energy)
        assert np.all(err <= tr.energy_bound), (n, k, float((err / tr.energy_bound).max()))
        assert _bits(new_radii[k:k + 1])[0] == _bits(np.array([tr.radius], dtype=dtype))[0], (n, k, new_radii[k], tr.radius)
        assert (acc[k], rej[k]) == (tr.num_accept, tr.num_reject)
        undecided += int(np.sum(ins & (tr.klass == tt.UNDECIDED)))
    share = undecided / (steps * reps.shape[0])
    print(f"trajectory N={n} {np.dtype(dtype).name}: accepted {acc.tolist()}, undecided share {share:.4f}")
    assert share <= cap, (n, share)
    return pt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_trajectory_replayed_by_the_twin(n, dtype):
    reps, beta, radii, R = tt.trajectory_inputs(n, dtype)
    _check_trajectory(n, dtype, reps, beta, radii, R, tt.TRAJECTORY_SEED + n, tt.TRAJECTORY_STEPS, tt.UNDECIDED_CAP[np.dtype(dtype)])


# ------------------------------------------------------------------------------ 3. exact limits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_infinite_temperature_accepts_every_inside_proposal(n, dtype):
    reps, _, radii, R = tt.trajectory_inputs(n, dtype)
    steps = 300
    dev, pt = _make(reps, np.zeros(reps.shape[0]), radii * 5, R, 7, record=steps)
    pt.temper(steps)
    code = pt.read(dzo.TEMPERING_REC_CODE)
    assert set(np.unique(code)) <= {tt.CODE_ACCEPTED, tt.CODE_OUTSIDE}
    assert (code == tt.CODE_ACCEPTED).sum() > 0
    final = pt.coordinates.astype(dtype)
    r2 = final[:, 0] * final[:, 0] + final[:, 1] * final[:, 1] + final[:, 2] * final[:, 2]
    assert np.all(r2 < np.dtype(dtype).type(R) * np.dtype(dtype).type(R))


@pytest.mark.parametrize("n", NS)
def test_zero_temperature_never_goes_up(n):
    reps, _, radii, R = tt.trajectory_inputs(n, np.float64)
    steps = 400
    dev, pt = _make(reps, np.full(reps.shape[0], 1e300), radii, R, 11, record=steps)
    energies = dzo.DeviceArray.zeros(steps * reps.shape[0])
    pt.temper(steps, energies)
    trace = _trace(energies, steps, reps.shape[0])
    assert np.all(np.diff(trace, axis=1) <= 0)
    assert (pt.read(dzo.TEMPERING_REC_CODE) == tt.CODE_ACCEPTED).sum() > 0
    assert np.all(trace[:, -1] < trace[:, 0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_constraining_radius_zero_freezes_everything(n, dtype):
    reps, beta, radii, _ = tt.trajectory_inputs(n, dtype)
    steps = 100
    dev, pt = _make(reps, beta, radii, 0.0, 3, record=steps)
    energies = dzo.DeviceArray.zeros(steps * reps.shape[0], dtype)
    pt.temper(steps, energies)
    trace = _trace(energies, steps, reps.shape[0])
    assert np.array_equal(_bits(pt.coordinates), _bits(reps))
    assert np.all(pt.read(dzo.TEMPERING_REC_CODE) == tt.CODE_OUTSIDE)
    assert np.all(trace == trace[:, :1])
    for k in range(reps.shape[0]):
        e, s = pw.energy(*reps[k])
        assert abs(LD(trace[k, 0]) - e) <= tt.delta_bound(n, s, dtype)
    want = np.array([np.dtype(dtype).type(r) / tt.fac(dtype) for r in radii], dtype=dtype)
    assert np.array_equal(_bits(pt.perturbation_radii), _bits(want))
    assert np.all(pt.num_accept == 0) and np.all(pt.num_reject == steps)


# ------------------------------------------------------------------------------ 4. drift
@pytest.mark.parametrize("dtype", DTYPES)
def test_trace_does_not_drift_from_the_energy(dtype):
    """10^4 steps from octahedron38 at T = 0.05: the last trace value (10^4 additions of a delta) against the pairwise energy
    of the final replica, within the bound accumulated along the replayed path plus the bound of that energy itself."""
    n, steps = 38, 10000
    base = np.stack(pw.octahedron38())
    reps = base[None].astype(dtype)
    R = float(np.sqrt((base ** 2).sum(axis=0)).max() + 0.6)
    dev, pt = _make(reps, [20.0], [0.03], R, 2024, record=steps)
    energies = dzo.DeviceArray.zeros(steps, dtype)
    pt.temper(steps, energies)
    idx, nrm, uni, code = _record(pt)
    trace = _trace(energies, steps, 1)[0]
    tr = tt.replay(reps[0], idx[0], nrm[0], uni[0], code[0], np.dtype(dtype).type(0.03), np.dtype(dtype).type(20.0), R, dtype)
    assert np.array_equal(_bits(pt.coordinates[0]), _bits(tr.final))
    x, y, z = (dev.view(c * n, n) for c in range(3))
    e_final = dzo.pairwise_radial_energy(x, y, z)
    _, s_final = pw.energy(*tr.final)
    bound = tr.energy_bound[-1] + tt.delta_bound(n, s_final, dtype)
    drift = abs(LD(trace[-1]) - LD(e_final))
    print(f"drift {np.dtype(dtype).name}: {tr.num_accept} accepted of {steps}, |trace - E| = {float(drift):.3e}, bound {float(bound):.3e}")
    assert tr.num_accept > 100
    assert drift <= bound


# ------------------------------------------------------------------------------ 5. swap
def _swap_case(n, replicas, dtype, beta, seed):
    base = np.stack(pw.cluster(n, seed=n))
    reps = np.stack([np.stack(pw.jittered(tuple(base), 50 + k, 0.03)) for k in range(replicas)]).astype(dtype)
    R = float(np.sqrt((base ** 2).sum(axis=0)).max() + 1.0)
    return reps, _make(reps, beta, np.full(replicas, 0.01), R, seed)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("replicas,odd", [(6, 0), (6, 1), (7, 0), (7, 1), (1, 0), (1, 1), (2, 1)])
def test_swap_decisions_and_blocks(n, replicas, odd, dtype):
    beta = 1.0 / np.linspace(0.05, 0.35, replicas)
    seed = 600 + n
    reps, (dev, pt) = _swap_case(n, replicas, dtype, beta, seed)
    pt.swap(odd)
    after, dec, logp = pt.coordinates, pt.read(dzo.TEMPERING_REC_SWAP), pt.read(dzo.TEMPERING_REC_SWAP_LOGP)
    states = pt.rng_states
    leaders = list(range(1 if odd else 0, replicas - 1, 2))
    touched = set()
    for a in leaders:
        b = a + 1
        touched |= {a, b}
        raw, st = tt.pcg_raw(tt.pcg_state(seed + a), 1)
        assert int(states[a]) == st                                   # one draw, always consumed
        klass, lp, err = tt.swap_classify(reps[a], reps[b], beta[a], beta[b], tt.swap_uniform(raw[0], dtype), dtype)
        assert dec[a] in (0, 1)
        assert abs(LD(logp[a]) - lp) <= err, (a, logp[a], float(lp), float(err))
        if klass != tt.UNDECIDED:
            assert dec[a] == klass, (a, dec[a], klass, float(lp))
        first, second = (reps[b], reps[a]) if dec[a] else (reps[a], reps[b])
        assert np.array_equal(_bits(after[a]), _bits(first)) and np.array_equal(_bits(after[b]), _bits(second))
    for k in range(replicas):
        if k not in touched:
            assert np.array_equal(_bits(after[k]), _bits(reps[k]))
            assert int(states[k]) == tt.pcg_state(seed + k)
        if k not in leaders:
            assert dec[k] == -1 and logp[k] == 0
    assert np.array_equal(_bits(pt.inverse_temperatures), _bits(beta.astype(dtype)))     # temperatures stay with the slot


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_temperatures_always_swap(dtype):
    replicas = 8
    reps, (dev, pt) = _swap_case(38, replicas, dtype, np.full(replicas, 4.0), 9)
    pt.swap(0)
    after = pt.coordinates
    assert np.all(pt.read(dzo.TEMPERING_REC_SWAP)[0::2] == 1)
    for a in range(0, replicas, 2):
        assert np.array_equal(_bits(after[a]), _bits(reps[a + 1])) and np.array_equal(_bits(after[a + 1]), _bits(reps[a]))


# ------------------------------------------------------------------------------ 6. reproducibility
def _everything(pt, energies, steps, replicas):
    return [_bits(pt.coordinates), _bits(pt.perturbation_radii), _bits(pt.rng_states), pt.num_accept, pt.num_reject,
            _bits(_trace(energies, steps, replicas))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_same_seed_same_bits(n, dtype):
    reps, beta, radii, R = tt.trajectory_inputs(n, dtype)
    steps, out = 300, []
    for _ in range(2):
        dev, pt = _make(reps, beta, radii, R, 5, record=steps)
        energies = dzo.DeviceArray.zeros(steps * reps.shape[0], dtype)
        pt.temper(steps, energies)
        pt.swap(0)
        out.append(_everything(pt, energies, steps, reps.shape[0]) + [pt.read(dzo.TEMPERING_REC_CODE), pt.read(dzo.TEMPERING_REC_SWAP)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_one_call_equals_two_halves(n, dtype):
    """500 steps in one call against 2 x 250 with the random states read and set back (a checkpoint) and the radii set back to
    their start values in between (the adaptation runs at the end of every call; its inputs, the counts, must add up).  The
    energy is recomputed at the start of the second call, so the traces agree within twice the replayed path's bound."""
    reps, beta, radii, R = tt.trajectory_inputs(n, dtype)
    replicas = reps.shape[0]
    dev1, one = _make(reps, beta, radii, R, 77, record=500)
    e1 = dzo.DeviceArray.zeros(500 * replicas, dtype)
    one.temper(500, e1)
    codes1, trace1 = one.read(dzo.TEMPERING_REC_CODE), _trace(e1, 500, replicas)
    dev2, two = _make(reps, beta, radii, R, 77, record=250)
    e2 = dzo.DeviceArray.zeros(500 * replicas, dtype)
    two.temper(250, e2, ld=500)
    acc_a, rej_a, codes_a = two.num_accept, two.num_reject, two.read(dzo.TEMPERING_REC_CODE)
    states = two.rng_states
    two.rng_states = states
    two.perturbation_radii = np.asarray(radii, dtype=dtype)
    two.temper(250, e2.view(250, 500 * replicas - 250), ld=500)
    codes_b = two.read(dzo.TEMPERING_REC_CODE)
    trace2 = _trace(e2, 500, replicas, ld=500)
    assert np.array_equal(_bits(one.coordinates), _bits(two.coordinates))
    assert np.array_equal(codes1, np.concatenate([codes_a, codes_b], axis=1))
    assert np.array_equal(one.num_accept, acc_a + two.num_accept) and np.array_equal(one.num_reject, rej_a + two.num_reject)
    assert np.array_equal(_bits(one.rng_states), _bits(two.rng_states))
    assert np.array_equal(_bits(trace1[:, :250]), _bits(trace2[:, :250]))
    idx, nrm, uni, _ = _record(one)
    for k in range(replicas):
        tr = tt.replay(reps[k], idx[k], nrm[k], uni[k], codes1[k], np.dtype(dtype).type(radii[k]), np.dtype(dtype).type(beta[k]), R, dtype)
        assert np.all(np.abs(trace1[k].astype(LD) - trace2[k].astype(LD)) <= 2 * tr.energy_bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_run_equals_the_four_calls(n, dtype):
    replicas, steps, batches = 6, 60, 2
    beta = 1.0 / np.linspace(0.05, 0.35, replicas)
    rows = 2 * steps * batches
    reps, (dev1, a) = _swap_case(n, replicas, dtype, beta, 15)
    _, (dev2, b) = _swap_case(n, replicas, dtype, beta, 15)
    ea, eb = dzo.DeviceArray.zeros(rows * replicas, dtype), dzo.DeviceArray.zeros(rows * replicas, dtype)
    a.run(steps, batches, ea)
    for i in range(batches):
        b.temper(steps, eb.view(steps * (2 * i), rows * replicas - steps * (2 * i)), ld=rows)
        b.swap(False)
        b.temper(steps, eb.view(steps * (2 * i + 1), rows * replicas - steps * (2 * i + 1)), ld=rows)
        b.swap(True)
    for x, y in zip(_everything(a, ea, rows, replicas), _everything(b, eb, rows, replicas)):
        assert np.array_equal(x, y)
    assert not np.array_equal(_bits(a.coordinates), _bits(reps))


# ------------------------------------------------------------------------------ 7. analyze
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,ld", [(1000, 1000), (777, 1000), (1, 5)])
def test_analyze(rows, ld, dtype):
    """Moments within n u mean|term| of the longdouble twin (the device forms terms and sums in fp64 and rounds once to T);
    cv and cv_prime are :173-176 in T on the device's own moments: numpy performs the same single-rounded operations, a few
    u of the largest intermediate are allowed for a differently rounded division."""
    replicas = 5
    rng = np.random.default_rng(rows)
    host = (-170.0 + 3.0 * rng.standard_normal((replicas, ld))).astype(dtype)
    beta = 1.0 / np.linspace(0.05, 0.35, replicas)
    reps, (dev, pt) = _swap_case(13, replicas, dtype, beta, 1)
    e = dzo.DeviceArray.from_host(host.reshape(-1))
    off = 3 if ld - rows >= 3 else 0
    cv, cvp, mom = pt.analyze(e.view(off, host.size - off), rows, ld=ld)
    u = U[np.dtype(dtype)]
    for k in range(replicas):
        V1, V2, V3, A1, A2, A3 = tt.moments(host[k, off:off + rows])
        for got, want, scale in zip(mom[k], (V1, V2, V3), (A1, A2, A3)):
            assert abs(LD(got) - want) <= rows * u * scale, (k, got, float(want))
            assert np.dtype(dtype).type(got) == got
        want_cv, want_cvp = tt.heat_capacity(mom[k][0], mom[k][1], mom[k][2], np.dtype(dtype).type(beta[k]), dtype)
        b2 = float(np.dtype(dtype).type(beta[k])) ** 2
        assert abs(cv[k] - float(want_cv)) <= 4 * float(u) * b2 * abs(mom[k][1])
        assert abs(cvp[k] - float(want_cvp)) <= 4 * float(u) * b2 * b2 * (abs(mom[k][2]) + 2 * abs(mom[k][0]) * abs(mom[k][1]))


# ------------------------------------------------------------------------------ 8. errors
def test_error_codes():
    n, replicas = 13, 4
    reps, beta, radii, R = tt.trajectory_inputs(n, np.float64)
    reps = np.concatenate([reps, reps[:1]])
    beta = np.linspace(3.0, 20.0, replicas); radii = np.full(replicas, 0.02)
    dev = dzo.DeviceArray.from_host(reps.reshape(-1))
    L = dzo.lib()
    bp, rp = beta.ctypes.data_as(C.POINTER(C.c_double)), radii.ctypes.data_as(C.POINTER(C.c_double))
    h = C.c_void_p()
    create = lambda radial=0, n_=n, r_=replicas, dt=dzo.F64, ptr=dev.ptr, b=bp, r=rp, out=C.byref(h): \
        L.dzo_tempering_create(radial, n_, r_, dt, ptr, b, r, R, 1, out)
    assert create(radial=7) == 1
    assert create(n_=0) == 1 and create(r_=0) == 1 and create(dt=9) == 1
    assert create(ptr=None) == 1 and create(b=None) == 1 and create(r=None) == 1 and create(out=None) == 1
    assert create(n_=dzo.TEMPERING_MAX_PARTICLES + 1) == 5                          # DZO_ERR_UNSUPPORTED
    host = np.zeros(3 * n * replicas)
    assert create(ptr=host.ctypes.data) == 3                                         # DZO_ERR_ASSERT: not device memory
    assert b"replicas" in L.dzo_last_error()
    assert create() == 0 and h.value
    e = dzo.DeviceArray.zeros(50 * replicas)
    assert L.dzo_tempering_temper(None, 10, e.ptr, 50) == 1
    assert L.dzo_tempering_temper(h, -1, e.ptr, 50) == 1
    assert L.dzo_tempering_temper(h, 50, e.ptr, 49) == 1                             # ld < rows
    hostE = np.zeros(50 * replicas)
    assert L.dzo_tempering_temper(h, 50, hostE.ctypes.data, 50) == 3
    assert L.dzo_tempering_run(h, 25, 2, e.ptr, 50) == 1                             # 100 rows do not fit ld = 50
    assert L.dzo_tempering_run(h, 10, -1, e.ptr, 50) == 1
    cv = (C.c_double * replicas)()
    assert L.dzo_tempering_analyze(h, 50, None, 50, cv, cv, None) == 1
    assert L.dzo_tempering_analyze(h, 0, e.ptr, 50, cv, cv, None) == 1
    assert L.dzo_tempering_analyze(h, 50, hostE.ctypes.data, 50, cv, cv, None) == 3
    assert L.dzo_tempering_read(h, 99, hostE.ctypes.data) == 1
    assert L.dzo_tempering_read(h, dzo.TEMPERING_REC_CODE, hostE.ctypes.data) == 6   # DZO_ERR_STATE: nothing recorded
    assert L.dzo_tempering_set(h, dzo.TEMPERING_INV_TEMPS, hostE.ctypes.data) == 1
    assert L.dzo_tempering_set_record(h, 20) == 0
    assert L.dzo_tempering_temper(h, 21, e.ptr, 50) == 1                             # longer than the record
    assert L.dzo_tempering_temper(h, 20, e.ptr, 50) == 0
    assert L.dzo_tempering_temper(h, 20, None, 0) == 0                               # no trace
    assert L.dzo_tempering_set_record(h, 0) == 0
    assert L.dzo_tempering_swap(h, 1) == 0
    p = C.c_void_p()
    assert L.dzo_tempering_get_ptr(h, dzo.TEMPERING_REPLICAS, C.byref(p)) == 0 and p.value == dev.ptr
    assert L.dzo_tempering_destroy(h) == 0
    assert L.dzo_tempering_destroy(None) == 0


# ------------------------------------------------------------------------------ 9. the C example
def test_lj_tempering_example_runs(tmp_path):
    dzo.build()
    exe = str(tmp_path / "lj_tempering")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lj_tempering.c"),
                    "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "500", "20", "0.05"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Monte Carlo steps per second" in r.stdout and "OK" in r.stdout
    mean = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) == 6 and f[0] == "replica":
            mean[int(f[1])] = float(f[3])                    # replica k  T  <E>  cv  cv_prime
    assert len(mean) == 256
    cold = np.mean([mean[k] for k in range(8)])
    hot = np.mean([mean[k] for k in range(248, 256)])
    assert cold < hot, (cold, hot)
