"""tests/sphere_twin.py pinned against things it does not depend on -- the literal restatement of the legacy functions, finite
differences, closed forms -- and, from the twin alone, that the inputs of tests/test_gpu_sphere.py meet that file's own
conditions: no undecided trial inside a decision window, the twin's arithmetic in T within half of every derived bound, its
directions within a quarter of the direction tolerance, and the tolerances of the minima.  No GPU here."""
import numpy as np
import pytest

import quench_checks as qc
import quench_twin as qt
import sphere_twin as st
from oracle import oracle as orc

LD = np.longdouble
dtypes = pytest.mark.parametrize("dtype", st.DTYPES)
cases = pytest.mark.parametrize("n,m", st.CASES)


def as_matrix(p):
    """[x | y | z] -> the (3, N) matrix of the legacy functions"""
    return np.ascontiguousarray(np.asarray(p).reshape(3, -1))


# ------------------------------------------------------------------------------ the legacy restatement against the radial form
@dtypes
@pytest.mark.parametrize("n", [2, 3, 7, 12, 33])
def test_radial_form_has_the_bits_of_the_legacy_functions(n, dtype):
    """Per term, 2 (-0.5 (inv_r / r2)) (r_j - r_i) is the reference's dist * inv_dist_cubed; in order, so is the raw gradient; the
    constrained gradient is constrain_riesz_gradient_sphere!'s."""
    t = np.dtype(dtype).type
    p = st.start(n, 5, dtype)
    P = as_matrix(p)
    terms = {}
    g_legacy = st.legacy_gradient(P, terms)
    e, f, dx, dy, dz = st.pair_terms(p, dtype)
    for k, d in enumerate((dx, dy, dz)):
        for j in range(n):
            for i in range(n):
                if i != j:
                    ours = f[j, i] * d[j, i]                     # row j of the device: (r_j - r_i), scaled by -1/2
                    assert qc.same(t(ours + ours), t(terms[(k, i, j)])), (k, i, j)
    _, g_raw = st.energy_gradient(p, dtype, constrained=False)
    assert qc.same(as_matrix(g_raw), g_legacy)
    _, g_con = st.energy_gradient(p, dtype)
    assert qc.same(as_matrix(g_con), st.legacy_constrain(g_legacy.copy(), P))
    # the energy: another order of summation (each pair once), so within the derived bound of each other
    E, _ = st.energy_gradient(p, dtype)
    exact, S = st.exact_energy(p)
    assert abs(LD(st.legacy_energy(P)) - exact) <= st.bound_energy(n, dtype, S) and abs(LD(E) - exact) <= st.bound_energy(n, dtype, S)


def test_project_and_tangent_are_the_stated_operations():
    p = np.array([3.0, 0.0, 1.0, 4.0, 2.0, 2.0])               # particles (3, 4) and (0, 2) in the plane z = ...: [x | y | z]
    q = st.project(p)
    assert np.allclose(q.reshape(3, 2)[:, 0], np.array([3.0, 1.0, 2.0]) / np.sqrt(14.0), rtol=1e-15)
    g = np.arange(6.0)
    gt = st.tangent(q, g).reshape(3, 2)
    assert np.all(np.abs((q.reshape(3, 2) * gt).sum(axis=0)) < 1e-15)
    with np.errstate(all="ignore"):
        assert np.all(np.isnan(st.project(np.zeros(3))))         # a particle on the origin: NaN, and the trial is rejected


# ------------------------------------------------------------------------------ finite differences along tangent directions
@pytest.mark.parametrize("n", [4, 12, 33])
def test_tangent_gradient_is_the_derivative_along_the_sphere(n):
    p = st.start(n, 2, np.float64)
    E, S, g, _ = st.exact(p)
    gt = st.exact_tangent(p, g)
    rng = np.random.default_rng(n)
    for _ in range(3):
        v = st.exact_tangent(p, rng.standard_normal((3, n)).astype(LD))      # a tangent direction
        eps = LD(1e-7)
        def moved(s):
            q = np.asarray(p, dtype=LD).reshape(3, n) + s * eps * v
            return (q / np.sqrt((q * q).sum(axis=0))[None, :]).reshape(-1)
        fd = (st.exact_energy(moved(1))[0] - st.exact_energy(moved(-1))[0]) / (2 * eps)
        slope = (gt * v).sum()
        assert abs(fd - slope) <= 1e-8 * np.abs(gt * v).sum() + 1e-9, (float(fd), float(slope))
        # the raw gradient has the same slope along a tangent direction
        assert abs((g * v).sum() - slope) <= 1e-15 * np.abs(g * v).sum()


# ------------------------------------------------------------------------------ closed forms
def test_closed_forms():
    want = {2: LD(1) / 2, 3: np.sqrt(LD(3)), 4: 3 * np.sqrt(LD(6)) / 2, 6: 12 / np.sqrt(LD(2)) + LD(3) / 2}
    for n in st.CLOSED_N:
        P, E = st.closed_form(n)
        assert np.all(np.abs((P * P).sum(axis=0) - 1) < 1e-18)
        exact, S, g, Srow = st.exact(P.reshape(-1))
        if n in want:
            assert E == want[n]
        assert abs(exact - E) <= 4 * np.finfo(LD).eps * E, (n, float(exact - E))
        assert np.max(np.abs(st.exact_tangent(P.reshape(-1), g))) <= 1e-17 * np.max(Srow), n     # a stationary point on the sphere
        for dtype in st.DTYPES:
            p = P.reshape(-1).astype(dtype)
            Et, gt = st.energy_gradient(p, dtype)
            e1, S1, g1, Srow1 = st.exact(p)
            assert abs(LD(Et) - e1) <= st.bound_energy(n, dtype, S1) / 2, (n, dtype)
            err = np.abs(as_matrix(gt).astype(LD) - st.exact_tangent(p, g1))
            assert np.all(err <= st.bound_gradient(n, dtype, Srow1)[None, :] / 2), (n, dtype)
    assert abs(float(st.E_ICOSAHEDRON) - 49.16525305763) < 1e-10


# ------------------------------------------------------------------------------ the bounds of one normalisation and one tangent
@dtypes
def test_normalisation_and_tangent_bounds_hold_over_a_million_vectors(dtype):
    rng = np.random.default_rng(11)
    v = (rng.standard_normal(3 * 10 ** 6) * np.exp(rng.uniform(-8, 8, 3 * 10 ** 6))).astype(dtype)
    q = st.project(v, dtype)
    Q = q.reshape(3, -1).astype(LD)
    worst = np.max(np.abs((Q * Q).sum(axis=0) - 1))
    print(np.dtype(dtype).name, "worst | |p|^2 - 1 | / u:", float(worst / st.U[np.dtype(dtype)]))
    assert worst <= st.bound_norm(dtype)                         # derived: 7 u and second order; the confirmation, not a margin
    again = st.project(q, dtype)
    assert not qc.same(again, q)                                 # not the identity in floating point
    g = rng.standard_normal(3 * 10 ** 6).astype(dtype)
    gt = st.tangent(q, g, dtype).reshape(3, -1).astype(LD)
    raw = np.sqrt((g.reshape(3, -1).astype(LD) ** 2).sum(axis=0))
    ratio = np.max(np.abs((Q * gt).sum(axis=0)) / st.bound_overlap(dtype, raw))
    print(np.dtype(dtype).name, "worst p . g / bound:", float(ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------ the GPU tests' inputs, from the twin alone
def test_case_table():
    assert st.CASES[:3] == [(2, 1), (3, 2), (4, 3)]
    for dtype in st.DTYPES:
        assert {qc.path(n, m, dtype) for n, m in st.CASES} == {qc.WAVE, qc.BLOCK_LDS, qc.BLOCK_SLAB}
    assert qc.path(97, 32, np.float64) == qc.BLOCK_LDS and qc.path(98, 32, np.float64) == qc.BLOCK_SLAB
    assert qc.path(195, 32, np.float32) == qc.BLOCK_LDS and qc.path(196, 32, np.float32) == qc.BLOCK_SLAB
    assert qc.path(64, 1, np.float64) == qc.WAVE and qc.path(65, 2, np.float32) == qc.BLOCK_LDS and qc.path(1024, 1, np.float64) == qc.BLOCK_SLAB
    for n, _ in st.CASES:
        for dtype in st.DTYPES:
            for b in range(st.batch_of(n)):
                Q = st.start(n, b, dtype).reshape(3, n).astype(LD)
                assert np.all(np.abs((Q * Q).sum(axis=0) - 1) <= st.bound_norm(dtype))


@dtypes
@cases
def test_windows_have_no_undecided_trial_and_bounds_leave_half(n, m, dtype):
    """What tests/test_gpu_sphere.py asks of the device, asked of the twin: at the start and after the steps before the second
    look the twin's energy and tangent gradient in T are within HALF the derived bounds; in the decision window every trial's
    longdouble energy is further from the old one than the margin."""
    window, look = st.window(n, dtype), st.steps_before_the_second_look(n)
    undecided = trials = 0
    worst_e = worst_g = 0.0
    for b in range(st.batch_of(n)):
        q = st.SphereQuench(st.start(n, b, dtype), st.STEP, m, dtype)
        for k in range(max(window, look) + 1):
            if k in (0, look):
                E, S, g, Srow = st.exact(q.x)
                worst_e = max(worst_e, float(abs(LD(q.f) - E) / st.bound_energy(n, dtype, S)))
                err = np.abs(as_matrix(q.g).astype(LD) - st.exact_tangent(q.x, g))
                worst_g = max(worst_g, float(np.max(err / st.bound_gradient(n, dtype, Srow)[None, :])))
            if k >= window:
                if k < look:
                    q.step()
                continue
            x_old = q.x.copy()
            assert not q.step().is_stuck, (n, m, b, k)
            old = st.exact_energy(x_old)
            for h, _ in q.trials:
                diff, bound = st.decision_margin(x_old, st.project(x_old + q.t(2.0 ** -h) * q.d, dtype), dtype, old)
                trials += 1
                undecided += int(abs(diff) <= bound)
    print(f"N={n} m={m} {np.dtype(dtype).name}: {undecided} of {trials} undecided; twin error / bound: energy {worst_e:.3f}, gradient {worst_g:.3f}")
    assert undecided == 0 and trials >= window * st.batch_of(n)
    assert worst_e <= 0.5 and worst_g <= 0.5


@dtypes
@cases
def test_direction_tolerance_covers_the_twin(n, m, dtype):
    """qt.direction in T against the fp64 oracle on the twin's own states over m + 8 steps: below a quarter of
    quench_checks.tol_direction(m, T) in every case, so that tolerance stands as it is (worst measured: fp32 2.11e-7 at
    (98, 32), fp64 4.8e-15 at (1024, 1))."""
    worst = 0.0
    for b in range(st.batch_of(n)):
        q = st.SphereQuench(st.start(n, b, dtype), st.STEP, m, dtype)
        for _ in range(m + 8):
            q.step()
            if q.is_stuck:
                break
            S, Y = np.array(q.S, dtype=np.float64), np.array(q.Y, dtype=np.float64)
            d_ref, _ = orc.lbfgs_direction(q.g.astype(np.float64), S, Y, np.array(q.rho))
            d = qt.direction(q.g, q.S, q.Y, q.rho, dtype).astype(np.float64)
            worst = max(worst, float(np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)))
    print(f"N={n} m={m} {np.dtype(dtype).name}: worst {worst:.3e}, tolerance {qc.tol_direction(m, dtype):.1e}")
    assert worst <= qc.tol_direction(m, dtype) / 4


@dtypes
def test_twin_reaches_the_minima(dtype):
    dt = np.dtype(dtype)
    for n in st.CLOSED_N:
        E = st.closed_form(n)[1]
        worst = 0.0
        for s in range(16):
            q = st.SphereQuench(st.jittered(n, s, dtype), st.STEP, 10, dtype)
            assert q.run(500) < 500
            worst = max(worst, float(abs(st.exact_energy(q.x)[0] - E)), float(abs(LD(q.f) - E)))
        print(f"closed form N={n} {dt.name}: twin's worst {worst:.3e}, recorded {st.TWIN_WORST_CLOSED[(n, dt)]:.3e}, floor {float(st.bound_energy(n, dtype, E)):.3e}")
        assert worst <= st.TWIN_WORST_CLOSED[(n, dt)]
    for n, lowest in ((12, st.E_ICOSAHEDRON), (32, st.E_LOWEST_32)):
        worst = 0.0
        for r in st.random_starts(n, 16, st.RANDOM_SEED, dtype):
            q = st.SphereQuench(r, st.STEP, 10, dtype)
            assert q.run(1000) < 1000
            worst = max(worst, float(abs(st.exact_energy(q.x)[0] - lowest)), float(abs(LD(q.f) - lowest)))
        print(f"random N={n} {dt.name}: twin's worst {worst:.3e}, recorded {st.TWIN_WORST_RANDOM[(n, dt)]:.3e}")
        assert worst <= st.TWIN_WORST_RANDOM[(n, dt)]
