"""The CPU twin of the batched lowest Hessian mode (tests/lowmode_twin.py) against things it does not depend on: its exact
fused multiply-adds against pairwise_twin's Fraction arithmetic, its vectorised product against hessian_twin.hvp_bits, its small
Jacobi iteration against LAPACK, and the iteration itself against the dense truth (``hessian_f64`` of the points as rounded to T,
P as a dense matrix, ``eigvalsh`` restricted to the range of P) on the cases the unit was designed on.  No device here.

The iteration is judged the way tests/test_gpu_lowmode.py judges the device: for a CONVERGED instance
rho_host = |P (H u - lambda u)| <= res_tol scale + delta, lambda - lambda_1 <= rho_host + delta and lambda_1 - lambda <= delta,
with delta = gamma eps_T ||H| |u||_2 and gamma = N + 32 (lowmode_twin.gamma counts it).  Here `scale` is the twin's own.
"""
import functools

import numpy as np
import pytest

import hessian_twin as ht
import lowmode_twin as lt
import pairwise_twin as tw

DTYPES = [np.float64, np.float32]
RES_TOL = {np.dtype(np.float64): 2.0 ** -30, np.dtype(np.float32): 2.0 ** -14}
CASES = ["icosahedron13", "octahedron38", "square4", "cluster3", "cluster4", "cluster13", "cluster38", "cluster64", "cluster65", "cluster257"]


@functools.lru_cache(maxsize=None)
def _point(name):
    if name == "icosahedron13":
        return np.concatenate(tw.icosahedron13())
    if name == "octahedron38":
        return np.concatenate(tw.octahedron38())
    if name == "square4":
        return ht.square4()
    n = int(name[len("cluster"):])
    return np.concatenate(tw.cluster(n, seed=n))


def test_exact_fused_multiply_adds_on_arrays():
    rng = np.random.default_rng(0)
    a, b, c = rng.standard_normal((3, 600)) * np.exp(rng.uniform(-5, 5, (3, 600)))
    c[::3] = -(a * b)[::3] * (1 + rng.standard_normal(200) * 1e-15)          # cancellation: the rounding of a * b decides
    got = lt.fma64(a, b, c)
    assert [i for i in range(600) if got[i] != tw.fma(a[i], b[i], c[i], np.float64)] == []
    a, b, c = (v.astype(np.float32) for v in (a, b, c))
    c[::3] = -(a * b)[::3]
    got = lt.fma32(a, b, c)
    assert got.dtype == np.float32
    assert [i for i in range(600) if got[i] != tw.fma(a[i], b[i], c[i], np.float32)] == []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [2, 3, 7])
def test_vectorised_product_has_the_bits_of_hvp_bits(n, dtype):
    P = np.concatenate(tw.cluster(n, seed=n)).astype(dtype).reshape(3, n)
    U = np.random.default_rng(n).standard_normal((3, n)).astype(dtype)
    F, S = lt.radials(P, dtype)
    assert np.array_equal(lt.hvp(P, F, S, U), ht.hvp_bits(*P, *U, dtype))


def test_sums_follow_the_stated_order():
    """N <= 64: the xor tree; above: a thread's particles first, then the tree, then the four waves."""
    rng = np.random.default_rng(1)
    t = rng.standard_normal(38)
    lanes = np.zeros(64)
    lanes[:38] = t
    for off in (32, 16, 8, 4, 2, 1):
        lanes = np.array([lanes[l] + lanes[l ^ off] for l in range(64)])
    assert lt.psum(t) == lanes[0]
    t = rng.standard_normal(300)
    own = [t[i] + (t[i + 256] if i + 256 < 300 else 0.0) for i in range(256)]
    waves = []
    for w in range(4):
        lanes = np.array(own[64 * w:64 * w + 64])
        for off in (32, 16, 8, 4, 2, 1):
            lanes = np.array([lanes[l] + lanes[l ^ off] for l in range(64)])
        waves.append(lanes[0])
    assert lt.psum(t) == ((waves[0] + waves[1]) + waves[2]) + waves[3]


@pytest.mark.parametrize("k", [1, 2, 3, 7, 32])
def test_jacobi_on_the_tridiagonal_against_lapack(k):
    rng = np.random.default_rng(k)
    alpha, beta = rng.standard_normal(k) * 10, np.abs(rng.standard_normal(max(k - 1, 0)))
    if k > 4:
        beta[2] = 0.0                                        # a closed Krylov space: two uncoupled blocks
    theta, y, sweeps = lt.jacobi_lowest(list(alpha), list(beta))
    T = np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)
    lam = np.linalg.eigvalsh(T)
    assert abs(theta - lam[0]) <= 64 * 2.0 ** -52 * np.abs(lam).max()
    assert abs(np.linalg.norm(y) - 1) <= 64 * 2.0 ** -52 and np.linalg.norm(T @ y - theta * y) <= 64 * 2.0 ** -52 * np.abs(lam).max()
    assert sweeps <= 12


def test_projector_removes_rigid_motions_and_is_idempotent():
    p = _point("cluster13")
    P = p.reshape(3, -1)
    proj = lt.Projector(P)
    assert proj.ok
    B = lt.rigid_basis(p)
    assert B.shape == (39, 6)
    v = np.random.default_rng(2).standard_normal((3, 13))
    pv = proj(v)
    assert np.abs(B.T @ pv.reshape(-1)).max() <= 1e-14 * np.linalg.norm(v)
    Pm = np.eye(39) - B @ B.T
    assert np.abs(Pm @ v.reshape(-1) - pv.reshape(-1)).max() <= 1e-14 * np.linalg.norm(v)


@pytest.mark.parametrize("project_rigid", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_twin_finds_the_lowest_eigenvalue_of_the_dense_truth(case, dtype, project_rigid):
    p = _point(case)
    tol = RES_TOL[np.dtype(dtype)]
    r = lt.lowest_mode(p, dtype, project_rigid=project_rigid, krylov=32, max_cycles=40, res_tol=tol, seed=len(p))
    ev, rho, delta, hnorm = lt.truth_figures(p, dtype, project_rigid, r.eigenvalue, r.vector)
    print(case, np.dtype(dtype).name, project_rigid, "cycles", r.cycles, "products", r.products, "lambda", float(r.eigenvalue), "lambda_1", ev[0],
          "gap", ev[1] - ev[0], "residual", r.residual, "rho_host", rho, "delta", delta, "scale", r.scale)
    assert lt.gap_is_usable(ev), (ev[0], ev[1])
    assert r.status == lt.CONVERGED
    n = len(p) // 3
    assert r.products <= (r.cycles - 1) * min(32, 3 * n - 6 if project_rigid else 3 * n) + 1
    assert r.scale <= hnorm * (1 + 1e-6)
    assert abs(np.linalg.norm(r.vector.astype(np.float64)) - 1) <= 4 * lt.EPS[np.dtype(dtype)]
    assert r.residual <= tol * r.scale
    assert rho <= tol * r.scale + delta
    assert float(r.eigenvalue) - ev[0] <= rho + delta
    assert ev[0] - float(r.eigenvalue) <= delta


def test_the_range_of_three_particles_clips_the_krylov_space():
    r = lt.lowest_mode(_point("cluster3"), np.float64, project_rigid=True, krylov=32, max_cycles=40, res_tol=2.0 ** -30, seed=3)
    assert r.status == lt.CONVERGED and r.products == (r.cycles - 1) * 3 + 1          # K = 3 N - 6 = 3


def test_square4_has_morse_index_two():
    ev, _, _ = lt.dense_truth(ht.square4(), np.float64, True)
    assert (ev < -1e-6).sum() == 2
    r = lt.lowest_mode(ht.square4(), np.float64, project_rigid=True, res_tol=2.0 ** -30, seed=4)
    assert r.status == lt.CONVERGED and float(r.eigenvalue) < -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_collinear_particles_fail_and_return(dtype):
    line = np.array([0.0, 1.1, 2.3, 0.0, 1.1, 2.3, 0.0, 1.1, 2.3])          # x = y = z: on a line that is no axis
    r = lt.lowest_mode(line, dtype, project_rigid=True, seed=5)
    assert r.status == lt.FAILED and r.cycles == 0 and r.products == 0 and np.isnan(r.eigenvalue) and np.isnan(r.residual)
    r = lt.lowest_mode(line, dtype, project_rigid=False, res_tol=RES_TOL[np.dtype(dtype)], seed=5)
    assert r.status == lt.CONVERGED                          # H itself needs no inertia tensor


def test_limits_one_cycle_an_eigenvector_start_and_two_vectors():
    p = _point("cluster13")
    start = np.random.default_rng(6).standard_normal(39)
    one = lt.lowest_mode(p, np.float64, max_cycles=1, res_tol=0.0, start=start)
    assert one.status == lt.UNFINISHED and one.cycles == 1 and one.products == 1
    good = lt.lowest_mode(p, np.float64, res_tol=2.0 ** -30, start=start)
    again = lt.lowest_mode(p, np.float64, res_tol=2.0 ** -24, start=good.vector)
    assert again.status == lt.CONVERGED and again.products == 1 and again.cycles == 1
    two = lt.lowest_mode(ht.square4(), np.float64, krylov=2, max_cycles=200, res_tol=2.0 ** -30, seed=7)
    assert two.status == lt.CONVERGED and two.products == 2 * (two.cycles - 1) + 1
