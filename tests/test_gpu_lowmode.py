"""The batched lowest Hessian mode on the device (csrc/dzo_lowmode.hip) against the dense truth and against its CPU twin
(tests/lowmode_twin.py).

1. Truth.  N in {3, 4 (the planar square), 13, 38, 63, 64, 65, 256, 257}, four distinct instances each (the configuration and
   three uniformly compressed copies of it: compression keeps an exactly degenerate lowest eigenvalue degenerate), both element
   types, with and without the rigid-body projector.  The gaps are re-checked on the CPU: lambda_2 - lambda_1 >= 0.55 or a
   degenerate lambda_1.  Every instance must converge.  For each, in fp64 on the host from the dense Hessian of the points as
   rounded to T:  rho_host = |P (H u - lambda u)| <= residual + delta  and  residual <= res_tol |H|_2,  which together are the
   header's  rho_host <= res_tol scale + delta  (`scale` is a maximum of Rayleigh quotients and Ritz values of unit vectors, so
   at most |H|_2; the device does not report it);  lambda - lambda_1 <= rho_host + delta;  lambda_1 - lambda <= delta.
   delta = gamma eps_T ||H| |u||_2 with gamma = N + 32: the row sum of a product adds N terms sequentially, and one term carries at
   most 32 roundings of its own (lowmode_twin.gamma lists them; the count of tests/test_gpu_pairwise.py).
2. Replay.  N = 5, 38 and 65 from given start vectors: status, cycles, products, residual, eigenvalue and vector == the twin's.
3. Invariance.  An instance alone, first and last in a batch of five; a supplied start equal to the drawn one.
4. Limits: one cycle, an eigenvector as start, two Lanczos vectors, N = 1024, collinear particles, the argument errors; canaries.
5. The plain-C example.
"""
import functools
import subprocess

import numpy as np
import pytest

import hessian_twin as ht
import lowmode_twin as lt
import pairwise_twin as tw
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
RES_TOL = {np.dtype(np.float64): 2.0 ** -30, np.dtype(np.float32): 2.0 ** -14}
SCALES = (1.0, 0.995, 0.99, 0.985)
NS_TRUTH = [3, 4, 13, 38, 63, 64, 65, 256, 257]
CANARY = 12345.0
GUARD = 64


@functools.lru_cache(maxsize=None)
def _base(n):
    p = ht.square4() if n == 4 else np.concatenate(tw.cluster(n, seed=n))
    p = np.array(p, dtype=np.float64)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _instances(n, dtype, count=len(SCALES)):
    """`count` distinct instances (count, 3n): fp64 arrays holding values of `dtype`, so that the host sees what the device sees."""
    scales = SCALES[:count] if count <= len(SCALES) else SCALES + tuple(0.98 - 0.005 * k for k in range(count - len(SCALES)))
    p = np.stack([_base(n) * s for s in scales]).astype(dtype).astype(np.float64)
    p.setflags(write=False)
    return p


def _run(points, n, dtype, start=None, **kw):
    """dzo.lowest_modes of host points (batch, 3n); the vectors come back as a host array (batch, 3n)."""
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(points).ravel(), dtype=dtype)
    sdev = None if start is None else dzo.DeviceArray.from_host(np.ascontiguousarray(start).ravel(), dtype=dtype)
    r = dzo.lowest_modes(dev, n, start=sdev, **kw)
    r.vectors = r.vectors.to_host().reshape(len(points), 3 * n)
    assert r.eigenvalues.dtype == np.dtype(dtype) and r.vectors.dtype == np.dtype(dtype)
    return r


# ------------------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("project_rigid", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS_TRUTH)
def test_lowest_eigenpair_against_the_dense_truth(n, dtype, project_rigid):
    pts = _instances(n, dtype)
    tol = RES_TOL[np.dtype(dtype)]
    r = _run(pts, n, dtype, project_rigid=project_rigid, krylov=32, max_cycles=80, res_tol=tol, seed=100 + n)
    for b in range(len(pts)):
        ev, rho, delta, hnorm = lt.truth_figures(pts[b], dtype, project_rigid, r.eigenvalues[b], r.vectors[b])
        print(n, np.dtype(dtype).name, project_rigid, b, "status", r.status[b], "cycles", r.cycles[b], "products", r.products[b], "lambda",
              float(r.eigenvalues[b]), "lambda_1", ev[0], "gap", ev[1] - ev[0], "residual", r.residuals[b], "rho_host", rho, "delta", delta,
              "|H|", hnorm)
        assert lt.gap_is_usable(ev), (b, ev[0], ev[1])
        assert r.status[b] == dzo.LOWMODE_CONVERGED, b
        assert abs(np.linalg.norm(r.vectors[b].astype(np.float64)) - 1) <= 4 * lt.EPS[np.dtype(dtype)]
        assert 0 <= r.residuals[b] <= tol * hnorm
        assert rho <= r.residuals[b] + delta
        assert float(r.eigenvalues[b]) - ev[0] <= rho + delta
        assert ev[0] - float(r.eigenvalues[b]) <= delta
        K = min(32, 3 * n - 6 if project_rigid else 3 * n)
        assert 1 <= r.cycles[b] <= 80 and 1 <= r.products[b] <= (r.cycles[b] - 1) * K + 1


# ------------------------------------------------------------------------------ 2. replay
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, project_rigid, max_cycles", [(5, True, 40), (5, False, 40), (38, True, 40), (65, True, 3)])
def test_replay_of_the_twin_bit_for_bit(n, project_rigid, max_cycles, dtype):
    """Two instances from given start vectors.  N = 65 stops after three cycles (UNFINISHED): 65 products of the block shape."""
    pts = _instances(n, dtype, 2)
    start = np.random.default_rng(n).standard_normal((2, 3 * n)).astype(dtype)
    tol = RES_TOL[np.dtype(dtype)]
    r = _run(pts, n, dtype, start=start, project_rigid=project_rigid, krylov=32, max_cycles=max_cycles, res_tol=tol)
    for b in range(2):
        t = lt.lowest_mode(pts[b], dtype, project_rigid=project_rigid, krylov=32, max_cycles=max_cycles, res_tol=tol, start=start[b])
        print(n, np.dtype(dtype).name, b, "device", r.status[b], r.cycles[b], r.products[b], repr(r.eigenvalues[b]), r.residuals[b], "twin", t.status,
              t.cycles, t.products, repr(t.eigenvalue), t.residual)
        assert (r.status[b], r.cycles[b], r.products[b]) == (t.status, t.cycles, t.products)
        assert t.status == (dzo.LOWMODE_UNFINISHED if n == 65 else dzo.LOWMODE_CONVERGED)
        assert r.eigenvalues[b] == t.eigenvalue and r.residuals[b] == t.residual
        assert np.array_equal(r.vectors[b], t.vector)


# ------------------------------------------------------------------------------ 3. invariance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [38, 65])
def test_an_instance_computes_the_same_bits_anywhere_in_a_batch(n, dtype):
    five = _instances(n, dtype, 5)
    start = np.random.default_rng(7 * n).standard_normal((5, 3 * n)).astype(dtype)
    kw = dict(project_rigid=True, krylov=32, max_cycles=4, res_tol=RES_TOL[np.dtype(dtype)])
    whole = _run(five, n, dtype, start=start, **kw)
    drawn = _run(five, n, dtype, seed=50, **kw)
    for b in (0, 4):
        alone = _run(five[b:b + 1], n, dtype, start=start[b:b + 1], **kw)
        alone_drawn = _run(five[b:b + 1], n, dtype, seed=50 + b, **kw)          # the stream of instance b is base_seed + b
        for one, many in ((alone, whole), (alone_drawn, drawn)):
            assert np.array_equal(one.vectors[0], many.vectors[b]) and one.eigenvalues[0] == many.eigenvalues[b]
            assert one.residuals[0] == many.residuals[b]
            assert (one.status[0], one.cycles[0], one.products[0]) == (many.status[b], many.cycles[b], many.products[b])
    assert not np.array_equal(drawn.vectors[0], whole.vectors[0])


@pytest.mark.parametrize("n", [38, 65])
def test_a_supplied_start_equal_to_the_drawn_one_gives_the_same_bits(n):
    """fp32: the normals are fp64 Box-Muller values rounded to T, and numpy's and the device's fp64 functions differ by an ulp
    of fp64 at most, which the rounding to fp32 hides (lowmode_twin.drawn_start)."""
    pts = _instances(n, np.float32, 3)
    kw = dict(project_rigid=True, krylov=32, max_cycles=3, res_tol=RES_TOL[np.dtype(np.float32)])
    drawn = _run(pts, n, np.float32, seed=9, **kw)
    start = np.stack([lt.drawn_start(n, 9 + b, np.float32).reshape(-1) for b in range(3)])
    given = _run(pts, n, np.float32, start=start, seed=12345, **kw)
    assert np.array_equal(drawn.vectors, given.vectors) and np.array_equal(drawn.eigenvalues, given.eigenvalues)
    assert np.array_equal(drawn.residuals, given.residuals) and np.array_equal(drawn.products, given.products)


# ------------------------------------------------------------------------------ 4. limits
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_cycle_reports_the_rayleigh_quotient_and_residual_of_the_start(dtype):
    n = 13
    pts = _instances(n, dtype, 2)
    start = np.random.default_rng(3).standard_normal((2, 3 * n)).astype(dtype)
    r = _run(pts, n, dtype, start=start, max_cycles=1, res_tol=0.0)
    for b in range(2):
        assert (r.status[b], r.cycles[b], r.products[b]) == (dzo.LOWMODE_UNFINISHED, 1, 1)
        _, H, Pm = lt.dense_truth(pts[b], dtype, True)
        u = Pm @ start[b].astype(np.float64)
        u /= np.linalg.norm(u)
        bound = lt.gamma(n) * lt.EPS[np.dtype(dtype)] * np.linalg.norm(np.abs(H) @ np.abs(u))
        alpha = u @ H @ u
        assert abs(float(r.eigenvalues[b]) - alpha) <= bound + lt.EPS[np.dtype(dtype)] * abs(alpha)
        assert abs(r.residuals[b] - np.linalg.norm(Pm @ (H @ u) - alpha * u)) <= 2 * bound
        assert np.abs(r.vectors[b] - u).max() <= 8 * lt.EPS[np.dtype(dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_eigenvector_as_start_converges_with_one_product(dtype):
    n = 38
    pts = _instances(n, dtype, 2)
    tol = RES_TOL[np.dtype(dtype)]
    first = _run(pts, n, dtype, res_tol=tol, seed=1)
    assert first.status.tolist() == [dzo.LOWMODE_CONVERGED] * 2
    again = _run(pts, n, dtype, start=first.vectors, res_tol=64 * tol)
    assert again.status.tolist() == [dzo.LOWMODE_CONVERGED] * 2 and again.products.tolist() == [1, 1] and again.cycles.tolist() == [1, 1]
    assert np.abs(again.eigenvalues.astype(np.float64) - first.eigenvalues).max() <= 64 * tol * np.abs(first.eigenvalues).max()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_lanczos_vectors_still_find_the_lowest_mode(dtype):
    pts = _instances(4, dtype, 2)
    tol = RES_TOL[np.dtype(dtype)]
    r = _run(pts, 4, dtype, krylov=2, max_cycles=400, res_tol=tol, seed=2)
    for b in range(2):
        ev, rho, delta, _ = lt.truth_figures(pts[b], dtype, True, r.eigenvalues[b], r.vectors[b])
        assert r.status[b] == dzo.LOWMODE_CONVERGED and r.products[b] == 2 * (r.cycles[b] - 1) + 1
        assert float(r.eigenvalues[b]) - ev[0] <= rho + delta and ev[0] - float(r.eigenvalues[b]) <= delta


def test_the_largest_cluster_finishes_and_reports_the_residual_of_its_own_vector():
    """N = 1024, fp32, one instance, two cycles of eight vectors: the reported pair against dzo_pairwise_batch_hvp of the
    returned vector, projected on the host in fp64."""
    n, dtype = 1024, np.float32
    p = np.concatenate(tw.cluster(n, seed=n)).astype(dtype)
    dev = dzo.DeviceArray.from_host(p)
    r = dzo.lowest_modes(dev, n, krylov=8, max_cycles=2, res_tol=0.0, seed=3)
    assert (r.status[0], r.cycles[0], r.products[0]) == (dzo.LOWMODE_UNFINISHED, 2, 9)
    hu = dzo.pairwise_batch_hvp(dev, r.vectors, n).to_host().reshape(-1).astype(np.float64)
    u = r.vectors.to_host().reshape(-1).astype(np.float64)
    B = lt.rigid_basis(p.astype(np.float64))
    w = hu - B @ (B.T @ hu)
    lam = float(r.eigenvalues[0])
    H = ht.hessian_f64(p.astype(np.float64))
    delta = lt.gamma(n) * lt.EPS[np.dtype(dtype)] * np.linalg.norm(np.abs(H) @ np.abs(u))
    print("N = 1024: lambda", lam, "residual", r.residuals[0], "host", np.linalg.norm(w - lam * u), "delta", delta)
    assert np.isfinite(lam) and abs(np.linalg.norm(u) - 1) <= 4 * lt.EPS[np.dtype(dtype)]
    assert abs(lam - u @ w) <= delta
    assert abs(r.residuals[0] - np.linalg.norm(w - lam * u)) <= delta


@pytest.mark.parametrize("dtype", DTYPES)
def test_collinear_particles_fail_and_a_neighbour_does_not_notice(dtype):
    line = np.array([0.0, 1.1, 2.3, 0.0, 1.1, 2.3, 0.0, 1.1, 2.3])
    pts = np.stack([_instances(3, dtype, 1)[0], line, _instances(3, dtype, 2)[1]])
    tol = RES_TOL[np.dtype(dtype)]
    r = _run(pts, 3, dtype, res_tol=tol, seed=4)
    assert r.status.tolist() == [dzo.LOWMODE_CONVERGED, dzo.LOWMODE_FAILED, dzo.LOWMODE_CONVERGED]
    assert (r.cycles[1], r.products[1]) == (0, 0) and np.isnan(r.eigenvalues[1]) and np.isnan(r.residuals[1])
    alone = _run(pts[2:3], 3, dtype, res_tol=tol, seed=6)
    assert np.array_equal(alone.vectors[0], r.vectors[2]) and alone.eigenvalues[0] == r.eigenvalues[2]


def test_outputs_stay_inside_their_arrays_and_optional_ones_may_be_null():
    n, batch, dtype = 65, 2, np.float64
    pts = dzo.DeviceArray.from_host(_instances(n, dtype, batch).ravel())
    eig = dzo.DeviceArray.from_host(np.full(batch + 2 * GUARD, CANARY))
    vec = dzo.DeviceArray.from_host(np.full(3 * n * batch + 2 * GUARD, CANARY))
    rc = dzo.lib().dzo_pairwise_batch_lowest_mode(0, n, batch, dzo.F64, pts.ptr, 1, 4, 2, 0.0, 0, None, eig.view(GUARD, batch).ptr,
                                                  vec.view(GUARD, 3 * n * batch).ptr, None, None)
    assert rc == 0
    e, v = eig.to_host(), vec.to_host()
    for a in (e, v):
        assert np.all(a[:GUARD] == CANARY) and np.all(a[-GUARD:] == CANARY) and not np.any(a[GUARD:-GUARD] == CANARY)
    ref = _run(_instances(n, dtype, batch), n, dtype, krylov=4, max_cycles=2, res_tol=0.0, seed=0)
    assert np.array_equal(e[GUARD:-GUARD], ref.eigenvalues) and np.array_equal(v[GUARD:-GUARD], ref.vectors.ravel())


def test_argument_errors():
    pts = dzo.DeviceArray.from_host(_instances(13, np.float64, 1).ravel())
    for kw in (dict(krylov=1), dict(krylov=33), dict(max_cycles=0), dict(res_tol=-1.0), dict(res_tol=float("nan")), dict(res_tol=float("inf"))):
        with pytest.raises(dzo.DzoError) as e:
            dzo.lowest_modes(pts, 13, **kw)
        assert e.value.code == 1, kw
    two = dzo.DeviceArray.from_host(np.array([0.0, 1.1, 0.0, 0.0, 0.0, 0.0]))
    with pytest.raises(dzo.DzoError) as e:
        dzo.lowest_modes(two, 2, project_rigid=True)
    assert e.value.code == 1
    assert dzo.lowest_modes(two, 2, project_rigid=False, res_tol=2.0 ** -30).status.tolist() == [dzo.LOWMODE_CONVERGED]
    big = dzo.DeviceArray.zeros(3 * 1025)
    with pytest.raises(dzo.DzoError) as e:
        dzo.lowest_modes(big, 1025)
    assert e.value.code == 5
    out = dzo.DeviceArray.zeros(64)
    args = [0, 13, 1, dzo.F64, pts.ptr, 1, 8, 2, 0.0, 0, None, out.ptr, out.ptr, None, None]
    for k in (4, 11, 12):
        bad = list(args)
        bad[k] = None
        assert dzo.lib().dzo_pairwise_batch_lowest_mode(*bad) == 1, k
    for k, v in ((0, 7), (3, 9), (2, 0)):
        bad = list(args)
        bad[k] = v
        assert dzo.lib().dzo_pairwise_batch_lowest_mode(*bad) == 1, k
    host = np.zeros(39)
    bad = list(args)
    bad[4] = host.ctypes.data
    assert dzo.lib().dzo_pairwise_batch_lowest_mode(*bad) == 3


# ------------------------------------------------------------------------------ 5. the example
def test_lj_lowest_mode_example_runs(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_lowest_mode")
    out = subprocess.run([exe, "38", "16"], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
    assert "16 converged" in out.stdout and "largest difference from eigenvalue 6" in out.stdout
