"""Batched Hessian-vector products and dense Hessians of Lennard-Jones clusters on the device (csrc/dzo_hessian_batch.hip) against
their CPU twin (tests/hessian_twin.py, tests/pairwise_twin.py).

1. the product bit for bit: N = 2 against the single-pair twin, N = 3, 4, 13 against the twin that replays the device's order;
2. the product against the DERIVED bound of tests/test_gpu_pairwise.py, |gpu_i - exact_i| <= (N + 32) u S_i, at the wave and
   block edges, and the curvatures u.Hu, u.u within 3N u64 sum|terms| of the fp64 dots of the returned vectors;
3. independence: an instance's bits alone, anywhere in a batch, with a shared or a repeated point, and on a second call;
4. the column identity with ==: column c of the dense Hessian against the product with the unit direction e_c; translation rows;
   canaries around the output;
5. spectra of the two polished minima and of the planar LJ4 saddle, by Weyl's inequality; Morse indices;
6. the hand-over from ParallelTempering.quench;
7. error codes and coincident particles;
8. the plain-C example.
"""
import functools
import subprocess

import numpy as np
import pytest

import hessian_twin as ht
import pairwise_twin as tw
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = {np.dtype(np.float64): LD(2.0) ** -53, np.dtype(np.float32): LD(2.0) ** -24}
U64 = LD(2.0) ** -53
DTYPES = [np.float64, np.float32]
NS_BOUND = [38, 63, 64, 65, 66, 255, 256, 257, 1024]      # wave / block edges, the second trip of the strided loops, the largest
NS_COLUMNS = [2, 3, 13, 38, 63, 64, 65, 66, 255, 256, 257]
CANARY = 12345.0
GUARD = 64


# ------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _instances(n, dtype, batch=3):
    """`batch` distinct instances of n particles: the configuration of tests/test_gpu_pairwise.py (tw.cluster(n, seed=n),
    directions from default_rng(1000 + n)), then jitters of it with seeds n + k.  (points, directions): fp64 arrays (batch, 3n)
    holding values of `dtype`, so that the twin sees exactly what the device sees."""
    base = tw.cluster(n, seed=n)
    pts, dirs = [], []
    for k in range(batch):
        xyz = base if k == 0 else tw.jittered(base, seed=n + k, jitter=0.01)
        pts.append(np.concatenate(xyz))
        dirs.append(np.random.default_rng(1000 + n + k).normal(size=3 * n))
    cast = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    p, d = cast(pts), cast(dirs)
    p.setflags(write=False); d.setflags(write=False)
    return p, d


def _guarded(size, dtype):
    """A device buffer of `size` elements between two runs of GUARD canaries: (whole buffer, view of the middle)."""
    buf = dzo.DeviceArray.from_host(np.full(size + 2 * GUARD, CANARY, dtype=dtype))
    return buf, buf.view(GUARD, size)


def _guards_intact(buf):
    h = buf.to_host()
    return bool(np.all(h[:GUARD] == CANARY) and np.all(h[-GUARD:] == CANARY))


def _hvp(points, directions, n, dtype, curvatures=True, shared_point=False):
    """(products (batch, 3, n), curvatures (batch, 2)) of host arrays; canaries around the products are checked."""
    d = dzo.DeviceArray.from_host(np.ascontiguousarray(directions).ravel(), dtype=dtype)
    p = dzo.DeviceArray.from_host(np.ascontiguousarray(points).ravel(), dtype=dtype)
    buf, out = _guarded(d.size, dtype)
    r = dzo.pairwise_batch_hvp(p, d, n, products=out, curvatures=curvatures, shared_point=shared_point)
    assert _guards_intact(buf), "the product kernel wrote outside its output"
    prod = out.to_host().reshape(-1, 3, n)
    return (prod, r[1]) if curvatures else (prod, None)


def _hessian(points, n, dtype):
    """Host array [b, c, r] of the dense Hessians; canaries around the device output are checked."""
    p = dzo.DeviceArray.from_host(np.ascontiguousarray(points).ravel(), dtype=dtype)
    batch = p.size // (3 * n)
    buf, out = _guarded(9 * n * n * batch, dtype)
    h = dzo.pairwise_batch_hessian(p, n, out=out)
    assert _guards_intact(buf), "the Hessian kernel wrote outside its output"
    return h


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _split(v, n):
    return v[:n], v[n:2 * n], v[2 * n:]


# ------------------------------------------------------------------------------ 1. the product, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_pairs_bit_for_bit(dtype):
    """200 random pairs as 200 instances of one launch: at N = 2 no summation order exists."""
    rng = np.random.default_rng(20)
    pts, dirs, want = [], [], []
    for k in range(200):
        r2 = np.exp(rng.uniform(np.log(0.6), np.log(16.0)))
        d = rng.normal(size=3); d *= np.sqrt(r2) / np.linalg.norm(d)
        p0 = rng.uniform(-1, 1, size=3)
        p0, p1 = np.asarray(p0, dtype), np.asarray(p0 + d, dtype)
        u0, u1 = np.asarray(rng.normal(size=3), dtype), np.asarray(rng.normal(size=3), dtype)
        pts.append([p0[0], p1[0], p0[1], p1[1], p0[2], p1[2]])
        dirs.append([u0[0], u1[0], u0[1], u1[1], u0[2], u1[2]])
        want.append(np.array(tw.pair_hvp(p0, p1, u0, u1, dtype), dtype=dtype).T)      # [component, particle]
    got, _ = _hvp(np.array(pts, dtype=dtype), np.array(dirs, dtype=dtype), 2, dtype)
    want = np.array(want, dtype=dtype)
    bad = [k for k in range(200) if not np.array_equal(_bits(got[k]), _bits(want[k]))]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3, 4, 13])
def test_small_clusters_bit_for_bit(n, dtype):
    """The twin replays the device's order: rows over j = 0 .. N-1 from +0, every operation rounded once."""
    base = tw.jittered(tw.icosahedron13(), seed=n)
    pts = np.asarray([np.concatenate([a[:n] for a in tw.jittered(base, seed=50 + k, jitter=0.01)]) for k in range(2)], dtype=dtype)
    dirs = np.asarray(np.random.default_rng(7 + n).normal(size=(2, 3 * n)), dtype=dtype)
    got, _ = _hvp(pts, dirs, n, dtype)
    for k in range(2):
        want = ht.hvp_bits(*_split(pts[k], n), *_split(dirs[k], n), dtype)
        assert np.array_equal(got[k], want), (k, got[k], want)              # values; the sign of a zero is free


# ------------------------------------------------------------------------------ 2. the derived bound
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS_BOUND)
def test_products_within_the_derived_bound(n, dtype):
    """|gpu - exact| <= (N + 32) u S_i against the longdouble sums, S_i one scale per row (tests/test_gpu_pairwise.py).  The
    curvatures are fp64 dots of 3N products: any order costs at most 3N u64 sum|terms| against the exact dot of the SAME
    vectors (the returned products, the given directions)."""
    pts, dirs = _instances(n, dtype)
    got, curv = _hvp(pts, dirs, n, dtype)
    u = U[np.dtype(dtype)]
    worst = 0.0
    for k in range(len(pts)):
        exact, S, _ = tw.hvp(*_split(pts[k], n), *_split(dirs[k], n))
        bound = LD(n + 32) * u * S[None, :]
        err = np.abs(got[k].astype(LD) - exact)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (n, k, np.argwhere(~(err <= bound))[:5].tolist())
        uvec, pvec = dirs[k].astype(LD), got[k].reshape(-1).astype(LD)
        for what, a, b in ((0, uvec, pvec), (1, uvec, uvec)):
            terms = a * b
            tol = LD(3 * n) * U64 * np.abs(terms).sum()
            assert abs(LD(curv[k, what]) - terms.sum()) <= tol, (n, k, what, curv[k, what], float(terms.sum()), float(tol))
    print(f"hvp N={n} {np.dtype(dtype).name}: worst error / bound = {worst:.4f}")


# ------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [13, 64, 65, 257])
def test_an_instance_computes_the_same_bits_anywhere(n, dtype):
    pts, dirs = _instances(n, dtype)
    alone, c_alone = _hvp(pts[:1], dirs[:1], n, dtype)
    h_alone = _hessian(pts[:1], n, dtype)
    for pos in (0, 2, 4):
        order = [1, 2, 1, 2, 1]
        order[pos] = 0
        got, curv = _hvp(pts[order], dirs[order], n, dtype)
        assert _same_bits(got[pos], alone[0]) and _same_bits(curv[pos], c_alone[0]), pos
        assert _same_bits(_hessian(pts[order], n, dtype)[pos], h_alone[0]), pos
    # five directions on one point: shared (point_stride 0) against the point repeated (point_stride 3N)
    five = np.stack([dirs[0], dirs[1], dirs[2], -dirs[0], dirs[1] + dirs[2]])
    shared, c_shared = _hvp(pts[:1], five, n, dtype, shared_point=True)
    repeated, c_repeated = _hvp(np.repeat(pts[:1], 5, axis=0), five, n, dtype)
    assert _same_bits(shared, repeated) and _same_bits(c_shared, c_repeated)
    assert _same_bits(shared[0], alone[0])
    again, c_again = _hvp(pts[:1], five, n, dtype, shared_point=True)
    assert _same_bits(again, shared) and _same_bits(c_again, c_shared)
    assert _same_bits(_hessian(pts[:1], n, dtype), h_alone)
    no_curv, _ = _hvp(pts[:1], dirs[:1], n, dtype, curvatures=False)          # curvatures_dev = NULL
    assert _same_bits(no_curv, alone)


# ------------------------------------------------------------------------------ 4. the column identity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS_COLUMNS)
def test_hessian_columns_are_products_of_unit_vectors(n, dtype):
    """hessians[b][:, c] == the product of points[b] with e_c: ONE call with point_stride = 0, batch = 3N and the identity as
    directions gives all columns.  Then the translation rows: row r of H t_a is the row's diagonal-block entry, the sequential
    sum of N - 1 rounded terms doubled, minus the exact sum of the same terms doubled (the off-diagonal entries): the error of
    one sequential sum, within (N + 32) u sum_c |H[r, c] t_a[c]|."""
    pts = _instances(n, dtype)[0][:2] if n > 2 else np.asarray([[0.0, 1.1, 0.0, 0.3, 0.0, -0.2], [0.1, 0.9, 0.0, 0.5, 0.2, 1.0]], dtype=dtype)
    H = _hessian(pts, n, dtype)                               # [b, c, r]
    assert np.all(np.isfinite(H))
    eye = np.eye(3 * n, dtype=dtype)
    for b in range(2):
        cols, _ = _hvp(pts[b:b + 1], eye, n, dtype, curvatures=False, shared_point=True)
        cols = cols.reshape(3 * n, 3 * n)                     # [c, r]
        bad = np.argwhere(~(H[b] == cols))
        assert bad.size == 0, (n, b, bad[:5].tolist(), H[b][tuple(bad[0])], cols[tuple(bad[0])])
        Hl = H[b].astype(LD)
        for a in range(3):
            part = Hl[a * n:(a + 1) * n, :]                   # the columns of component a: [j, r]
            resid, scale = np.abs(part.sum(axis=0)), np.abs(part).sum(axis=0)
            assert np.all(resid <= LD(n + 32) * U[np.dtype(dtype)] * scale), (n, b, a, float(np.max(resid / scale)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hessian_columns_at_the_largest_size(dtype):
    """N = 1024, one instance: the columns of particles 0, 255, 256 and 1023 (first and last of a thread's first trip, first of
    its second, the last of all), copied from the device one by one."""
    n = 1024
    pts = _instances(n, dtype)[0][:1]
    p = dzo.DeviceArray.from_host(pts.ravel(), dtype=dtype)
    buf, out = _guarded(9 * n * n, dtype)
    rc = dzo.lib().dzo_pairwise_batch_hessian(dzo.RADIAL_LENNARD_JONES, n, 1, dzo._dt(dtype), p.ptr, out.ptr)
    assert rc == 0, dzo.lib().dzo_last_error()
    assert _guards_intact(buf)
    columns = [c * n + j for c in range(3) for j in (0, 255, 256, 1023)]
    eye = np.zeros((len(columns), 3 * n), dtype=dtype)
    eye[np.arange(len(columns)), columns] = 1
    want, _ = _hvp(pts, eye, n, dtype, curvatures=False, shared_point=True)
    for k, c in enumerate(columns):
        col = out.view(3 * n * c, 3 * n).to_host()
        assert np.all(np.isfinite(col)) and np.count_nonzero(col) > 0
        assert np.all(col == want[k].reshape(-1)), (c, np.argwhere(~(col == want[k].reshape(-1)))[:5].tolist())


# ------------------------------------------------------------------------------ 5. spectra
FIXTURES = {"ico13": (lambda: ht.polished_minimum(tw.icosahedron13), 13, (0, 6)),
            "oct38": (lambda: ht.polished_minimum(tw.octahedron38), 38, (0, 6)),
            "square4": (ht.square4, 4, (2, 6))}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_spectra_and_morse_indices(name, dtype):
    """Weyl: |lambda_k(A) - lambda_k(B)| <= ||A - B||_2 <= ||A - B||_F, with A = sym(H_gpu) and B the fp64 Hessian of the same
    (rounded) point, plus the two eigen-solves' own backward error, 30 3N 2^-53 lambda_max.  The Frobenius norm itself is held
    to a scale derived like the products' bound: an entry is a sum of at most N terms and errs by at most (N + 32) u times the
    sum of their absolute values, which is of the size of the largest entry; 9 N^2 such entries give a norm of at most
    3N (N + 32) u max|H|."""
    make, n, index = FIXTURES[name]
    p = np.asarray(make(), dtype=dtype).astype(np.float64)
    dev = dzo.DeviceArray.from_host(p, dtype=dtype)
    ev = dzo.hessian_eigenvalues(dev, n)
    assert ev.shape == (1, 3 * n) and ev.dtype == np.float64 and np.all(np.diff(ev[0]) >= 0)
    H = dzo.pairwise_batch_hessian(dev, n)[0].astype(np.float64)
    Hcpu = ht.hessian_f64(p)
    fro = np.linalg.norm(0.5 * (H + H.T) - Hcpu)
    want = ht.spectrum_of(p)
    lam_max = want[-1]
    assert fro <= float(LD(n + 32) * U[np.dtype(dtype)]) * 3 * n * np.abs(Hcpu).max(), fro
    bound = fro + 30 * 3 * n * 2.0 ** -53 * lam_max
    err = np.abs(ev[0] - want)
    print(f"{name} {np.dtype(dtype).name}: ||sym(H_gpu) - H_cpu||_F = {fro:.3e}, worst eigenvalue error {err.max():.3e}, bound {bound:.3e}")
    assert np.all(err <= bound), (err.max(), bound)
    negatives, zeros = dzo.morse_index(ev, ht.zero_tolerance(dtype, lam_max))
    assert (int(negatives[0]), int(zeros[0])) == index, (negatives, zeros, ev[0][:10])


# ------------------------------------------------------------------------------ 6. the hand-over
@pytest.mark.parametrize("dtype", DTYPES)
def test_quenched_replicas_are_minima(dtype):
    """ParallelTempering.quench hands its array to hessian_eigenvalues.  Which minimum a replica reaches is not asserted.  A
    stuck instance is a minimum to the line search's resolution, not a polished one: a rigid rotation t = w x r has
    H t = -w x g, so the residual gradient g moves the six zero modes by up to about |g| / |r| -- zero_tol is the larger of the
    fixtures' tolerance and 10 |g|_2 of that instance."""
    n, replicas = 13, 8
    starts = np.asarray([np.concatenate(tw.jittered(tw.icosahedron13(), seed=k)) for k in range(replicas)], dtype=dtype)
    rdev = dzo.DeviceArray.from_host(starts.ravel())
    pt = dzo.ParallelTempering(rdev, n, np.geomspace(20.0, 5.0, replicas), [0.05] * replicas, 3.0, base_seed=5)
    pt.run(100, 2)
    energies, minima, opt = pt.quench(max_steps=2000 if dtype == np.float64 else 200)
    ev = dzo.hessian_eigenvalues(minima, n)
    assert ev.shape == (replicas, 3 * n)
    stuck, grads = opt.is_stuck, opt.current_gradients.astype(np.float64)
    print(f"{np.dtype(dtype).name}: {int(stuck.sum())} of {replicas} stuck; energies {np.sort(energies)}")
    for k in np.flatnonzero(stuck):
        assert np.all(np.isfinite(ev[k])), k
        tol = max(ht.zero_tolerance(dtype, ev[k, -1]), 10 * np.linalg.norm(grads[k]))
        negatives, zeros = dzo.morse_index(ev[k], tol)
        assert int(negatives[0]) == 0, (k, ev[k][:8], tol)


# ------------------------------------------------------------------------------ 7. errors
def test_error_codes():
    n, batch = 38, 2
    pts, dirs = _instances(n, np.float64)
    p = dzo.DeviceArray.from_host(pts[:batch].ravel())
    d = dzo.DeviceArray.from_host(dirs[:batch].ravel())
    out = dzo.DeviceArray.zeros(3 * n * batch)
    hes = dzo.DeviceArray.zeros(9 * n * n * batch)
    curv = dzo.DeviceArray.zeros(2 * batch)
    L = dzo.lib()
    hvp, hessian = L.dzo_pairwise_batch_hvp, L.dzo_pairwise_batch_hessian
    ok = (0, n, batch, dzo.F64, p.ptr, 3 * n, d.ptr, out.ptr, curv.ptr)

    def with_(**kw):
        names = ["radial", "n", "batch", "dtype", "points", "stride", "directions", "products", "curvatures"]
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    assert hvp(*ok) == 0
    assert hvp(*with_(curvatures=None)) == 0                                   # NULL is allowed
    assert hvp(*with_(stride=0)) == 0
    assert hvp(*with_(radial=7)) == 1 and hessian(7, n, batch, dzo.F64, p.ptr, hes.ptr) == 1
    assert hvp(*with_(dtype=9)) == 1 and hessian(0, n, batch, 9, p.ptr, hes.ptr) == 1
    assert hvp(*with_(n=0)) == 1 and hessian(0, 0, batch, dzo.F64, p.ptr, hes.ptr) == 1
    assert hvp(*with_(batch=0)) == 1 and hessian(0, n, 0, dzo.F64, p.ptr, hes.ptr) == 1
    for stride in (-1, 1, 3 * n - 1, -3 * n):
        assert hvp(*with_(stride=stride)) == 1, stride
    for name in ("points", "directions", "products"):
        assert hvp(*with_(**{name: None})) == 1, name
    assert hessian(0, n, batch, dzo.F64, None, hes.ptr) == 1 and hessian(0, n, batch, dzo.F64, p.ptr, None) == 1
    assert hvp(*with_(n=1025)) == 5 and hessian(0, 1025, 1, dzo.F64, p.ptr, hes.ptr) == 5
    assert dzo.HESSIAN_BATCH_MAX_PARTICLES == 1024
    host = np.ascontiguousarray(pts[:batch].ravel())
    hcurv = np.zeros(2 * batch)
    for name in ("points", "directions", "products"):
        assert hvp(*with_(**{name: host.ctypes.data})) == 3, name
    assert hvp(*with_(curvatures=hcurv.ctypes.data)) == 3
    assert hessian(0, n, batch, dzo.F64, host.ctypes.data, hes.ptr) == 3
    assert hessian(0, n, batch, dzo.F64, p.ptr, host.ctypes.data) == 3
    with pytest.raises(dzo.AssertionFailed):
        dzo.pairwise_batch_hvp(dzo.DeviceArray(3 * n * batch, np.float64, ptr=host.ctypes.data, owner=False), d, n)
    with pytest.raises(TypeError):
        dzo.morse_index(np.zeros(3))                                           # zero_tol has no default


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [38, 70])
def test_coincident_particles(n, dtype):
    """The treatment of tests/test_gpu_pairwise.py: a coincident pair gives non-finite values in ITS rows, no fault, and nothing
    outside the instance changes."""
    pts, dirs = _instances(n, dtype)
    bad = pts.copy()
    for c in range(3):
        bad[1, c * n + 7] = bad[1, c * n + 5]
    good, c_good = _hvp(pts, dirs, n, dtype)
    got, curv = _hvp(bad, dirs, n, dtype)                                      # canaries checked inside
    assert _same_bits(got[0], good[0]) and _same_bits(got[2], good[2])
    assert _same_bits(curv[0], c_good[0]) and _same_bits(curv[2], c_good[2])
    others = [k for k in range(n) if k not in (5, 7)]
    assert not np.all(np.isfinite(got[1][:, [5, 7]])) and np.all(np.isfinite(got[1][:, others]))
    assert not np.isfinite(curv[1, 0]) and np.isfinite(curv[1, 1])
    Hgood, H = _hessian(pts, n, dtype), _hessian(bad, n, dtype)
    assert _same_bits(H[0], Hgood[0]) and _same_bits(H[2], Hgood[2])
    rows = np.array([c * n + k for c in range(3) for k in (5, 7)])
    mask = np.zeros((3 * n, 3 * n), dtype=bool)                                # [c, r]: blocks (5, 7), (7, 5), (5, 5), (7, 7)
    mask[np.ix_(rows, rows)] = True
    assert np.all(np.isfinite(H[1][~mask])) and not np.all(np.isfinite(H[1][mask]))


# ------------------------------------------------------------------------------ 8. the plain-C example
def test_lj_hessian_example_runs(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_hessian")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
    lines = {l.split(":", 1)[0]: l.split(":", 1)[1] for l in r.stdout.splitlines() if ":" in l}
    trace = float(lines["trace"])
    point = np.array([float(v) for v in lines["point"].split()])
    assert point.size == 39
    ev = dzo.hessian_eigenvalues(dzo.DeviceArray.from_host(point), 13)
    assert abs(trace - ev.sum()) <= 1e-9 * abs(trace), (trace, ev.sum())
