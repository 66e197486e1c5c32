"""The structure unit on the device (csrc/dzo_structure.hip) against its CPU twin (tests/structure_twin.py).

1. Fingerprints at N = 1, 2, 3 (the smallest), 13, 38 (the icosahedron and the octahedron), 63, 64, 65 (the wave/block seam), 127,
   128, 129, 257 (the power-of-two padding of the sort on either side, one or two particles per thread) and 1024 (the maximum),
   batch 1, 3 and 67, both element types.  A batch repeats three distinct clusters (the twin is computed once per cluster):

   * the sorted per-particle energies equal the twin's with ``==`` on the bits;
   * E equals ``dzo.pairwise_batch_energy_gradient`` with ``==`` on the bits;
   * the sorted distances are within eps (4 sum_c |r_ic - c_c| |c_c| + 4 d_i) of the twin's, eps the unit roundoff: the two
     centroids are fp64 sums of the same terms rounded once to T, so they differ by at most one unit in the last place of c
     (2 eps |c_c|), which moves d_i by 2 |r_ic - c_c| 2 eps |c_c| per coordinate, and d_i itself carries three roundings on each
     side.  (The twin sums in the device's order, so the test also prints whether the bits are equal: they are.);
   * cluster 0 gives the same bits alone and at positions 0, 33 and 66 of the batch of 67;
   * one coincident pair in the middle instance makes that fingerprint non-finite and leaves its neighbours' bits alone.

2. The classifier: batches of 1, 2, 65 and 257 built from five distinct 13-atom clusters, every instance another random
   orthogonal matrix (a reflection or not), translation and relabelling, interleaved.  tol is 100 x the rounding bound of
   tests/test_structure_twin.py (gamma_N times the largest sum of absolute values); the test first asserts ON THE TWIN that the
   smallest relative distance between two distinct clusters is at least 100 x tol.  The device labels equal the twin's labels of
   the downloaded fingerprints exactly, and they are b mod 5.  Then the non-transitive chain, the non-finite rows, 16384 rows
   whose representatives fill every word of the mask, and every error code.

3. connect_saddles on LJ7, whose four minima have the energies LJ7 below.  They come from an fp64 CPU run of
   tests/quench_twin.py: 60 starts ``default_rng(7).normal(size=(3, 7)) * 0.55`` quenched with ``Quench(p, 0.01, 10)``;
   the four energies reached more than once (15, 7, 8 and 24 times, each to all twelve printed digits) are the four minima.
"""
import functools

import ctypes
import numpy as np
import pytest

import pairwise_twin as tw
import structure_twin as st
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 13, 38, 63, 64, 65, 127, 128, 129, 257, 1024]
DTYPES = [np.float64, np.float32]
LJ7 = (-16.505384168012, -15.935043060489, -15.593210938193, -15.533060054575)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _clusters(n, dtype):
    """Three distinct clusters of n particles in ``dtype`` (the ideal one first) and their twin fingerprints: computed once."""
    ideal = np.concatenate(tw.cluster(n, 0))
    pts = [ideal] + [np.concatenate(tw.jittered(tw.cluster(n, 0), seed)) for seed in (1, 2)]
    pts = [np.asarray(p, dtype=dtype) for p in pts]
    return pts, [st.fingerprint(p, dtype) for p in pts]


def _device(points, n):
    fp, e = dzo.structure_fingerprints(dzo.DeviceArray.from_host(np.ascontiguousarray(points).ravel()), n)
    return fp.to_host(), e


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_fingerprints_equal_the_twin(n, dtype):
    pts, twin = _clusters(n, dtype)
    eps = st.EPS[np.dtype(dtype)]
    rows = {}
    for batch in (67, 3, 1):
        points = np.stack([pts[b % 3] for b in range(batch)])
        fp, e = _device(points, n)
        assert fp.shape == (batch, 2 * n) and fp.dtype == np.dtype(dtype) and e.shape == (batch,)
        assert _same_bits(e, dzo.pairwise_batch_energy_gradient(dzo.DeviceArray.from_host(points.ravel()), n))
        for b in range(batch):
            want, E = twin[b % 3]
            assert _same_bits(fp[b, :n], want[:n]), (n, batch, b)
            assert _same_bits(e[b:b + 1], np.array([E], dtype=dtype)), (n, batch, b, e[b], E)
            P = points[b].reshape(3, n).astype(np.float64)
            c = P.mean(axis=1, keepdims=True)
            bound = eps * (4 * (np.abs(P - c) * np.abs(c)).sum(axis=0) + 4 * ((P - c) ** 2).sum(axis=0))
            err = np.abs(fp[b, n:].astype(np.float64) - want[n:].astype(np.float64))
            assert err.max() <= np.sort(bound)[-1] and np.all(np.diff(fp[b, n:]) >= 0), (n, batch, b, err.max(), bound.max())
            if batch == 67 and b == 0:
                print("n = %d %s: distances differ from the twin by %.2e at most (bound %.2e), bits equal: %s"
                      % (n, np.dtype(dtype).name, err.max(), bound.max(), _same_bits(fp[b, n:], want[n:])))
        rows[batch] = fp
    for other in (rows[67][33], rows[67][66], rows[3][0], rows[1][0]):
        assert _same_bits(rows[67][0], other)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [13, 65])
def test_a_coincident_pair_spoils_its_instance_only(n, dtype):
    pts, _ = _clusters(n, dtype)
    points = np.stack(pts)
    clean, e_clean = _device(points, n)
    bad = points.copy().reshape(3, 3, n)
    bad[1, :, 5] = bad[1, :, 2]
    fp, e = _device(bad.reshape(3, 3 * n), n)
    assert _same_bits(fp[0], clean[0]) and _same_bits(fp[2], clean[2]) and _same_bits(e[[0, 2]], e_clean[[0, 2]])
    assert np.isnan(e[1]) and np.isnan(fp[1, n - 2:n]).all() and np.isfinite(fp[1, :n - 2]).all() and np.isfinite(fp[1, n:]).all()
    labels, reps = dzo.classify_structures(dzo.DeviceArray.from_host(fp), 1e-3)
    assert labels.tolist() == [0, -1, 2] and reps.tolist() == [0, 2]


# ------------------------------------------------------------------------------ the classifier
K, NC, SHIFT = 5, 13, 0.1


@functools.lru_cache(maxsize=None)
def _families(dtype):
    """Five distinct 13-atom clusters (jittered cubic lattice fragments of spacing 1.15^k, centred, so that the sums of absolute
    values that scale the bound stay small), tol and the twin's check of it.  Measured on the twin: the closest two are 0.46
    apart, tol is 6.6e-4 in fp32 and 1.2e-12 in fp64, and the copies stay within 1.3 % of tol."""
    def base(k):
        P = np.stack(tw.lattice(NC, seed=k, spacing=1.15 ** k, jitter=0.03))
        return (P - P.mean(axis=1, keepdims=True)).reshape(-1)

    bases = [base(k) for k in range(K)]
    g = st.gamma(NC, dtype)
    images = [np.asarray(st.image(p, seed=100 + k, shift=SHIFT), dtype=dtype).astype(np.float64) for k, p in enumerate(bases)]
    bound = g * max(max(float(st.row_scales(p)[1].max()), float(st.distance_scales(p)[1].max())) for p in bases + images)
    tol = 100.0 * bound
    prints = [st.fingerprint(np.asarray(p, dtype=dtype), dtype)[0] for p in bases]
    apart = min(st.relative_distance(prints[i], prints[j]) for i in range(K) for j in range(i))
    return bases, tol, apart


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [1, 2, 65, 257])
def test_labels_of_moved_reflected_relabelled_copies_equal_the_twin(batch, dtype):
    bases, tol, apart = _families(dtype)
    print("%s: tol = %.3e, the closest two distinct clusters are %.3e apart" % (np.dtype(dtype).name, tol, apart))
    assert apart >= 100.0 * tol                              # on the twin, before the device is touched
    points = np.stack([np.asarray(st.image(bases[b % K], seed=b, shift=SHIFT), dtype=dtype) for b in range(batch)])
    fp_dev, _ = dzo.structure_fingerprints(dzo.DeviceArray.from_host(points.ravel()), NC)
    labels, reps = dzo.classify_structures(fp_dev, tol)
    want, want_reps = st.classify(fp_dev.to_host(), tol)
    assert labels.dtype == np.int32 and np.array_equal(labels, want) and np.array_equal(reps, want_reps)
    assert labels.tolist() == [b % K for b in range(batch)]
    got = dzo.unique_structures(dzo.DeviceArray.from_host(points.ravel()), NC, tol)
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], reps) and got[2].sum() == batch and len(got[3]) == len(reps)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_chain_non_finite_rows_and_a_database_in_front(dtype):
    F = np.zeros((3, 4), dtype=dtype)
    F[1, 2], F[2, 2] = 0.6e-3, 1.2e-3                        # a ~ b, b ~ c, a !~ c
    labels, reps = dzo.classify_structures(dzo.DeviceArray.from_host(F), 1e-3)
    assert labels.tolist() == [0, 0, 2] == st.classify(F, 1e-3)[0].tolist() and reps.tolist() == [0, 2]
    F = np.array([[1.0, np.nan], [1.0, 2.0], [np.inf, 2.0], [1.0, 2.0], [np.inf, 2.0], [-np.inf, 2.0]], dtype=dtype)
    labels, reps = dzo.classify_structures(dzo.DeviceArray.from_host(F), 1.0)
    assert labels.tolist() == [-1, 1, -1, 1, -1, -1] == st.classify(F, 1.0)[0].tolist() and reps.tolist() == [1]
    known = np.array([[3.0, 1.0], [1.0, 2.0], [2.0, 2.0]], dtype=dtype)
    found = np.array([[2.0, 2.0], [5.0, 5.0], [3.0, 1.0], [5.0, 5.0]], dtype=dtype)
    labels, _ = dzo.classify_structures(dzo.DeviceArray.from_host(np.concatenate([known, found])), 1e-6)
    assert labels.tolist() == [0, 1, 2, 2, 4, 0, 4]
    labels, reps = dzo.classify_structures(dzo.DeviceArray.from_host(np.array([[1.0, 1.5]], dtype=dtype).repeat(3, axis=0)), 0.0)
    assert labels.tolist() == [0, 0, 0] and reps.tolist() == [0]


def test_the_largest_batch_fills_every_word_of_the_mask():
    """16384 rows in families of 40 consecutive rows, three distinct values per family (0.25 apart, which tol times the largest
    value, 820, does not reach): new representatives appear all the way through the batch, so they sit in all 256 words of the
    mask and in all four words a lane holds.  Every 97th row is not finite."""
    batch = dzo.STRUCTURE_MAX_BATCH
    F = np.zeros((batch, 3), dtype=np.float32)
    F[:, 1] = 2.0 * (np.arange(batch) // 40) + 0.25 * (np.arange(batch) % 3)
    F[::97, 2] = np.nan
    labels, reps = dzo.classify_structures(dzo.DeviceArray.from_host(F), 0.26 / 1024)     # relative to |a| <= 820
    want, want_reps = st.classify(F, 0.26 / 1024)
    assert np.array_equal(labels, want) and np.array_equal(reps, want_reps)
    assert (labels == -1).sum() == len(range(0, batch, 97)) and len(reps) > batch // 40 and reps.max() > batch - 64


def test_error_codes():
    d = dzo.DeviceArray.zeros((4, 6))
    labels = dzo.DeviceArray((4,), np.int32)
    count = ctypes.c_int32(0)
    call = dzo.lib().dzo_structure_batch_classify
    ok = lambda *a: call(*a)
    assert ok(6, 4, dzo.F64, d.ptr, 1e-3, labels.ptr, ctypes.byref(count)) == 0 and count.value == 1
    for args in ((6, 4, dzo.F64, d.ptr, -1e-3, labels.ptr, ctypes.byref(count)), (6, 4, dzo.F64, d.ptr, float("nan"), labels.ptr, ctypes.byref(count)),
                 (0, 4, dzo.F64, d.ptr, 1e-3, labels.ptr, ctypes.byref(count)), (6, 0, dzo.F64, d.ptr, 1e-3, labels.ptr, ctypes.byref(count)),
                 (6, 4, 9, d.ptr, 1e-3, labels.ptr, ctypes.byref(count)), (6, 4, dzo.F64, None, 1e-3, labels.ptr, ctypes.byref(count)),
                 (6, 4, dzo.F64, d.ptr, 1e-3, None, ctypes.byref(count)), (6, 4, dzo.F64, d.ptr, 1e-3, labels.ptr, None)):
        assert ok(*args) == 1, args                          # DZO_ERR_INVALID
    big = dzo.DeviceArray.zeros((dzo.STRUCTURE_MAX_BATCH + 1, 1), np.float32)
    with pytest.raises(dzo.DzoError) as err:
        dzo.classify_structures(big, 1e-3)
    assert err.value.code == 5                               # DZO_ERR_UNSUPPORTED
    host = np.zeros(24)
    assert ok(6, 4, dzo.F64, host.ctypes.data, 1e-3, labels.ptr, ctypes.byref(count)) == 3     # DZO_ERR_ASSERT
    fingerprint = dzo.lib().dzo_structure_batch_fingerprint
    pts, out = dzo.DeviceArray.zeros(3 * 1025), dzo.DeviceArray.zeros(2 * 1025)
    assert fingerprint(0, 1025, 1, dzo.F64, pts.ptr, out.ptr, None) == 5
    assert fingerprint(0, 4, 1, dzo.F64, pts.ptr, out.ptr, None) == 0          # energies may be NULL
    for args in ((1, 4, 1, dzo.F64, pts.ptr, out.ptr, None), (0, 0, 1, dzo.F64, pts.ptr, out.ptr, None), (0, 4, 0, dzo.F64, pts.ptr, out.ptr, None),
                 (0, 4, 1, 9, pts.ptr, out.ptr, None), (0, 4, 1, dzo.F64, None, out.ptr, None), (0, 4, 1, dzo.F64, pts.ptr, None, None)):
        assert fingerprint(*args) == 1, args
    assert fingerprint(0, 4, 1, dzo.F64, host.ctypes.data, out.ptr, None) == 3


# ------------------------------------------------------------------------------ pathways
def test_connect_saddles_on_lj7():
    n, displacement, tol = 7, 0.02, 1e-5
    rng = np.random.default_rng(7)
    starts = dzo.DeviceArray.from_host(rng.normal(size=(48, 3 * n)) * 0.55)
    quench = dzo.BatchedLBFGS(starts, n, 0.01, 10)
    for _ in range(60):
        if quench.step(50):
            break
    energies = quench.current_objective_values
    is_minimum = quench.is_stuck & (np.abs(energies[:, None] - np.array(LJ7)[None, :]).min(axis=1) <= 1e-8)
    assert is_minimum.sum() >= 16, energies
    minima = dzo.DeviceArray.from_host(quench.current_points[is_minimum])
    batch = int(is_minimum.sum())
    search = dzo.find_saddles_hybrid(minima, n, kick=0.05, max_steps=400)
    modes = dzo.DeviceArray((batch, 3 * n), np.float64, ptr=search.ptr(dzo.HYBRIDEF_MODES), owner=False)
    before = minima.to_host()
    paths = dzo.connect_saddles(minima, modes, n, displacement, tol, max_steps=4000)
    assert _same_bits(minima.to_host(), before)              # the saddles are not moved
    saddle = (search.status == dzo.HYBRIDEF_CONVERGED) & (search.eigenvalues < -1e-4)
    print("%d of %d searches on saddles, %d distinct minima below them, edges %s" % (saddle.sum(), batch, len(paths.minimum_energies), paths.edges.tolist()))
    assert paths.edges.shape == (batch, 2) and paths.edges.dtype == np.int32 and paths.barriers.shape == (batch, 2)
    assert _same_bits(paths.saddle_energies, dzo.pairwise_batch_energy_gradient(minima, n))
    ok = paths.edges >= 0
    for b in np.flatnonzero(saddle):
        assert ok[b].all(), (b, paths.edges[b])
        assert np.all(paths.minimum_energies[paths.edges[b]] < paths.saddle_energies[b]), (b, paths.minimum_energies[paths.edges[b]], paths.saddle_energies[b])
    want = paths.saddle_energies[:, None] - paths.minimum_energies[np.where(ok, paths.edges, 0)]
    assert np.array_equal(paths.barriers[ok], want[ok]) and np.isnan(paths.barriers[~ok]).all()
    assert np.array_equal(paths.degenerate, ok[:, 0] & (paths.edges[:, 0] == paths.edges[:, 1]))
    # the twin's classification of the downloaded ends
    ends = paths.ends.to_host()
    prints, _ = st.fingerprints(ends, n, np.float64)
    prints[~paths.end_stuck, 0] = np.nan
    labels, reps = st.classify(prints, tol)
    position = {int(r): i for i, r in enumerate(reps)}
    twin_edges = np.array([[position.get(int(labels[side * batch + b]), -1) for side in range(2)] for b in range(batch)])
    assert np.array_equal(paths.edges, twin_edges)
    assert _same_bits(paths.minima.to_host(), ends[reps])
    for e in paths.minimum_energies:
        assert np.abs(e - np.array(LJ7)).min() <= 1e-8, (e, LJ7)
    assert len(paths.triples()) == int(ok.all(axis=1).sum())
