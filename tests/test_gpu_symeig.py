"""The batched symmetric eigensolver on the device (csrc/dzo_symeig.hip) against its CPU twin (tests/symeig_twin.py) and
against numpy.linalg.

1. bit for bit against the twin -- eigenvalues, sweeps and vectors, both dtypes -- at n = 1 .. 114, at the last size on LDS
   storage and the first on memory storage (read from dzo_symeig_plan), at n = 384, on the structured small cases, on a
   non-symmetric matrix and on the three Lennard-Jones Hessians;
2. the three bounds of tests/test_symeig_twin.py for the device results themselves;
3. physics: Morse indices of the fixtures, agreement with hessian_eigenvalues, the tempering -> quench -> hessian_spectrum
   hand-over;
4. independence: an instance's bits alone and anywhere in a mixed batch, with and without vectors and sweeps_dev; the input
   bytes stay as they were on both storages;
5. the sweep limit and a NaN;
6. error codes;
7. the plain-C example.
"""
import functools
import subprocess

import numpy as np
import pytest

import hessian_twin as ht
import pairwise_twin as tw
import symeig_twin as st
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
CANARY = 12345.0
GUARD = 64
CASE_NAMES = {d: [name for name, _ in st.case_list(np.dtype(d))] for d in DTYPES}
ALL_CASES = [(d, name) for d in DTYPES for name in CASE_NAMES[d]]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _device_eigen(mats, dtype, vectors=True, max_sweeps=0, want_sweeps=True):
    """The device call on a list of (n, n) host matrices A[r, c] of one size, with canaries around every output and a check
    that the input bytes did not change.  Returns (w (batch, n), V (batch, n, n) with V[b][:, k] the vector of eigenvalue k,
    or None, sweeps (batch,) or None)."""
    dt = np.dtype(dtype)
    n, batch = mats[0].shape[0], len(mats)
    host = np.ascontiguousarray(np.stack([np.asarray(A, dtype=dt).T for A in mats]))         # [b, c, r]
    dev = dzo.DeviceArray.from_host(host)

    def guarded(size, np_dtype):
        buf = dzo.DeviceArray.from_host(np.full(size + 2 * GUARD, CANARY, dtype=np_dtype))
        return buf, buf.view(GUARD, size)

    wbuf, w = guarded(batch * n, dt)
    vbuf, v = guarded(batch * n * n, dt) if vectors else (None, None)
    sbuf, s = guarded(batch, np.int32) if want_sweeps else (None, None)
    rc = dzo.lib().dzo_symmetric_batch_eigen(n, batch, dzo._dt(dt), dev.ptr, w.ptr, v.ptr if vectors else None,
                                             s.ptr if want_sweeps else None, max_sweeps)
    assert rc == 0, dzo.lib().dzo_last_error()
    for buf in (wbuf, vbuf, sbuf):
        if buf is not None:
            h = buf.to_host()
            assert np.all(h[:GUARD] == h.dtype.type(CANARY)) and np.all(h[-GUARD:] == h.dtype.type(CANARY)), "wrote outside its output"
    assert _same_bits(dev.to_host().reshape(host.shape), host), "the input matrices were modified"
    V = np.ascontiguousarray(v.to_host().reshape(batch, n, n).transpose(0, 2, 1)) if vectors else None
    return w.to_host().reshape(batch, n), V, (s.to_host().reshape(batch) if want_sweeps else None)


def _case(dtype, name):
    return np.asarray(dict(st.case_list(np.dtype(dtype)))[name], dtype=np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _device_case(dtype, name):
    """The device's (w, V, sweeps) of a named case, batch 1 with vectors: computed once, shared by items 1 and 2."""
    return _device_eigen([_case(dtype, name)], dtype)


# ------------------------------------------------------------------------------ 1. bit for bit, and 2. the bounds
def test_the_case_list_sits_on_the_edges_of_the_plan():
    for d in DTYPES:
        last, first = st.lds_edge(np.dtype(d), dzo.symeig_plan)
        assert last == st.LDS_LAST[np.dtype(d)] and first == last + 1
        assert "random%d" % last in CASE_NAMES[d] and "random%d" % first in CASE_NAMES[d] and "random384" in CASE_NAMES[d]
        assert dzo.symeig_plan(last, d)[0] == dzo.SYMEIG_STORAGE_LDS and dzo.symeig_plan(first, d)[0] == dzo.SYMEIG_STORAGE_MEMORY
        assert dzo.symeig_plan(384, d)[0] == dzo.SYMEIG_STORAGE_MEMORY


@pytest.mark.parametrize("dtype,name", ALL_CASES)
def test_bit_for_bit_against_the_twin(dtype, name):
    A = _case(dtype, name)
    w, V, sweeps = _device_case(dtype, name)
    tw_w, tw_V, tw_sweeps = st.twin_result(name, dtype)
    print(name, dtype, "sweeps", sweeps[0], "twin", tw_sweeps)
    assert sweeps[0] == tw_sweeps
    assert _same_bits(w[0], tw_w), (np.flatnonzero(_bits(w[0]) != _bits(tw_w))[:5], w[0][:4], tw_w[:4])
    assert _same_bits(V[0], tw_V), np.argwhere(_bits(V[0]) != _bits(tw_V))[:5].tolist()
    w2, V2, sweeps2 = _device_eigen([A], dtype, vectors=False)
    assert V2 is None and _same_bits(w2, w) and sweeps2[0] == sweeps[0]


@pytest.mark.parametrize("dtype,name", ALL_CASES)
def test_device_results_meet_the_bounds(dtype, name):
    """Independent of the twin: eigenvalues against numpy.linalg.eigvalsh of the fp64 copy of the symmetrised T matrix within
    2 (n + 4) eps F, the residual within 4 (n + 4) eps F, the orthogonality within 4 n^1.5 eps, at most 30 sweeps."""
    A = _case(dtype, name)
    w, V, sweeps = _device_case(dtype, name)
    assert 0 <= sweeps[0] <= 30
    assert np.all(np.diff(w[0]) >= 0)
    st.assert_bounds("%s %s (%d sweeps)" % (name, dtype, sweeps[0]), A, w[0], V[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_structured_cases_on_the_device(dtype):
    dt = np.dtype(dtype)
    w, V, sweeps = _device_eigen([_case(dtype, "diagonal5"), _case(dtype, "zeros5")], dtype)
    assert sweeps.tolist() == [0, 0]
    assert w[0].tolist() == [-4.0, -1.0, 0.5, 2.0, 3.0] and not w[1].any()
    perm = np.zeros((5, 5), dtype=dt)
    perm[[3, 1, 4, 2, 0], np.arange(5)] = 1                  # eigenvalue k sat at this row of the diagonal
    assert np.array_equal(V[0], perm) and np.array_equal(V[1], np.eye(5, dtype=dt))
    G = np.asarray(st.random_general(33, 2), dtype=dt)       # a non-symmetric matrix: the bits of its symmetric part given directly
    S = dt.type(0.5) * (G + G.T)
    w, V, sweeps = _device_eigen([G, S], dtype)
    assert not np.array_equal(G, G.T)
    assert _same_bits(w[0], w[1]) and _same_bits(V[0], V[1]) and sweeps[0] == sweeps[1]


# ------------------------------------------------------------------------------ 3. physics
@pytest.mark.parametrize("dtype", DTYPES)
def test_morse_indices_of_the_fixtures(dtype):
    """hessian_spectrum on the three fixtures: the known indices, and the eigenvalues hessian_eigenvalues gives within the
    eigenvalue bound (both diagonalise the device Hessian: the bound's F is its Frobenius norm)."""
    dt = np.dtype(dtype)
    eps = float(np.finfo(dt).eps)
    for make, n, index in ((lambda: ht.polished_minimum(tw.icosahedron13), 13, (0, 6)), (lambda: ht.polished_minimum(tw.octahedron38), 38, (0, 6)),
                           (ht.square4, 4, (2, 6))):
        dev = dzo.DeviceArray.from_host(np.asarray(make(), dtype=dt))
        ev = dzo.hessian_spectrum(dev, n)
        assert ev.shape == (1, 3 * n) and ev.dtype == np.float64
        old = dzo.hessian_eigenvalues(dev, n)
        tol = ht.zero_tolerance(dt, old[0, -1])
        got = tuple(int(v[0]) for v in dzo.morse_index(ev, tol))
        assert got == index, (n, got, ev[0][:8])
        assert got == tuple(int(v[0]) for v in dzo.morse_index(old, tol))
        F = np.linalg.norm(dzo.pairwise_batch_hessian(dev, n)[0].astype(np.float64))
        print(n, dtype, "max difference", np.abs(ev - old).max(), "bound", 2 * (3 * n + 4) * eps * F)
        assert np.abs(ev - old).max() <= 2 * (3 * n + 4) * eps * F
        ev2, modes = dzo.hessian_spectrum(dev, n, vectors=True)
        assert np.array_equal(ev2, ev) and modes.shape == (1, 3 * n, 3 * n) and modes.dtype == dt


@pytest.mark.parametrize("dtype", DTYPES)
def test_tempering_quench_spectrum_hand_over(dtype):
    """The device pipeline end to end on a small run: tempering -> quench -> hessian_spectrum, against hessian_eigenvalues of
    the same points within the eigenvalue bound."""
    dt = np.dtype(dtype)
    n, replicas = 13, 8
    starts = np.asarray([np.concatenate(tw.jittered(tw.icosahedron13(), seed=k)) for k in range(replicas)], dtype=dt)
    pt = dzo.ParallelTempering(dzo.DeviceArray.from_host(starts.ravel()), n, np.geomspace(20.0, 5.0, replicas), [0.05] * replicas, 3.0, base_seed=5)
    pt.run(100, 2)
    _, minima, _ = pt.quench(max_steps=2000 if dt == np.float64 else 200)
    ev = dzo.hessian_spectrum(minima, n)
    old = dzo.hessian_eigenvalues(minima, n)
    assert ev.shape == old.shape == (replicas, 3 * n)
    F = np.linalg.norm(dzo.pairwise_batch_hessian(minima, n).astype(np.float64), axis=(1, 2))
    bound = 2 * (3 * n + 4) * float(np.finfo(dt).eps) * F
    print(dtype, "max difference / bound", (np.abs(ev - old).max(axis=1) / bound).max())
    assert np.all(np.abs(ev - old).max(axis=1) <= bound)


# ------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [33, "memory"])
def test_an_instance_computes_the_same_bits_anywhere(n, dtype):
    """A batch of 9 whose instances converge after different numbers of sweeps: a diagonal matrix (0), the rank-one matrix
    (1), random matrices, a nearly diagonal one.  The matrix under test alone, first, in the middle and last."""
    dt = np.dtype(dtype)
    if n == "memory":
        n = st.LDS_LAST[dt] + 1
    rng = np.random.default_rng(n)
    others = [np.diag(rng.uniform(-1, 1, n)), np.ones((n, n)), st.random_symmetric(n, 3), np.diag(rng.uniform(1, 2, n)) + 1e-6 * st.random_symmetric(n, 4),
              st.random_symmetric(n, 5) * 100.0, np.zeros((n, n)), st.random_general(n, 6), np.eye(n)]
    A = st.random_symmetric(n, 1)
    alone = _device_eigen([A], dtype)
    counts = set()
    for pos in (0, 4, 8):
        batch = others[:pos] + [A] + others[pos:]
        w, V, sweeps = _device_eigen(batch, dtype)
        counts |= set(sweeps.tolist())
        assert _same_bits(w[pos], alone[0][0]) and _same_bits(V[pos], alone[1][0]) and sweeps[pos] == alone[2][0], pos
        if pos == 4:
            w2, _, sweeps2 = _device_eigen(batch, dtype, vectors=False)
            assert _same_bits(w2, w) and np.array_equal(sweeps2, sweeps)
            w3, V3, none = _device_eigen(batch, dtype, want_sweeps=False)                 # sweeps_dev = NULL
            assert none is None and _same_bits(w3, w) and _same_bits(V3, V)
    assert len(counts) >= 3 and min(counts) == 0, counts


# ------------------------------------------------------------------------------ 5. the sweep limit
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_limit_and_nan(dtype):
    dt = np.dtype(dtype)
    R = np.asarray(st.random_symmetric(16, 1), dtype=dt)
    w, V, sweeps = _device_eigen([R], dtype, max_sweeps=1)
    assert sweeps[0] == -1
    tw_w, tw_V, tw_sweeps = st.jacobi(R, dt, max_sweeps=1)
    assert tw_sweeps == -1 and _same_bits(w[0], tw_w) and _same_bits(V[0], tw_V)       # one sweep, the same bits
    bad = R.copy()
    bad[3, 5] = np.nan
    good = _device_eigen([R, R], dtype)
    w, V, sweeps = _device_eigen([R, bad, R], dtype)                                   # returns
    assert sweeps[1] == -1 and sweeps[0] == sweeps[2] == good[2][0] >= 1
    for k in (0, 2):
        assert _same_bits(w[k], good[0][0]) and _same_bits(V[k], good[1][0])


# ------------------------------------------------------------------------------ 6. errors
def test_error_codes():
    n, batch = 5, 2
    a = dzo.DeviceArray.zeros(n * n * batch)
    w = dzo.DeviceArray.zeros(n * batch)
    v = dzo.DeviceArray.zeros(n * n * batch)
    s = dzo.DeviceArray.from_host(np.zeros(batch, dtype=np.int32))
    eig = dzo.lib().dzo_symmetric_batch_eigen
    ok = (n, batch, dzo.F64, a.ptr, w.ptr, v.ptr, s.ptr, 0)
    names = ["n", "batch", "dtype", "matrices", "eigenvalues", "eigenvectors", "sweeps", "max_sweeps"]

    def with_(**kw):
        return tuple(kw.get(k, x) for k, x in zip(names, ok))

    assert eig(*ok) == 0
    assert eig(*with_(eigenvectors=None)) == 0 and eig(*with_(sweeps=None)) == 0 and eig(*with_(max_sweeps=-3)) == 0
    assert eig(*with_(dtype=9)) == 1
    assert eig(*with_(n=0)) == 1 and eig(*with_(n=-1)) == 1
    assert eig(*with_(batch=0)) == 1 and eig(*with_(batch=(1 << 30) + 1)) == 1
    assert eig(*with_(matrices=None)) == 1 and eig(*with_(eigenvalues=None)) == 1
    assert eig(*with_(n=385, batch=1)) == 5
    assert dzo.SYMEIG_MAX_N == 384
    host = np.zeros(n * n * batch)
    hs = np.zeros(batch, dtype=np.int32)
    for name in ("matrices", "eigenvalues", "eigenvectors"):
        assert eig(*with_(**{name: host.ctypes.data})) == 3, name
    assert eig(*with_(sweeps=hs.ctypes.data)) == 3
    with pytest.raises(dzo.AssertionFailed):
        dzo.symmetric_batch_eigen(dzo.DeviceArray(n * n * batch, np.float64, ptr=host.ctypes.data, owner=False), n)
    with pytest.raises(dzo.DzoError):
        dzo.symmetric_batch_eigen(np.zeros((1, 385, 385)), 385)
    # non-finite Hessians (two coincident particles): hessian_spectrum raises
    p = np.concatenate(tw.icosahedron13())
    for c in range(3):
        p[c * 13 + 7] = p[c * 13 + 5]
    with pytest.raises(dzo.DzoError):
        dzo.hessian_spectrum(dzo.DeviceArray.from_host(p), 13)


def test_python_wrapper_takes_host_and_device_matrices():
    A = np.asarray(st.random_symmetric(17, 1))
    w, V, sweeps = dzo.symmetric_batch_eigen(np.stack([A.T, A.T]), 17, vectors=True)
    assert w.shape == (2, 17) and V.shape == (2, 17, 17) and sweeps.shape == (2,) and sweeps.dtype == np.int32
    tw_w, tw_V, tw_sweeps = st.twin_result("random17", "float64")
    assert _same_bits(w[1], tw_w) and _same_bits(np.ascontiguousarray(V[1].T), tw_V) and sweeps.tolist() == [tw_sweeps] * 2
    w2, none, _ = dzo.symmetric_batch_eigen(dzo.DeviceArray.from_host(np.stack([A.T, A.T])), 17)
    assert none is None and _same_bits(w2, w)


# ------------------------------------------------------------------------------ 7. the plain-C example
def test_lj_spectrum_example_runs(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_spectrum")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("instance")]
    assert len(rows) >= 2
    for row in rows:                                         # "instance k: index I zeros Z sweeps S ..."
        assert row[2:6] == ["index", "0", "zeros", "6"], row
