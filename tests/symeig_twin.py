"""CPU twin of the batched symmetric eigensolver (csrc/dzo_symeig.hip; the block "Batched symmetric eigensolver" of
include/dzo.h is the specification): two-sided cyclic Jacobi in the round-robin ordering, every operation in the element type
with one rounding -- numpy arrays and scalars of that dtype -- and the two norms in fp64 in the device's order.  A helper module
for tests/test_symeig_twin.py (which checks it against numpy.linalg) and tests/test_gpu_symeig.py (which checks the kernels
against it bit for bit).  Not a conftest, no fixtures.

The round-robin list is kept literally as the header words it; the kernel uses a closed form of it.
"""
import functools

import numpy as np

import hessian_twin as ht
import pairwise_twin as tw

DEFAULT_SWEEPS = 30
_XOR_TREE = (32, 16, 8, 4, 2, 1)


def norm_sum(sq):
    """The sum of the (n, n) fp64 array ``sq[r, c]`` in the order of the norms: thread (w, l) adds columns w, w + 4, ... (outer)
    and rows l, l + 64, ... (inner) from +0, the xor tree over the 64 lanes of a wave, the four waves in order from +0."""
    n = sq.shape[0]
    rb, cb = -(-n // 64), -(-n // 4)
    pad = np.zeros((rb * 64, cb * 4), dtype=np.float64)      # a missing element adds +0: exact
    pad[:n, :n] = sq
    cells = pad.reshape(rb, 64, cb, 4)
    acc = np.zeros((64, 4), dtype=np.float64)
    for c in range(cb):
        for r in range(rb):
            acc = acc + cells[r, :, c, :]
    lanes = np.arange(64)
    for offset in _XOR_TREE:
        acc = acc + acc[lanes ^ offset, :]
    total = np.float64(0)
    for w in range(4):
        total = total + acc[0, w]
    return total


def round_pairs(n):
    """The rounds of one sweep: a list of m - 1 pairs of index arrays (p, q), p < q, the dropped pair left out."""
    m = n + (n & 1)
    idx = list(range(m))
    rounds = []
    for _ in range(m - 1):
        pairs = [(idx[k], idx[m - 1 - k]) for k in range(m // 2)]
        pairs = [(min(i, j), max(i, j)) for i, j in pairs if i != n and j != n]
        rounds.append((np.array([p for p, _ in pairs], dtype=np.intp), np.array([q for _, q in pairs], dtype=np.intp)))
        idx = [idx[0], idx[m - 1]] + idx[1:m - 1]
    assert idx == list(range(m))                             # which is why resetting the list between sweeps changes nothing
    return rounds


def jacobi(A, dtype, vectors=True, max_sweeps=0):
    """``(eigenvalues (n,), V (n, n) with V[:, k] the vector of eigenvalue k, or None, sweeps)`` of the symmetric part of
    ``A[r, c]``, as the device computes them."""
    dt = np.dtype(dtype)
    t = dt.type
    A = np.asarray(A, dtype=dt)
    n = A.shape[0]
    assert A.shape == (n, n)
    limit = DEFAULT_SWEEPS if max_sweeps <= 0 else int(max_sweeps)
    eps = np.float64(np.finfo(dt).eps)
    one, zero = t(1), t(0)
    with np.errstate(all="ignore"):
        a = t(0.5) * (A + A.T)
        V = np.eye(n, dtype=dt) if vectors else None
        a64 = a.astype(np.float64)
        threshold = eps * np.sqrt(norm_sum(a64 * a64))
        rounds = round_pairs(n)
        offdiag = ~np.eye(n, dtype=bool)
        sweeps = 0
        while True:
            a64 = a.astype(np.float64)
            off = np.sqrt(norm_sum(np.where(offdiag, a64 * a64, 0.0)))
            if off <= threshold and threshold < np.inf:
                verdict = sweeps
                break
            if sweeps == limit:
                verdict = -1
                break
            for p, q in rounds:
                if len(p) == 0:
                    continue
                apq, app, aqq = a[p, q], a[p, p], a[q, q]
                tau = (aqq - app) / (apq + apq)
                tt = np.copysign(one, tau) / (np.abs(tau) + np.sqrt(one + tau * tau))
                cc = one / np.sqrt(one + tt * tt)
                ss = tt * cc
                c = np.where(apq == zero, one, cc).astype(dt)
                s = np.where(apq == zero, zero, ss).astype(dt)
                x, y = a[:, p], a[:, q]                      # fancy indexing copies: the old columns
                a[:, p] = c * x - s * y
                a[:, q] = s * x + c * y
                if vectors:
                    x, y = V[:, p], V[:, q]
                    V[:, p] = c * x - s * y
                    V[:, q] = s * x + c * y
                x, y = a[p, :], a[q, :]
                a[p, :] = c[:, None] * x - s[:, None] * y
                a[q, :] = s[:, None] * x + c[:, None] * y
                a[p, q] = zero
                a[q, p] = zero
            sweeps += 1
        d = np.diagonal(a).copy()
        k = np.arange(n)
        rank = (d[None, :] < d[:, None]).sum(axis=1) + ((d[None, :] == d[:, None]) & (k[None, :] < k[:, None])).sum(axis=1)
        w = np.zeros(n, dtype=dt)
        w[rank] = d                                          # (NaN: ranks coincide and the values are unspecified)
        if vectors:
            Vs = np.zeros_like(V)
            Vs[:, rank] = V
            V = Vs
    return w, V, verdict


# ------------------------------------------------------------------------------ the matrices the tests use
def random_symmetric(n, seed):
    """Seeded, entries in [-1, 1), exactly symmetric in fp64 (and so in fp32 after rounding)."""
    g = np.random.default_rng([seed, n]).uniform(-1.0, 1.0, size=(n, n))
    return np.triu(g) + np.triu(g, 1).T


def random_general(n, seed):
    """A NON-symmetric matrix whose entries are multiples of 2^-20 in [-1, 1): the sums A + A^T are exact in both dtypes."""
    return np.random.default_rng([seed, n, 7]).integers(-(1 << 20), 1 << 20, size=(n, n)).astype(np.float64) / (1 << 20)


def special_matrices():
    """{name: matrix}: the fixed small cases."""
    tiny = 1e-30
    return {
        "diagonal5": np.diag([3.0, -1.0, 2.0, -4.0, 0.5]),   # unsorted: 0 sweeps, V a permutation
        "zeros5": np.zeros((5, 5)),
        "ones5": np.ones((5, 5)),                            # rank one: eigenvalues 0 (four times) and 5
        "equal_diagonal2": np.array([[2.0, 0.75], [0.75, 2.0]]),           # tau = 0: the 45 degree rotation
        "tiny_offdiagonal2": np.array([[1.0, tiny], [tiny, 3.0]]),         # tau = 1e30: tau * tau overflows in fp32
        # the same quotient inside a sweep that the other entries force
        "tiny_offdiagonal3": np.array([[1.0, tiny, 0.5], [tiny, 3.0, 0.25], [0.5, 0.25, 2.0]]),
    }


@functools.lru_cache(maxsize=None)
def lj_hessian(name):
    """The fp64 Hessians of the three Lennard-Jones fixtures of hessian_twin.py: 'lj13', 'lj38' (polished minima), 'square4'
    (Morse index 2)."""
    p = {"lj13": lambda: ht.polished_minimum(tw.icosahedron13), "lj38": lambda: ht.polished_minimum(tw.octahedron38),
         "square4": ht.square4}[name]()
    h = ht.hessian_f64(p)
    h.setflags(write=False)
    return h


SIZES = (1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 64, 65, 113, 114)
LJ_NAMES = ("lj13", "lj38", "square4")


def lds_edge(dtype, plan):
    """(last n on LDS storage, first n on memory storage) by ``plan(n, dtype) -> (storage, ld, lds_bytes)``."""
    first = next(n for n in range(1, 385) if plan(n, dtype)[0] != 0)
    return first - 1, first


# the edges dzo_symeig_plan gives (tests/test_symeig_build.py checks them against the library): n on LDS up to here
LDS_LAST = {np.dtype(np.float64): 141, np.dtype(np.float32): 201}


def case_list(dtype):
    """[(name, matrix as fp64 (n, n))] of every matrix of the GPU tests for this dtype, batch-1 giant last."""
    last = LDS_LAST[np.dtype(dtype)]
    cases = [("random%d" % n, random_symmetric(n, 1)) for n in SIZES + (last, last + 1)]
    cases += list(special_matrices().items())
    cases += [("general%d" % n, random_general(n, 2)) for n in (4, 33)]
    cases += [(name, lj_hessian(name)) for name in LJ_NAMES]
    cases.append(("random384", random_symmetric(384, 1)))
    return cases


@functools.lru_cache(maxsize=None)
def twin_result(name, dtype_name, vectors=True, max_sweeps=0):
    """``jacobi`` of a named case, computed once per session and shared (the arrays are read-only)."""
    dt = np.dtype(dtype_name)
    A = dict(case_list(dt))[name]
    w, V, sweeps = jacobi(np.asarray(A, dtype=dt), dt, vectors=vectors, max_sweeps=max_sweeps)
    w.setflags(write=False)
    if V is not None:
        V.setflags(write=False)
    return w, V, sweeps


# ------------------------------------------------------------------------------ the bounds of the issue
def bounds_report(A_t, w, V):
    """(eigenvalue error, its bound, residual, its bound, orthogonality, its bound) of a result (w, V) for the matrix ``A_t``
    already rounded to the element type; everything measured in fp64.  V may be None (then the last four are 0)."""
    dt = A_t.dtype
    eps = float(np.finfo(dt).eps)
    n = A_t.shape[0]
    S = (dt.type(0.5) * (A_t + A_t.T)).astype(np.float64)    # the fp64 copy of the symmetrised T matrix
    F = float(np.linalg.norm(S))
    ref = np.linalg.eigvalsh(S)
    w64 = np.asarray(w, dtype=np.float64)
    ev = float(np.max(np.abs(w64 - ref)))
    if V is None:
        return ev, 2 * (n + 4) * eps * F, 0.0, 0.0, 0.0, 0.0
    V64 = np.asarray(V, dtype=np.float64)
    res = float(np.linalg.norm(S @ V64 - V64 * w64[None, :]))
    orth = float(np.linalg.norm(V64.T @ V64 - np.eye(n)))
    return ev, 2 * (n + 4) * eps * F, res, 4 * (n + 4) * eps * F, orth, 4 * n ** 1.5 * eps


def assert_bounds(label, A_t, w, V):
    ev, ev_b, res, res_b, orth, orth_b = bounds_report(A_t, w, V)
    print("%s: eigenvalues %.3e <= %.3e, residual %.3e <= %.3e, orthogonality %.3e <= %.3e" % (label, ev, ev_b, res, res_b, orth, orth_b))
    assert ev <= ev_b, (label, "eigenvalues", ev, ev_b)
    assert res <= res_b, (label, "residual", res, res_b)
    assert orth <= orth_b, (label, "orthogonality", orth, orth_b)
