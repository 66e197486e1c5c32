"""The CPU twin of the batched symmetric eigensolver (tests/symeig_twin.py) against things it does not depend on:
numpy.linalg.eigvalsh of the fp64 copy of the symmetrised matrix, the eigenvector residual and orthogonality, on every matrix
the GPU tests use (tests/test_gpu_symeig.py compares the kernels with the twin bit for bit, so what holds for the twin here
holds for them).  With eps = finfo(T).eps and F the Frobenius norm of the symmetrised matrix:

    max |lambda - lambda_ref| <= 2 (n + 4) eps F,   |A V - V Lambda|_F <= 4 (n + 4) eps F,   |V^T V - I|_F <= 4 n^1.5 eps,

and at most 30 sweeps.  No GPU here."""
import numpy as np
import pytest

import symeig_twin as st

DTYPES = ("float64", "float32")


@pytest.mark.parametrize("dtype", DTYPES)
def test_twin_meets_the_bounds_on_every_matrix_of_the_gpu_tests(dtype):
    dt = np.dtype(dtype)
    worst = 0
    for name, A in st.case_list(dt):
        A_t = np.asarray(A, dtype=dt)
        w, V, sweeps = st.twin_result(name, dtype)
        assert 0 <= sweeps <= 30, (name, sweeps)
        worst = max(worst, sweeps)
        assert np.all(np.diff(w) >= 0), name
        st.assert_bounds("%s %s (%d sweeps)" % (name, dtype, sweeps), A_t, w, V)
    print("most sweeps:", worst)


def test_round_robin_meets_every_pair_once_per_sweep():
    for n in (1, 2, 3, 4, 5, 16, 17, 114):
        rounds = st.round_pairs(n)
        m = n + (n & 1)
        assert len(rounds) == m - 1
        seen = set()
        for p, q in rounds:
            assert np.all(p < q) and np.all(q < n)
            both = np.concatenate([p, q])
            assert len(set(both.tolist())) == len(both)      # disjoint within a round
            seen |= set(zip(p.tolist(), q.tolist()))
        assert seen == {(i, j) for i in range(n) for j in range(i + 1, n)}


def test_norm_order_is_a_plain_sum_up_to_rounding_and_exact_on_integers():
    rng = np.random.default_rng(5)
    for n in (1, 5, 64, 65, 114):
        sq = rng.integers(0, 1000, size=(n, n)).astype(np.float64)
        assert st.norm_sum(sq) == sq.sum()                   # integers: every order gives the same bits
        sq = rng.uniform(0, 1, size=(n, n))
        assert abs(st.norm_sum(sq) - sq.sum()) <= 1e-12 * sq.sum()


@pytest.mark.parametrize("dtype", DTYPES)
def test_structured_cases(dtype):
    dt = np.dtype(dtype)
    special = st.special_matrices()
    w, V, sweeps = st.twin_result("diagonal5", dtype)
    assert sweeps == 0 and w.tolist() == [-4.0, -1.0, 0.5, 2.0, 3.0]
    assert sorted(map(tuple, V.T.tolist())) == sorted(map(tuple, np.eye(5).tolist())) and V[3, 0] == 1 and V[0, 4] == 1
    w, V, sweeps = st.twin_result("zeros5", dtype)
    assert sweeps == 0 and not w.any() and np.array_equal(V, np.eye(5, dtype=dt))
    w, V, sweeps = st.twin_result("ones5", dtype)
    assert sweeps >= 1 and abs(w[-1] - 5) <= 16 * np.finfo(dt).eps * 5 and np.all(np.abs(w[:4]) <= 16 * np.finfo(dt).eps * 5)
    w, V, sweeps = st.twin_result("equal_diagonal2", dtype)
    assert sweeps == 1 and np.allclose(w, [1.25, 2.75], rtol=4 * np.finfo(dt).eps) and np.allclose(np.abs(V), np.sqrt(0.5), rtol=4 * np.finfo(dt).eps)
    w, V, sweeps = st.twin_result("tiny_offdiagonal2", dtype)
    assert sweeps == 0 and w.tolist() == [1.0, 3.0]
    w, V, sweeps = st.twin_result("tiny_offdiagonal3", dtype)
    assert 1 <= sweeps <= 30 and np.all(np.isfinite(w)) and np.all(np.isfinite(V))
    assert special["tiny_offdiagonal3"][0, 1] == 1e-30


@pytest.mark.parametrize("dtype", DTYPES)
def test_symmetric_part_vectors_flag_sweep_limit_and_nan(dtype):
    dt = np.dtype(dtype)
    G = np.asarray(st.random_general(33, 2), dtype=dt)
    assert not np.array_equal(G, G.T)
    S = dt.type(0.5) * (G + G.T)
    a, b = st.jacobi(G, dt), st.jacobi(S, dt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    c = st.jacobi(G, dt, vectors=False)
    assert np.array_equal(a[0], c[0]) and c[1] is None and a[2] == c[2]
    R = np.asarray(st.random_symmetric(16, 1), dtype=dt)
    assert st.jacobi(R, dt, max_sweeps=1)[2] == -1
    R[3, 5] = np.nan
    assert st.jacobi(R, dt, max_sweeps=4)[2] == -1


def test_lj_fixtures_have_the_known_morse_indices():
    import hessian_twin as ht
    for name, expect in (("lj13", (0, 6)), ("lj38", (0, 6)), ("square4", (2, 6))):
        for dtype in DTYPES:
            w, _, _ = st.twin_result(name, dtype)
            w = w.astype(np.float64)
            tol = ht.zero_tolerance(dtype, w.max())
            assert (int((w < -tol).sum()), int((np.abs(w) <= tol).sum())) == expect, (name, dtype, w[:8])
