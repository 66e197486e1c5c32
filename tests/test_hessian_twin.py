"""The CPU twin of the batched Hessian kernels (tests/hessian_twin.py) against things it does not depend on, and the spectra of the
fixtures that tests/test_gpu_hessian_batch.py relies on.  No GPU, no library call."""
import numpy as np
import pytest

import hessian_twin as ht
import pairwise_twin as tw

LD = np.longdouble
U = {np.dtype(np.float64): LD(2.0) ** -53, np.dtype(np.float32): LD(2.0) ** -24}
DTYPES = [np.float64, np.float32]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_values(a, b):
    """== with the sign of a zero free; NaN never equal."""
    return bool(np.all(np.asarray(a) == np.asarray(b)))


def _small(n, dtype, seed):
    xyz = tw.jittered(tw.icosahedron13(), seed)
    return tuple(np.asarray(a[:n], dtype=dtype).astype(np.float64) for a in xyz)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_exact_twin_is_the_pair_twin_at_two_particles(dtype):
    rng = np.random.default_rng(20)
    for k in range(50):
        r2 = np.exp(rng.uniform(np.log(0.6), np.log(16.0)))
        d = rng.normal(size=3); d *= np.sqrt(r2) / np.linalg.norm(d)
        p0 = rng.uniform(-1, 1, size=3)
        p0, p1 = np.asarray(p0, dtype), np.asarray(p0 + d, dtype)
        u0, u1 = np.asarray(rng.normal(size=3), dtype), np.asarray(rng.normal(size=3), dtype)
        want = np.array(tw.pair_hvp(p0, p1, u0, u1, dtype), dtype=dtype).T          # [component, particle]
        cols = [np.array([p0[c], p1[c]]) for c in range(3)] + [np.array([u0[c], u1[c]]) for c in range(3)]
        got = ht.hvp_bits(*cols, dtype)
        assert np.array_equal(_bits(got), _bits(want)), (k, got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3, 4, 13])
def test_bit_exact_twin_within_the_derived_bound_of_the_longdouble_sums(n, dtype):
    """(N + 32) u S_i, the bound of tests/test_gpu_pairwise.py: any order of N terms, ~32 u per term."""
    x, y, z = _small(n, dtype, seed=n)
    u, v, w = (np.asarray(a, dtype=dtype).astype(np.float64) for a in np.random.default_rng(1000 + n).normal(size=(3, n)))
    got = ht.hvp_bits(x, y, z, u, v, w, dtype)
    exact, S, _ = tw.hvp(x, y, z, u, v, w)
    bound = LD(n + 32) * U[np.dtype(dtype)] * S[None, :]
    err = np.abs(got.astype(LD) - exact)
    print(f"N={n} {np.dtype(dtype).name}: worst error / bound = {float(np.max(err / bound)):.4f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [2, 3, 5])
def test_twin_hessian_columns_are_twin_products_of_unit_vectors(n, dtype):
    x, y, z = _small(n, dtype, seed=10 + n)
    H = ht.hessian_bits(x, y, z, dtype)
    for c in range(3 * n):
        e = np.zeros(3 * n); e[c] = 1.0
        col = ht.hvp_bits(x, y, z, e[:n], e[n:2 * n], e[2 * n:], dtype).reshape(-1)
        assert _same_values(H[:, c], col), (c, H[:, c], col)
    H64 = ht.hessian_f64(np.concatenate([x, y, z]))
    assert np.array_equal(H64, H64.T)
    assert np.abs(H.astype(np.float64) - H64).max() <= 64 * float(U[np.dtype(dtype)]) * np.abs(H64).max()


def test_dense_fp64_hessian_is_the_derivative_of_the_gradient():
    """Central differences of tw.gradient_f64 (step h: truncation ~ h^2 |g'''|, rounding ~ u |g| / h)."""
    p = np.concatenate(tw.jittered(tw.icosahedron13(), 5))
    H = ht.hessian_f64(p)
    h = 1e-5
    for c in range(0, p.size, 7):
        e = np.zeros(p.size); e[c] = h
        fd = (tw.gradient_f64(p + e) - tw.gradient_f64(p - e)) / (2 * h)
        assert np.abs(fd - H[:, c]).max() <= 1e-6 * np.abs(H).max(), c


def test_polished_minima_and_the_square():
    for gen, energy in ((tw.icosahedron13, -44.326801419534), (tw.octahedron38, -173.928426590629)):
        p = ht.polished_minimum(gen)
        assert abs(tw.energy_f64(p) - energy) <= 1e-11, tw.energy_f64(p)
        assert np.abs(tw.gradient_f64(p)).max() <= 6e-14
    p = ht.square4()
    assert p[1] == 1.1126198391757889 and np.abs(tw.gradient_f64(p)).max() <= 1e-13
    assert not p[8:].any()                                   # planar


# fixture -> (zero modes fp64, zero modes fp32, negative eigenvalues, the first eigenvalues above the zero modes, lambda_max)
SPECTRA = {
    "ico13": (1.1e-13, 2.2e-6, [], [42.654], 592.74),
    "oct38": (1.1e-13, 1.5e-6, [], [10.005], 521.31),
    "square4": (2e-14, 4.5e-6, [-7.8628, -2.2182], [130.30, 135.95, 135.95, 138.16], 138.16),
}


def fixture_point(name):
    return {"ico13": lambda: ht.polished_minimum(tw.icosahedron13), "oct38": lambda: ht.polished_minimum(tw.octahedron38),
            "square4": ht.square4}[name]()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(SPECTRA))
def test_fixture_spectra(name, dtype):
    """The spectra the GPU tests rely on, of the inputs rounded to the element type.  The six zero modes are zero in exact
    arithmetic only: in fp32 they carry the rounding of the coordinates, in fp64 they are the eigen-solver's own rounding
    (a few 1e-14 ... 1e-13 with numpy's eigvalsh on the exactly symmetric fp64 Hessian; of the order 3N 2^-53 lambda_max at the
    worst).  What the GPU tests need is the last assertion: with their zero_tol every zero mode is below zero_tol / 10 and every
    other eigenvalue beyond 10 zero_tol."""
    zero64, zero32, negatives, stiff, lam_max = SPECTRA[name]
    ev = ht.spectrum_of(fixture_point(name), dtype)
    k = len(negatives)
    zeros, rest = ev[k:k + 6], np.concatenate([ev[:k], ev[k + 6:]])
    print(f"{name} {np.dtype(dtype).name}: zero modes <= {np.abs(zeros).max():.3e}, then {ev[k + 6]:.6f}, lambda_max {ev[-1]:.6f}")
    assert np.abs(zeros).max() <= (zero64 if np.dtype(dtype) == np.float64 else zero32)
    assert np.allclose(ev[:k], negatives, rtol=0, atol=1e-4)
    assert np.allclose(ev[k + 6:k + 6 + len(stiff)], stiff, rtol=0, atol=5e-3)
    assert abs(ev[-1] - lam_max) <= 5e-3
    tol = ht.zero_tolerance(dtype, ev[-1])
    assert np.abs(zeros).max() < tol / 10 and np.abs(rest).min() > 10 * tol
