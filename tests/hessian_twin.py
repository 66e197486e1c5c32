"""CPU twin of the batched Hessian-vector product and the dense Hessian of a Lennard-Jones cluster (csrc/dzo_hessian_batch.hip;
src/ExampleFunctions.jl:367-468 with the radial functions of :16-72).  A helper module for tests/test_hessian_twin.py (which
checks it against things it does not depend on) and tests/test_gpu_hessian_batch.py (which checks the device kernels against
it).  Not a conftest, no fixtures.

Three levels:

* ``hvp_bits`` / ``hessian_bits``: the device's operations one by one in the element type, every operation rounded once, the
  radial functions with the exact fused multiply-add of pairwise_twin.py, row sums over j = 0 .. N-1 sequentially from +0.  What
  a correct kernel must reproduce bit for bit.  Python loops: for small N.
* ``hessian_f64``: the dense Hessian from the formulas in vectorised fp64, H = sum over pairs of 2 e' (delta_ab) + 4 e'' d_a d_b
  blocks.  The reference of the spectra.
* fixtures whose spectra the GPU tests rely on: the two polished minima and the planar LJ4 square, a saddle of index 2.
"""
import functools

import numpy as np

import pairwise_twin as tw


# ------------------------------------------------------------------------------ bit-exact forms
def _pair_terms(t, dtype, d, du):
    """(f du_a + g d_a for a = x, y, z) of one pair, :395-419, every operation rounded once to ``dtype``."""
    with np.errstate(all="ignore"):
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        f = t(tw.lj_first_derivative(r2, dtype))
        s = t(tw.lj_second_derivative(r2, dtype))
        overlap = d[0] * du[0] + d[1] * du[1] + d[2] * du[2]
        os_ = overlap * s
        g = os_ + os_
        return [f * du[a] + g * d[a] for a in range(3)]


def hvp_bits(x, y, z, u, v, w, dtype):
    """The product as the device computes it: array (3, N) of ``dtype``."""
    t = np.dtype(dtype).type
    P = [[t(c) for c in a] for a in (x, y, z)]
    U = [[t(c) for c in a] for a in (u, v, w)]
    n = len(P[0])
    out = np.zeros((3, n), dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = [t(0), t(0), t(0)]
            for j in range(n):
                if j == i:
                    continue                                # the dropped self term adds f = s = 0: an exact zero
                term = _pair_terms(t, dtype, [P[a][i] - P[a][j] for a in range(3)], [U[a][i] - U[a][j] for a in range(3)])
                acc = [acc[a] + term[a] for a in range(3)]
            for a in range(3):
                out[a, i] = acc[a] + acc[a]
    return out


def hessian_bits(x, y, z, dtype):
    """The dense Hessian as the device assembles it, H[r, c] with r = a N + i, c = b N + j: an off-diagonal block is the single
    term with du = -e_b, the diagonal block the sequential sum over j of the terms with du = +e_b; both doubled once."""
    t = np.dtype(dtype).type
    P = [[t(c) for c in a] for a in (x, y, z)]
    n = len(P[0])
    H = np.zeros((3 * n, 3 * n), dtype=dtype)
    unit = [[t(1) if a == b else t(0) for a in range(3)] for b in range(3)]
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = [[t(0)] * 3 for _ in range(3)]
            for j in range(n):
                if j == i:
                    continue
                d = [P[a][i] - P[a][j] for a in range(3)]
                for b in range(3):
                    minus = _pair_terms(t, dtype, d, [t(0) - unit[b][a] for a in range(3)])
                    plus = _pair_terms(t, dtype, d, [unit[b][a] - t(0) for a in range(3)])
                    for a in range(3):
                        H[a * n + i, b * n + j] = (t(0) + minus[a]) + (t(0) + minus[a])
                        acc[b][a] = acc[b][a] + plus[a]
            for b in range(3):
                for a in range(3):
                    H[a * n + i, b * n + i] = acc[b][a] + acc[b][a]
    return H


# ------------------------------------------------------------------------------ fp64, from the formulas
def hessian_f64(p):
    """Dense Hessian (3N, 3N) of the point p = [x | y | z] in fp64: block (i, j != i) = -(2 e' delta_ab + 4 e'' d_a d_b), block
    (i, i) = minus the sum of the others of its row."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p) // 3
    c = p.reshape(3, n)
    d = c[:, :, None] - c[:, None, :]                       # d[a, i, j]
    r2 = (d * d).sum(axis=0)
    np.fill_diagonal(r2, 1.0)
    inv_r2 = 1.0 / r2
    inv_r4 = inv_r2 * inv_r2
    inv_r6 = inv_r4 * inv_r2
    inv_r8 = inv_r4 * inv_r4
    f = -12.0 * (inv_r8 * (inv_r6 + inv_r6) - inv_r8)
    s = 48.0 * (3.5 * (inv_r8 * inv_r8) - inv_r8 * inv_r2)
    np.fill_diagonal(f, 0.0)
    np.fill_diagonal(s, 0.0)
    H = np.zeros((3, n, 3, n))
    for a in range(3):
        for b in range(3):
            blk = 4.0 * s * (d[a] * d[b]) + (2.0 * f if a == b else 0.0)
            H[a, :, b, :] = -blk
            H[a, np.arange(n), b, np.arange(n)] = blk.sum(axis=1)
    return H.reshape(3 * n, 3 * n)


def spectrum_of(p, dtype=np.float64):
    """Ascending fp64 eigenvalues of the Hessian at p rounded to ``dtype`` (what the device is given)."""
    q = np.asarray(p, dtype=dtype).astype(np.float64)
    h = hessian_f64(q)
    return np.linalg.eigvalsh(0.5 * (h + h.T))


# ------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def polished_minimum(gen):
    """The local minimum next to ``tw.icosahedron13`` / ``tw.octahedron38`` (``gen`` is that function) as a point [x | y | z]:
    30 Newton steps with the pseudo-inverse of the Hessian (eigenvalues below 1e-6 lambda_max dropped: the six rigid-body
    modes)."""
    p = np.concatenate(gen())
    for _ in range(30):
        lam, V = np.linalg.eigh(hessian_f64(p))
        keep = lam > 1e-6 * lam[-1]
        g = tw.gradient_f64(p)
        p = p - V[:, keep] @ ((V[:, keep].T @ g) / lam[keep])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def square4():
    """The planar LJ4 square, a stationary point of Morse index 2, as a point [x | y | z]: its side by 200 bisections on the
    gradient in [1.0, 1.3]."""
    def point(a):
        return np.array([0.0, a, a, 0.0, 0.0, 0.0, a, a, 0.0, 0.0, 0.0, 0.0])

    lo, hi = 1.0, 1.3                                       # dE/dx of the corner at the origin: > 0 (repelled) at lo, < 0 at hi
    assert tw.gradient_f64(point(lo))[0] > 0 > tw.gradient_f64(point(hi))[0]
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if tw.gradient_f64(point(mid))[0] > 0:
            lo = mid
        else:
            hi = mid
    p = point(0.5 * (lo + hi))
    p.setflags(write=False)
    return p


def zero_tolerance(dtype, lam_max):
    """The ``zero_tol`` the GPU tests hand to ``morse_index``: 1e-9 lambda_max in fp64, 1e-3 lambda_max in fp32."""
    return (1e-9 if np.dtype(dtype) == np.float64 else 1e-3) * lam_max
