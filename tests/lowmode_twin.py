"""CPU twin of the batched lowest Hessian mode (csrc/dzo_lowmode.hip) as include/dzo.h states it, items a .. h: the restarted
Lanczos iteration with classical Gram-Schmidt twice, the rigid-body projector, the clean-up passes and the Jacobi iteration on
the small tridiagonal, every operation in the precision and the order the header names.  A helper module for
tests/test_lowmode_twin.py (which checks it against things it does not depend on) and tests/test_gpu_lowmode.py (which checks
the device kernels against it).  Not a conftest, no fixtures.

Three levels:

* ``hvp``: the product of ``hessian_twin.hvp_bits`` with the loop over i vectorised (numpy rounds every array operation once,
  like the scalar loop) and the radial values of a point computed once; ``fma64`` / ``fma32`` are exact fused multiply-adds on
  arrays (error-free transforms and rounding to odd) in place of pairwise_twin's Fraction arithmetic.
* ``lowest_mode``: the iteration.  What a correct kernel must reproduce bit for bit for a given start vector.
* ``dense_truth``: the spectrum of the projected dense fp64 Hessian by LAPACK.  The reference of the eigenvalues.
"""
import numpy as np

import hessian_twin as ht
import pairwise_twin as tw
import tempering_twin as tt

CONVERGED, UNFINISHED, FAILED = 0, 1, 2
MAX_KRYLOV, SWEEPS, CLEANUPS = 32, 30, 4
F64 = np.float64


# ------------------------------------------------------------------------------ exact fused multiply-add on arrays
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _sum_to_odd(a, b):
    """a + b rounded to odd: the nearest-even sum unless it is inexact and even, then its neighbour on the side of the error."""
    s, e = _two_sum(a, b)
    s = np.ascontiguousarray(s, dtype=F64)
    even = (s.view(np.int64) & 1) == 0
    other = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    return np.where((e != 0) & even, other, s)


def fma64(a, b, c):
    """a * b + c with one rounding, fp64 arrays (Boldo and Melquiond: the low parts are added to odd).  Normal range only."""
    a, b, c = (np.atleast_1d(np.asarray(v, dtype=F64)) for v in (a, b, c))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        return th + _sum_to_odd(tl, ul)


def fma32(a, b, c):
    """a * b + c with one rounding, fp32 arrays: the product is exact in fp64, the sum to odd there, then one rounding."""
    a, b, c = (np.atleast_1d(np.asarray(v, dtype=np.float32)).astype(F64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        return _sum_to_odd(a * b, c).astype(np.float32)


def _fma(a, b, c, dtype):
    return fma64(a, b, c) if np.dtype(dtype) == F64 else fma32(a, b, c)


# ------------------------------------------------------------------------------ the product (item b)
def radials(P, dtype):
    """(F, S): lj_first_derivative and lj_second_derivative of every pair, [i, j], zero on the diagonal (the dropped self term)."""
    t = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        d = P[:, :, None] - P[:, None, :]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        np.fill_diagonal(r2, t(1))
        shape = r2.shape
        r2 = r2.ravel()
        inv_r2 = t(1) / r2
        inv_r4 = inv_r2 * inv_r2
        inv_r6 = inv_r4 * inv_r2
        inv_r8 = inv_r4 * inv_r4
        inv_r10 = inv_r8 * inv_r2
        F = t(-12) * _fma(inv_r8, inv_r6 + inv_r6, -inv_r8, dtype)
        S = t(48) * _fma(np.full_like(r2, t(3.5)), inv_r8 * inv_r8, -inv_r10, dtype)
    F, S = F.reshape(shape).astype(dtype), S.reshape(shape).astype(dtype)
    np.fill_diagonal(F, t(0))
    np.fill_diagonal(S, t(0))
    return F, S


def hvp(P, F, S, U):
    """hessian_twin.hvp_bits for all i at once: P, U (3, N) of the element type; the row sums run j = 0 .. N-1 from +0."""
    acc = np.zeros_like(P)
    with np.errstate(all="ignore"):
        for j in range(P.shape[1]):
            d = P - P[:, j:j + 1]
            du = U - U[:, j:j + 1]
            overlap = d[0] * du[0] + d[1] * du[1] + d[2] * du[2]
            os_ = overlap * S[:, j]
            g = os_ + os_
            acc = acc + (F[:, j] * du + g * d)
        return acc + acc


# ------------------------------------------------------------------------------ sums (item a)
_LANES = np.arange(64)


def _tree(v):
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ off]
    return v[0]


def psum(terms):
    """The sum over the particles of ``terms`` ((N,) or (N, m), fp64) in the order of the sums."""
    terms = np.asarray(terms, dtype=F64)
    n = terms.shape[0]
    if n <= 64:
        lanes = np.zeros((64,) + terms.shape[1:])
        lanes[:n] = terms
        return 0.0 + _tree(lanes)
    own = np.zeros((1024,) + terms.shape[1:])
    own[:n] = terms
    own = own.reshape((4, 256) + terms.shape[1:])                # [q, t]: particle t + 256 q
    part = np.zeros((256,) + terms.shape[1:])
    for q in range(4):
        part = part + own[q]
    waves = part.reshape((4, 64) + terms.shape[1:])
    r = np.zeros(terms.shape[1:])
    for k in range(4):
        r = r + _tree(waves[k])
    return r


def dots(Q, w):
    """q_k . w for every row of Q ((k, 3, N)), fp64: per particle a product and two fused multiply-adds, then the sum."""
    Q = np.asarray(Q).astype(F64)
    w = np.broadcast_to(np.asarray(w).astype(F64), Q.shape)
    shape = Q[:, 0].shape
    p = Q[:, 0] * w[:, 0]
    p = fma64(Q[:, 1].ravel(), w[:, 1].ravel(), p.ravel())
    p = fma64(Q[:, 2].ravel(), w[:, 2].ravel(), p).reshape(shape)
    return psum(p.T)


def dot(a, b):
    return float(dots(np.asarray(a)[None], b)[0])


# ------------------------------------------------------------------------------ projector (items c, d)
class Projector:
    def __init__(self, P):
        n = P.shape[1]
        self.n = F64(n)
        X = P.astype(F64)
        with np.errstate(all="ignore"):
            c = psum(X.T) / self.n
            self.rho = rho = X - c[:, None]
            xx, yy, zz = rho[0] * rho[0], rho[1] * rho[1], rho[2] * rho[2]
            g = psum(np.stack([yy + zz, xx + zz, xx + yy, rho[0] * rho[1], rho[0] * rho[2], rho[1] * rho[2]], axis=1))
            Gxx, Gyy, Gzz, Gxy, Gxz, Gyz = g[0], g[1], g[2], -g[3], -g[4], -g[5]
            A00, A01, A02 = Gyy * Gzz - Gyz * Gyz, Gxz * Gyz - Gxy * Gzz, Gxy * Gyz - Gxz * Gyy
            A11, A12, A22 = Gxx * Gzz - Gxz * Gxz, Gxy * Gxz - Gxx * Gyz, Gxx * Gyy - Gxy * Gxy
            det = Gxx * A00 + Gxy * A01 + Gxz * A02
            tr = Gxx + Gyy + Gzz
            self.ok = bool(det > 2.0 ** -36 * ((tr * tr) * tr))
            self.I = [A00 / det, A01 / det, A02 / det, A11 / det, A12 / det, A22 / det]

    def __call__(self, v):
        rho, t = self.rho, v.astype(F64)
        with np.errstate(all="ignore"):
            s = psum(np.stack([t[0], t[1], t[2], rho[1] * t[2] - rho[2] * t[1], rho[2] * t[0] - rho[0] * t[2],
                               rho[0] * t[1] - rho[1] * t[0]], axis=1))
            mx, my, mz = s[0] / self.n, s[1] / self.n, s[2] / self.n
            I00, I01, I02, I11, I12, I22 = self.I
            ox = I00 * s[3] + I01 * s[4] + I02 * s[5]
            oy = I01 * s[3] + I11 * s[4] + I12 * s[5]
            oz = I02 * s[3] + I12 * s[4] + I22 * s[5]
            out = np.stack([(t[0] - mx) - (oy * rho[2] - oz * rho[1]), (t[1] - my) - (oz * rho[0] - ox * rho[2]),
                            (t[2] - mz) - (ox * rho[1] - oy * rho[0])])
        return out.astype(v.dtype)


# ------------------------------------------------------------------------------ Ritz pair (item h)
def jacobi_lowest(alpha, beta):
    """(theta, y, sweeps) of the tridiagonal with diagonal ``alpha`` and off-diagonal ``beta``: the rules of the eigensolver's
    items 3-5 in fp64, the sweep test of item h."""
    k = len(alpha)
    A = np.zeros((k, k))
    V = np.eye(k)
    for i in range(k):
        A[i, i] = alpha[i]
    for i in range(k - 1):
        A[i + 1, i] = A[i, i + 1] = beta[i]
    m = k + (k & 1)
    cols = np.arange(k)
    sweeps = 0
    with np.errstate(all="ignore"):
        for sweep in range(SWEEPS + 1):
            off = np.zeros(k)
            for r in range(k):
                off = np.where(cols == r, off, off + A[r, :] * A[r, :])
            dia = np.diag(A) * np.diag(A)
            lanes = np.zeros((64, 2))
            lanes[:k, 0], lanes[:k, 1] = off, dia
            off2, dia2 = _tree(lanes)
            if off2 <= 2.0 ** -104 * (off2 + dia2) or sweep == SWEEPS:
                break
            sweeps += 1
            idx = list(range(m))
            for _ in range(m - 1):
                pairs = []
                for t in range(m // 2):
                    p, q = sorted((idx[t], idx[m - 1 - t]))
                    if q >= k:
                        continue
                    c, s = 1.0, 0.0
                    apq = A[p, q]
                    if apq != 0.0:
                        tau = (A[q, q] - A[p, p]) / (apq + apq)
                        tt_ = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                        c = 1.0 / np.sqrt(1.0 + tt_ * tt_)
                        s = tt_ * c
                    pairs.append((p, q, c, s))
                for p, q, c, s in pairs:
                    ap, aq = A[:, p].copy(), A[:, q].copy()
                    A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
                for p, q, c, s in pairs:
                    ap, aq = A[p, :].copy(), A[q, :].copy()
                    A[p, :], A[q, :] = c * ap - s * aq, s * ap + c * aq
                for p, q, c, s in pairs:
                    A[p, q] = A[q, p] = 0.0
                idx = [idx[0], idx[m - 1]] + idx[1:m - 1]
    best, low = 0, A[0, 0]
    for c in range(1, k):
        if A[c, c] < low:
            best, low = c, A[c, c]
    return A[best, best], V[:, best].copy(), sweeps


# ------------------------------------------------------------------------------ the start (item f)
def drawn_start(n, seed, dtype):
    """The start of the stream seeded with ``seed`` (= base_seed + b), (3, n) of dtype, by numpy's fp64 Box-Muller.  The
    device's fp64 logarithm and trigonometric functions may differ from numpy's in the last place, so a value that lies within
    that of a rounding boundary of dtype can differ: rare in fp32, expected in fp64."""
    raw, _ = tt.pcg_raw(tt.pcg_state(seed), 4 * n)
    d = raw.astype(np.uint64).reshape(n, 4)
    nx, ny, _ = tt.box_muller_f64(d[:, 0], d[:, 1])
    nz, _, _ = tt.box_muller_f64(d[:, 2], d[:, 3])
    return np.stack([nx, ny, nz]).astype(dtype)


# ------------------------------------------------------------------------------ the iteration (items e, g, h)
class Result:
    pass


def lowest_mode(point, dtype, project_rigid=True, krylov=32, max_cycles=20, res_tol=0.0, start=None, seed=0):
    """The header's iteration on the point [x | y | z].  Returns a Result with status, cycles, products, eigenvalue (dtype),
    vector ((3N,) of dtype), residual (fp64), and ``history``: (alpha_1, beta_1, scale) of every cycle."""
    dtype = np.dtype(dtype)
    P = np.asarray(point, dtype=dtype).reshape(3, -1)
    n = P.shape[1]
    assert 2 <= krylov <= MAX_KRYLOV and max_cycles >= 1 and (n >= 3 or not project_rigid)
    K = min(krylov, 3 * n - 6 if project_rigid else 3 * n)
    F, S = radials(P, dtype)
    proj = Projector(P) if project_rigid else None
    project = proj if project_rigid else (lambda t: t)
    v = drawn_start(n, seed, dtype) if start is None else np.asarray(start, dtype=dtype).reshape(3, n).copy()
    out = Result()
    out.status, out.cycles, out.products, out.history = FAILED, 0, 0, []
    alpha1 = beta1 = F64(np.nan)
    scale = F64(0)

    def normalise(t):
        with np.errstate(all="ignore"):
            s = np.sqrt(F64(dot(t, t)))
            r = F64(1) / s
            return (t.astype(F64) * r).astype(dtype), s

    def orthogonalise(t, Q):
        h = dots(Q, t)
        acc = t.astype(F64)
        with np.errstate(all="ignore"):
            for k in range(len(Q)):
                acc = acc - h[k] * Q[k].astype(F64)
        return acc.astype(dtype), h

    ok = proj.ok if project_rigid else True
    if ok:
        v, s0 = normalise(project(v))
        ok = bool(s0 > 0 and s0 < np.inf)
    cycle = 0
    with np.errstate(all="ignore"):
        while ok and cycle < max_cycles:
            out.cycles = cycle + 1
            Q = [v]
            alpha, beta = [], []
            finished = False
            for j in range(K):
                w = project(hvp(P, F, S, Q[j]))
                out.products += 1
                last = j == K - 1 and j > 0
                h = dots(np.stack(Q), w)
                alpha.append(F64(h[j]))
                if last:
                    break
                w, _ = orthogonalise(w, Q)
                if j == 0:
                    alpha1, beta1 = alpha[0], np.sqrt(F64(dot(w, w)))
                    if np.abs(alpha1) > scale:
                        scale = np.abs(alpha1)
                    out.history.append((float(alpha1), float(beta1), float(scale)))
                    if beta1 <= F64(res_tol) * scale:
                        out.status, finished = CONVERGED, True
                        break
                    if cycle == max_cycles - 1:
                        out.status, finished = UNFINISHED, True
                        break
                w, _ = orthogonalise(w, Q)
                bj = np.sqrt(F64(dot(w, w)))
                if not bj > 0:
                    break
                w = (w.astype(F64) * (F64(1) / bj)).astype(dtype)
                dead = False
                for _ in range(CLEANUPS):
                    w, _ = orthogonalise(project(w), Q)
                    w, s = normalise(w)
                    if not s > 0:
                        dead = True
                        break
                    if s > 0.7:
                        break
                if dead:
                    break
                beta.append(bj)
                Q.append(w)
            if finished:
                break
            steps = len(alpha)
            theta, y, _ = jacobi_lowest(alpha, beta[:steps - 1])
            if np.abs(theta) > scale:
                scale = np.abs(theta)
            acc = np.zeros((3, n))
            for k in range(steps):
                acc = acc + y[k] * Q[k].astype(F64)
            v, s = normalise(project(acc.astype(dtype)))
            if not (s > 0 and s < np.inf):
                out.status, alpha1, beta1 = FAILED, F64(np.nan), F64(np.nan)
                break
            cycle += 1
    out.eigenvalue = dtype.type(alpha1)
    out.vector = v.reshape(-1)
    out.residual = float(beta1)
    out.scale = float(scale)
    return out


# ------------------------------------------------------------------------------ dense truth
def rigid_basis(point):
    """Orthonormal basis (3N, 6) of the net translations and the rotations about the centroid of the point [x | y | z]
    (fewer columns for a collinear point)."""
    c = np.asarray(point, dtype=F64).reshape(3, -1)
    n = c.shape[1]
    rho = c - c.mean(axis=1, keepdims=True)
    B = np.zeros((3 * n, 6))
    for a in range(3):
        B[a * n:(a + 1) * n, a] = 1.0
        e = np.zeros(3)
        e[a] = 1.0
        B[:, 3 + a] = np.cross(e, rho.T).T.reshape(-1)          # omega x rho with omega = e_a
    u, s, _ = np.linalg.svd(B, full_matrices=False)
    return u[:, s > 1e-10 * s[0]]


def dense_truth(point, dtype, project_rigid=True):
    """(ascending eigenvalues of H restricted to the range of P, H, Pm): H = ``hessian_f64`` of the point as rounded to dtype,
    symmetrised; Pm the dense projector (the identity without ``project_rigid``)."""
    q = np.asarray(point, dtype=dtype).astype(F64)
    H = ht.hessian_f64(q)
    H = 0.5 * (H + H.T)
    n3 = len(q)
    if not project_rigid:
        return np.linalg.eigvalsh(H), H, np.eye(n3)
    B = rigid_basis(q)
    Pm = np.eye(n3) - B @ B.T
    Z = np.linalg.svd(B, full_matrices=True)[0][:, B.shape[1]:]
    R = Z.T @ H @ Z
    return np.linalg.eigvalsh(0.5 * (R + R.T)), H, Pm


EPS = {np.dtype(np.float64): 2.0 ** -52, np.dtype(np.float32): 2.0 ** -23}


def gamma(n):
    """The rounding count behind delta: the row sum of a product adds N terms sequentially (N roundings on the path of the
    first term) and one term carries at most 32 roundings of its own -- the differences d and du (2), r2 (5), the two radial
    functions (a division, the powers, the fused multiply-add and the constant: 10), the overlap (5), g (1), f du + g d (3),
    and the conversions of the projector and the last doubling with room to spare.  The count of tests/test_gpu_pairwise.py."""
    return n + 32


def truth_figures(point, dtype, project_rigid, eigenvalue, vector):
    """(ev, rho_host, delta, hnorm): the ascending dense eigenvalues on the range of P; rho_host = |P (H u - lambda u)| in fp64
    from the dense truth; delta = gamma eps_T | |H| |u| |_2; hnorm = the largest |eigenvalue| of H, a bound of every Rayleigh
    quotient and Ritz value the iteration can have seen (its `scale`)."""
    ev, H, Pm = dense_truth(point, dtype, project_rigid)
    u = np.asarray(vector, dtype=F64).reshape(-1)
    lam = float(eigenvalue)
    rho = float(np.linalg.norm(Pm @ (H @ u - lam * u)))
    delta = gamma(len(u) // 3) * EPS[np.dtype(dtype)] * float(np.linalg.norm(np.abs(H) @ np.abs(u)))
    hnorm = float(np.abs(np.linalg.eigvalsh(H)).max())
    return ev, rho, delta, hnorm


def gap_is_usable(ev):
    """The lowest eigenvalue is either separated by at least 0.55 or degenerate to rounding (1e-9 of the spectrum's scale)."""
    gap = ev[1] - ev[0]
    return bool(gap >= 0.55 or gap <= 1e-9 * np.abs(ev).max())
