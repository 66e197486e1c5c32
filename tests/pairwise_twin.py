"""CPU twin of the pairwise radial (Lennard-Jones) N-body functions of src/ExampleFunctions.jl, written from the
formulas (:16-72 for the radial functions, :117-149 / :224-262 / :367-424 / :477-534 for the four sums).  A helper
module for tests/test_pairwise_twin.py (which checks it against things it does not depend on) and
tests/test_gpu_pairwise.py (which checks the device kernels against it).  Not a conftest, no fixtures.

Two levels:

* single pairs with the reference's operations one by one, every operation rounded once to the element type and
  every ``muladd`` an EXACT fused multiply-add (``fractions.Fraction``, rounded once): ``pair_energy``,
  ``pair_gradient``, ``pair_hvp``.  What a correct kernel must reproduce bit for bit when N = 2.
* the sums in ``np.longdouble`` (64-bit mantissa on x86) as the "exact" value, together with S: the sum of the
  absolute values of the terms of each row, which scales the derived error bound of the GPU tests.
"""
from fractions import Fraction
import math

import numpy as np

LD = np.longdouble
PHI = (1.0 + math.sqrt(5.0)) / 2.0


# ------------------------------------------------------------------------------ exact fma, rounded once
def round_fraction(fr, dtype):
    """Fraction -> nearest value of dtype (ties to even); normal range only."""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return np.float64(float(fr))                      # int / int true division is correctly rounded
    assert dtype == np.float32
    if fr == 0:
        return np.float32(0.0)
    sign = -1 if fr < 0 else 1
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    assert -126 <= e <= 126, "outside fp32's normal range"
    q = a / Fraction(2) ** (e - 23)                       # in [2^23, 2^24)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** (e - 23))  # n <= 2^24: exact in double, exact in fp32


def fma(a, b, c, dtype):
    """a * b + c with ONE rounding to dtype."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return np.dtype(dtype).type(a) * np.dtype(dtype).type(b) + np.dtype(dtype).type(c)
    return round_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)), dtype)


# ------------------------------------------------------------------------------ radial functions, :16-72
def lj_energy(r2, dtype=np.float64):
    t = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        r2 = t(r2)
        inv_r2 = t(1) / r2
        inv_r4 = inv_r2 * inv_r2
        inv_r6 = inv_r4 * inv_r2
        return t(4) * fma(inv_r6, inv_r6, -inv_r6, dtype)


def lj_first_derivative(r2, dtype=np.float64):
    t = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        r2 = t(r2)
        inv_r2 = t(1) / r2
        inv_r4 = inv_r2 * inv_r2
        inv_r6 = inv_r4 * inv_r2
        inv_r8 = inv_r4 * inv_r4
        return t(-12) * fma(inv_r8, inv_r6 + inv_r6, -inv_r8, dtype)


def lj_second_derivative(r2, dtype=np.float64):
    t = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        r2 = t(r2)
        inv_r2 = t(1) / r2
        inv_r4 = inv_r2 * inv_r2
        inv_r8 = inv_r4 * inv_r4
        inv_r10 = inv_r8 * inv_r2
        return t(48) * fma(t(3.5), inv_r8 * inv_r8, -inv_r10, dtype)


# ------------------------------------------------------------------------------ single pairs (N = 2), the reference's order
def _r2(d, dtype):
    t = np.dtype(dtype).type
    dx, dy, dz = (t(v) for v in d)
    return dx * dx + dy * dy + dz * dz                     # left to right, :252


def pair_energy(p0, p1, dtype=np.float64):
    """E of two particles: row 0 is 0 + e, row 1 is 0 + e, each halved, summed (:137-147, :172)."""
    t = np.dtype(dtype).type
    p0 = [t(v) for v in p0]; p1 = [t(v) for v in p1]
    e01 = lj_energy(_r2([a - b for a, b in zip(p0, p1)], dtype), dtype)
    e10 = lj_energy(_r2([a - b for a, b in zip(p1, p0)], dtype), dtype)
    return float(t(0.5) * (t(0) + e01)) + float(t(0.5) * (t(0) + e10))


def pair_gradient(p0, p1, dtype=np.float64):
    """(g of particle 0, g of particle 1), three components each (:245-260)."""
    t = np.dtype(dtype).type
    p0 = [t(v) for v in p0]; p1 = [t(v) for v in p1]
    out = []
    for a, b in ((p0, p1), (p1, p0)):
        d = [ai - bi for ai, bi in zip(a, b)]
        f = lj_first_derivative(_r2(d, dtype), dtype)
        acc = [t(0) + f * dc for dc in d]
        out.append([ac + ac for ac in acc])
    return out


def pair_hvp(p0, p1, u0, u1, dtype=np.float64):
    """(p of particle 0, p of particle 1) for the direction (u0, u1) (:395-422)."""
    t = np.dtype(dtype).type
    p0 = [t(v) for v in p0]; p1 = [t(v) for v in p1]
    u0 = [t(v) for v in u0]; u1 = [t(v) for v in u1]
    out = []
    for (a, b, ua, ub) in ((p0, p1, u0, u1), (p1, p0, u1, u0)):
        d = [ai - bi for ai, bi in zip(a, b)]
        du = [ai - bi for ai, bi in zip(ua, ub)]
        r2 = _r2(d, dtype)
        f = lj_first_derivative(r2, dtype)
        s = lj_second_derivative(r2, dtype)
        overlap = d[0] * du[0] + d[1] * du[1] + d[2] * du[2]
        os_ = overlap * s
        g = os_ + os_
        acc = [t(0) + (f * duc + g * dc) for dc, duc in zip(d, du)]
        out.append([ac + ac for ac in acc])
    return out


# ------------------------------------------------------------------------------ the sums, "exact" (longdouble) + S
def _ld_radial(r2):
    """(e, e', e'') of a longdouble array of r2 (the formulas of :16-72; a muladd is a * b + c here)."""
    inv_r2 = LD(1) / r2
    inv_r4 = inv_r2 * inv_r2
    inv_r6 = inv_r4 * inv_r2
    inv_r8 = inv_r4 * inv_r4
    inv_r10 = inv_r8 * inv_r2
    e = LD(4) * (inv_r6 * inv_r6 - inv_r6)
    e1 = LD(-12) * (inv_r8 * (inv_r6 + inv_r6) - inv_r8)
    e2 = LD(48) * (LD(3.5) * (inv_r8 * inv_r8) - inv_r10)
    return e, e1, e2


def _rows_iter(n, rows, block):
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    for k in range(0, len(rows), block):
        yield k, rows[k:k + block]


def _deltas(x, y, z, r):
    xl, yl, zl = (np.asarray(a, dtype=LD) for a in (x, y, z))
    dx = xl[r, None] - xl[None, :]
    dy = yl[r, None] - yl[None, :]
    dz = zl[r, None] - zl[None, :]
    r2 = dx * dx + dy * dy + dz * dz
    self_ = r[:, None] == np.arange(len(xl))[None, :]
    return dx, dy, dz, r2, self_


def row_energies(x, y, z, rows=None, block=64):
    """(sum_{j != i} e(r2_ij), sum_{j != i} |e(r2_ij)|) for the given rows, longdouble."""
    n = len(x)
    nrows = n if rows is None else len(rows)
    e_out = np.zeros(nrows, dtype=LD); s_out = np.zeros(nrows, dtype=LD)
    with np.errstate(all="ignore"):
        for k, r in _rows_iter(n, rows, block):
            _, _, _, r2, self_ = _deltas(x, y, z, r)
            e, _, _ = _ld_radial(r2)
            e = np.where(self_, LD(0), e)
            e_out[k:k + len(r)] = e.sum(axis=1)
            s_out[k:k + len(r)] = np.abs(e).sum(axis=1)
    return e_out, s_out


def energy(x, y, z):
    """(E, S): E = sum_i 1/2 sum_{j != i} e, S = 1/2 sum_i S_i."""
    e, s = row_energies(x, y, z)
    return LD(0.5) * e.sum(), LD(0.5) * s.sum()


def energy_blockwise_f64(x, y, z, block=512):
    """(E, S) with every operation in fp64 numpy, upper-triangle blocks (each pair once: 1/2 (e_ij + e_ji) = e_ij);
    for N too large for the longdouble form."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    n = len(x)
    tot = []; s = []
    for a in range(0, n, block):
        xa, ya, za = x[a:a + block, None], y[a:a + block, None], z[a:a + block, None]
        for b in range(a, n, block):
            dx = xa - x[None, b:b + block]; dy = ya - y[None, b:b + block]; dz = za - z[None, b:b + block]
            r2 = dx * dx + dy * dy + dz * dz
            if a == b:
                iu = np.triu_indices(r2.shape[0], 1, r2.shape[1])
                r2 = r2[iu]
            inv_r2 = 1.0 / r2
            inv_r6 = inv_r2 * inv_r2 * inv_r2
            e = 4.0 * (inv_r6 * inv_r6 - inv_r6)
            tot.append(float(e.sum())); s.append(float(np.abs(e).sum()))     # numpy's pairwise sums per block
    return math.fsum(tot), math.fsum(s)


def gradient(x, y, z, rows=None, block=64):
    """(g, S, Sc): g[c, k] = 2 sum_{j != i} e'(r2_ij) d_c for row i = rows[k]; S[k] = sum_j 2 |e'| |r_i - r_j| (the absolute
    values of the row's terms, which are vectors: S_i of the error bound); Sc[c, k] = sum_j 2 |e'| |d_c|, the same per
    component (a stricter scale, for information)."""
    n = len(x)
    nrows = n if rows is None else len(rows)
    g = np.zeros((3, nrows), dtype=LD); S = np.zeros((3, nrows), dtype=LD); Srow = np.zeros(nrows, dtype=LD)
    with np.errstate(all="ignore"):
        for k, r in _rows_iter(n, rows, block):
            dx, dy, dz, r2, self_ = _deltas(x, y, z, r)
            _, f, _ = _ld_radial(r2)
            f = np.where(self_, LD(0), f)
            for c, d in enumerate((dx, dy, dz)):
                t = f * d
                g[c, k:k + len(r)] = LD(2) * t.sum(axis=1)
                S[c, k:k + len(r)] = LD(2) * np.abs(t).sum(axis=1)
            Srow[k:k + len(r)] = LD(2) * (np.abs(f) * np.sqrt(r2)).sum(axis=1)
    return g, Srow, S


def hvp(x, y, z, u, v, w, rows=None, block=64):
    """(p, S, Sc): p[c, k] = 2 sum_{j != i} [e' du_c + 2 (overlap e'') d_c];
    S[k] = sum_j 2 (|e'||du| + 2 |e''| (|dx du| + |dy dv| + |dz dw|) |dr|) with |du|, |dr| the lengths of u_i - u_j and
    r_i - r_j (overlap cancels, so its terms are taken apart): S_i of the error bound; Sc[c, k] the same with |du_c|, |d_c|."""
    n = len(x)
    nrows = n if rows is None else len(rows)
    p = np.zeros((3, nrows), dtype=LD); S = np.zeros((3, nrows), dtype=LD); Srow = np.zeros(nrows, dtype=LD)
    ul, vl, wl = (np.asarray(a, dtype=LD) for a in (u, v, w))
    with np.errstate(all="ignore"):
        for k, r in _rows_iter(n, rows, block):
            dx, dy, dz, r2, self_ = _deltas(x, y, z, r)
            du = ul[r, None] - ul[None, :]; dv = vl[r, None] - vl[None, :]; dw = wl[r, None] - wl[None, :]
            _, f, s = _ld_radial(r2)
            f = np.where(self_, LD(0), f); s = np.where(self_, LD(0), s)
            overlap = dx * du + dy * dv + dz * dw
            aover = np.abs(dx * du) + np.abs(dy * dv) + np.abs(dz * dw)
            gg = LD(2) * (overlap * s)
            for c, (d, dd) in enumerate(((dx, du), (dy, dv), (dz, dw))):
                p[c, k:k + len(r)] = LD(2) * (f * dd + gg * d).sum(axis=1)
                S[c, k:k + len(r)] = LD(2) * (np.abs(f) * np.abs(dd) + LD(2) * np.abs(s) * aover * np.abs(d)).sum(axis=1)
            Srow[k:k + len(r)] = LD(2) * (np.abs(f) * np.sqrt(du * du + dv * dv + dw * dw) + LD(2) * np.abs(s) * aover * np.sqrt(r2)).sum(axis=1)
    return p, Srow, S


def energy_delta(x, y, z, i, xn, yn, zn):
    """(delta, S_old + S_new) of :477-534: particle i (0-based) moved to (xn, yn, zn)."""
    xl, yl, zl = (np.asarray(a, dtype=LD) for a in (x, y, z))
    keep = np.arange(len(xl)) != i
    with np.errstate(all="ignore"):
        def part(px, py, pz):
            dx = px - xl[keep]; dy = py - yl[keep]; dz = pz - zl[keep]
            e, _, _ = _ld_radial(dx * dx + dy * dy + dz * dz)
            return e.sum(), np.abs(e).sum()
        e_old, s_old = part(xl[i], yl[i], zl[i])
        e_new, s_new = part(LD(xn), LD(yn), LD(zn))
    return e_new - e_old, s_old + s_new


# fp64 forms for scipy (the longdouble ones are for checking, these for minimising)
def energy_f64(p):
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]; dz = z[:, None] - z[None, :]
    r2 = dx * dx + dy * dy + dz * dz
    iu = np.triu_indices(n, 1)
    inv_r6 = 1.0 / r2[iu] ** 3
    return float(np.sum(4.0 * (inv_r6 * inv_r6 - inv_r6)))


def gradient_f64(p):
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]; dz = z[:, None] - z[None, :]
    r2 = dx * dx + dy * dy + dz * dz
    np.fill_diagonal(r2, 1.0)
    inv_r2 = 1.0 / r2
    inv_r6 = inv_r2 ** 3
    inv_r8 = inv_r6 * inv_r2
    f = -12.0 * (inv_r8 * (inv_r6 + inv_r6) - inv_r8)
    np.fill_diagonal(f, 0.0)
    return np.concatenate([2.0 * (f * d).sum(axis=1) for d in (dx, dy, dz)])


# ------------------------------------------------------------------------------ generators
def icosahedron13():
    """Centre + the 12 cyclic permutations of (0, +-1, +-phi), vertices 1.08 from the centre: (x, y, z)."""
    pts = [(0.0, 0.0, 0.0)]
    for a in (-1.0, 1.0):
        for b in (-PHI, PHI):
            pts += [(0.0, a, b), (a, b, 0.0), (b, 0.0, a)]
    p = np.array(pts) * (1.08 / math.sqrt(1.0 + PHI * PHI))
    assert p.shape == (13, 3)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def octahedron38():
    """The 38-atom truncated octahedron: integer points with odd coordinate sum, |a| + |b| + |c| <= 3 ... (an fcc
    fragment), nearest-neighbour distance 1.09."""
    pts = [(a, b, c) for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4)
           if (a + b + c) % 2 != 0 and abs(a) + abs(b) + abs(c) <= 3 and max(abs(a), abs(b), abs(c)) <= 2]
    assert len(pts) == 38, len(pts)
    p = np.array(pts, dtype=np.float64) * (1.09 / math.sqrt(2.0))
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def lattice(n, seed=0, spacing=1.12, jitter=0.05):
    """The first n sites of a cubic lattice, each coordinate jittered by a uniform +-jitter (seeded)."""
    m = 1
    while m ** 3 < n:
        m += 1
    idx = np.arange(n)
    p = np.stack([idx // (m * m), (idx // m) % m, idx % m], axis=1).astype(np.float64) * spacing
    p += np.random.default_rng(seed).uniform(-jitter, jitter, size=p.shape)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def jittered(xyz, seed, jitter=0.05):
    rng = np.random.default_rng(seed)
    return tuple(a + rng.uniform(-jitter, jitter, size=a.shape) for a in xyz)


def cluster(n, seed=0):
    """The configuration the GPU tests use for n particles: icosahedron / octahedron where n fits, lattice otherwise."""
    if n == 13:
        return icosahedron13()
    if n == 38:
        return octahedron38()
    return lattice(n, seed)


LJ13 = -44.326801      # Cambridge Cluster Database, to its printed precision
LJ38 = -173.928427
