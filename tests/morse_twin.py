"""CPU twin of the Morse pair potential (include/dzo.h: DZO_RADIAL_MORSE_RHO6, DZO_RADIAL_MORSE_RHO14) and of the pairwise
sums built on it, with rho as a parameter.  A helper module like pairwise_twin.py (no fixtures; imported by name) for
tests/test_morse_twin.py, which checks it against things it does not depend on, and tests/test_gpu_morse.py, which checks the
device kernels against it.

With r = sqrt(r2), a = rho (1 - r), t = exp(a):

    energy = t^2 - 2 t          first = dE/d(r2) = -rho t (t - 1) / r          second = d2E/d(r2)2 = rho t (rho r (2t - 1) + (t - 1)) / (2 r2 r)

Two levels of precision:

* ``radial_mp``: the three functions of one r2 in mpmath (50 digits by default), the yardstick of the yardstick;
* ``radial`` and the sums (energy, gradient, hvp, hessian, energy_delta): numpy.longdouble arrays (64-bit mantissa on x86, so
  2^-64 per operation against the 2^-53 of the most precise device type).  tests/test_morse_twin.py holds ``radial`` against
  ``radial_mp``; an (n, n) sum in mpmath itself would take minutes per test.

The device's exp is not correctly rounded, so a device result cannot be replayed bit for bit.  ``bound`` is the permitted
absolute error of one output entry instead; it is derived below from the functor's operation sequence (csrc/dzo_pairwise.h), not
from anything a kernel returned.

The bound
---------
u = eps_T / 2 is the unit roundoff of the device type (2^-53, 2^-24); every rounded operation has a relative error of at most u.
The coordinates are values of T, so the twin and the device see the same points.

    dx, dy, dz               one subtraction each                                     relative u
    r2 = dx^2 + dy^2 + dz^2  2u (the squared differences) + u (squares) + 2u (adds)   relative 5u (all terms positive)
    r = sqrt(r2)             5u / 2 + u (IEEE square root)                            relative 3.5u
    a = rho (1 - r)          3.5u r rho (from r) + |a| u (subtraction) + |a| u (product)   absolute
    t = exp(a)               the error of a, amplified by d(ln t)/da = 1, + EXP_ULPS ulps of the device exp (1 ulp <= 2u relative)
                             dt := 3.5 u rho r + 2 u |a| + 2 u EXP_ULPS                relative

(the amplification |a| of the issue's wording is the 2 u |a| term: the two roundings that form a are relative to a, and exp turns
an absolute error of its argument into a relative error of its value.)

    energy = fma(t, t, -2t)  |dE/dt| t dt + |e| u                    err_e = 2 t |t - 1| dt + |e| u
    first  = ((-rho t)(t - 1)) / r
             t - 1: t dt + |t - 1| u absolute; -rho t: dt + u; product u; r: 3.5u; division u
                                                                      err_f = |f| (dt + 7.5u) + rho t^2 dt / r
    second = ((rho t) inner) / ((2 r2) r),  inner = fma(rho r, 2t - 1, t - 1)
             rho r: 4.5u; 2t - 1: 2 t dt + |2t - 1| u absolute; fma: u
             err_inner = rho r |2t - 1| 4.5u + rho r (2 t dt + |2t - 1| u) + t dt + |t - 1| u + |inner| u
             err_num = rho t err_inner + |num| (dt + 2u);   denominator: 5u + 3.5u + u = 9.5u;   division u
                                                                      err_s = err_num / den + |s| 10.5u

These are absolute errors of one pair's radial values; written as |term| c they give the c_ij of "eps_T sum_j |term_ij| c_ij"
(c_ij = err / (eps_T |term|)), but the absolute form stays finite where a term is zero (the energy at t = 2, first at r = 1).
A row of n terms added one after the other in T costs at most (n - 1) u sum_j |term_ij| more, whatever the order; the pairwise
kernels may split a row into at most 64 partial sums (kPwMaxSplit) that are added afterwards, so rows count n + 64 additions.
Sums across lanes and blocks are taken in fp64 and rounded to T once: u_64 (n + 64) S + u |result|.  Everything is first order in
u; the second-order terms are below (n + 64) u of the bound itself (2e-5 for fp32 at n = 300) and are covered by the factor 1.01.

floor: for t below tiny_T / eps_T (1.0e-31 for fp32; never reached in fp64, where it would need r > 48) the device's t is
denormal or zero and has no relative accuracy.  There the pair's error is at most twice the magnitude the term has at
t_f = tiny_T / eps_T (the terms grow with t for t << 1): 4 t_f for the energy, 2 rho t_f / r for first, rho t_f (rho r + 1) / r^3
for second.  It is added to the pair's error instead of the relative terms.

EXP_ULPS: ROCm's documentation on the build machine does not state the accuracy of the device exp / expf, so 1 ulp is assumed
and doubled.
"""
import functools
import math

import numpy as np

LD = np.longdouble
EXP_ULPS = 2.0
EPS = {np.dtype(np.float64): LD(2.0) ** -52, np.dtype(np.float32): LD(2.0) ** -23}
TINY = {np.dtype(np.float64): LD(np.finfo(np.float64).tiny), np.dtype(np.float32): LD(np.finfo(np.float32).tiny)}
SPLIT_ADDS = 64
MORSE13_RHO6 = -42.439863      # Cambridge Cluster Database (Doye & Wales), to its printed precision


# ------------------------------------------------------------------------------ radial functions
def radial_mp(r2, rho, dps=50):
    """(energy, first, second) of one r2 as mpmath numbers (tests/test_morse_twin.py falls back on longdouble checks where
    mpmath is not importable)."""
    try:
        import mpmath
    except ImportError:                                      # the longdouble forms, as scalars
        return tuple(q[()] for q in radial(np.asarray(r2, dtype=LD), rho))
    with mpmath.workdps(dps):
        r2 = mpmath.mpf(r2)
        r = mpmath.sqrt(r2)
        t = mpmath.exp(rho * (1 - r))
        return t * t - 2 * t, -rho * t * (t - 1) / r, rho * t * (rho * r * (2 * t - 1) + (t - 1)) / (2 * r2 * r)


def radial(r2, rho):
    """(energy, first, second) of a longdouble array of r2."""
    r2 = np.asarray(r2, dtype=LD)
    r = np.sqrt(r2)
    t = np.exp(LD(rho) * (LD(1) - r))
    return t * t - LD(2) * t, -LD(rho) * t * (t - LD(1)) / r, LD(rho) * t * (LD(rho) * r * (LD(2) * t - LD(1)) + (t - LD(1))) / (LD(2) * r2 * r)


# ------------------------------------------------------------------------------ pairs of one configuration
def _pairs(x, y, z, rho, rows=None):
    """dx, dy, dz, r2, self and the three radial values (zero on the diagonal) of rows x all particles, longdouble."""
    xl, yl, zl = (np.asarray(a, dtype=LD) for a in (x, y, z))
    r = np.arange(len(xl)) if rows is None else np.asarray(rows, dtype=np.int64)
    dx = xl[r, None] - xl[None, :]; dy = yl[r, None] - yl[None, :]; dz = zl[r, None] - zl[None, :]
    r2 = dx * dx + dy * dy + dz * dz
    self_ = r[:, None] == np.arange(len(xl))[None, :]
    with np.errstate(all="ignore"):
        e, f, s = radial(np.where(self_, LD(1), r2), rho)
    zero = LD(0)
    return dx, dy, dz, r2, self_, np.where(self_, zero, e), np.where(self_, zero, f), np.where(self_, zero, s)


BLOCK_ROWS = 256               # the sums of a large configuration are taken over blocks of rows, to keep the arrays small


def _blocks(n):
    return [np.arange(k, min(k + BLOCK_ROWS, n)) for k in range(0, n, BLOCK_ROWS)]


def energy(x, y, z, rho):
    """E = sum_i 1/2 sum_{j != i} e(r2_ij)."""
    return LD(0.5) * sum(_pairs(x, y, z, rho, rows)[5].sum() for rows in _blocks(len(x)))


def row_energies(x, y, z, rho):
    """sum_{j != i} e(r2_ij) for every i (twice the per-particle energies)."""
    return _pairs(x, y, z, rho)[5].sum(axis=1)


def gradient(x, y, z, rho, rows=None):
    """g[c, k] = 2 sum_{j != i} e'(r2_ij) d_c for i = rows[k] (all rows when None)."""
    dx, dy, dz, _, _, _, f, _ = _pairs(x, y, z, rho, rows)
    return np.stack([LD(2) * (f * d).sum(axis=1) for d in (dx, dy, dz)])


def hvp(x, y, z, u, v, w, rho, rows=None):
    """p[c, k] = 2 sum_{j != i} [e' du_c + 2 (overlap e'') d_c] for i = rows[k] (all rows when None)."""
    dx, dy, dz, _, _, _, f, s = _pairs(x, y, z, rho, rows)
    ul, vl, wl = (np.asarray(a, dtype=LD) for a in (u, v, w))
    r = np.arange(len(ul)) if rows is None else np.asarray(rows, dtype=np.int64)
    du = ul[r, None] - ul[None, :]; dv = vl[r, None] - vl[None, :]; dw = wl[r, None] - wl[None, :]
    g = LD(2) * ((dx * du + dy * dv + dz * dw) * s)
    return np.stack([LD(2) * (f * dd + g * d).sum(axis=1) for d, dd in ((dx, du), (dy, dv), (dz, dw))])


def hessian(x, y, z, rho):
    """The dense Hessian, (3n, 3n), index c n + i: block (i, j != i) = -(2 f delta_ab + 4 s d_a d_b), block (i, i) = -sum of the row."""
    dx, dy, dz, _, _, _, f, s = _pairs(x, y, z, rho)
    n = len(x)
    d = (dx, dy, dz)
    h = np.zeros((3 * n, 3 * n), dtype=LD)
    for a in range(3):
        for b in range(3):
            blk = LD(4) * s * (d[a] * d[b]) + (LD(2) * f if a == b else LD(0))
            h[a * n:(a + 1) * n, b * n:(b + 1) * n] = -blk
            h[a * n + np.arange(n), b * n + np.arange(n)] = blk.sum(axis=1)
    return h


def energy_delta(x, y, z, i, xn, yn, zn, rho):
    """E(particle i at (xn, yn, zn)) - E."""
    xl, yl, zl = (np.asarray(a, dtype=LD) for a in (x, y, z))
    keep = np.arange(len(xl)) != i

    def part(px, py, pz):
        dx = px - xl[keep]; dy = py - yl[keep]; dz = pz - zl[keep]
        return radial(dx * dx + dy * dy + dz * dz, rho)[0].sum()
    return part(LD(xn), LD(yn), LD(zn)) - part(xl[i], yl[i], zl[i])


# ------------------------------------------------------------------------------ the bound (derivation: the module docstring)
def _pair_errors(r2, self_, rho, dtype):
    """(e, f, s, err_e, err_f, err_s) for an array of r2; zero where self_."""
    dt_ = np.dtype(dtype)
    u = EPS[dt_] / 2
    rho = LD(rho)
    r2 = np.where(self_, LD(1), np.asarray(r2, dtype=LD))
    r = np.sqrt(r2)
    a = rho * (LD(1) - r)
    t = np.exp(a)
    e, f, s = radial(r2, rho)
    dt = u * (LD(3.5) * rho * r + 2 * np.abs(a) + 2 * LD(EXP_ULPS))
    err_e = 2 * t * np.abs(t - 1) * dt + np.abs(e) * u
    err_f = np.abs(f) * (dt + LD(7.5) * u) + rho * t * t * dt / r
    inner = rho * r * (2 * t - 1) + (t - 1)
    err_inner = rho * r * np.abs(2 * t - 1) * LD(4.5) * u + rho * r * (2 * t * dt + np.abs(2 * t - 1) * u) + t * dt + np.abs(t - 1) * u + np.abs(inner) * u
    num, den = rho * t * inner, 2 * r2 * r
    err_s = (rho * t * err_inner + np.abs(num) * (dt + 2 * u)) / den + np.abs(s) * LD(10.5) * u
    t_f = TINY[dt_] / EPS[dt_]
    low = t < t_f
    err_e = np.where(low, 4 * t_f, err_e)
    err_f = np.where(low, 2 * rho * t_f / r, err_f)
    err_s = np.where(low, rho * t_f * (rho * r + 1) / (r2 * r), err_s)
    zero = LD(0)
    return tuple(np.where(self_, zero, q) for q in (e, f, s, err_e, err_f, err_s))


def bound(kind, dtype, x, y, z, rho, u=None, v=None, w=None, i=None, new=None, rows=None, with_value=False):
    """The permitted absolute error of every output entry of a device result of type ``dtype``:

    ``energy``: one number; ``rows``: (n,) of sum_{j != i} e; ``gradient``, ``hvp`` (with u, v, w): (3, n); ``hessian``: (3n, 3n);
    ``delta`` (with i and new = (xn, yn, zn)): one number.  ``rows``: the rows of ``gradient`` / ``hvp`` to give (all when None).
    ``with_value`` (``energy`` of more than BLOCK_ROWS particles): (bound, energy) from one pass over the pairs."""
    dt_ = np.dtype(dtype)
    uu, u64 = EPS[dt_] / 2, LD(2.0) ** -53
    n = len(x)
    adds = LD(n + SPLIT_ADDS)
    slack = LD(1.01)
    if kind == "delta":
        xl, yl, zl = (np.asarray(a, dtype=LD) for a in (x, y, z))
        keep = np.arange(n) != i
        total, sums = LD(0), []
        for px, py, pz in ((xl[i], yl[i], zl[i]), tuple(LD(q) for q in new)):
            dx = px - xl[keep]; dy = py - yl[keep]; dz = pz - zl[keep]
            e, _, _, err_e, _, _ = _pair_errors(dx * dx + dy * dy + dz * dz, np.zeros(keep.sum(), dtype=bool), rho, dtype)
            S = np.abs(e).sum()
            total += err_e.sum() + adds * (uu + u64) * S + uu * np.abs(e.sum())
            sums.append(e.sum())
        return slack * (total + uu * np.abs(sums[1] - sums[0]))
    if kind == "energy" and n > BLOCK_ROWS:                  # the same sums block by block
        rows_sum = S_sum = e_sum = LD(0)
        for blk in _blocks(n):
            _, _, _, r2, self_, _, _, _ = _pairs(x, y, z, rho, blk)
            e, _, _, err_e, _, _ = _pair_errors(r2, self_, rho, dtype)
            S = np.abs(e).sum(axis=1)
            rows_sum += (err_e.sum(axis=1) + adds * uu * S).sum(); S_sum += S.sum(); e_sum += e.sum()
        out = slack * (LD(0.5) * (rows_sum + adds * u64 * S_sum) + uu * np.abs(LD(0.5) * e_sum))
        return (out, LD(0.5) * e_sum) if with_value else out
    dx, dy, dz, r2, self_, _, _, _ = _pairs(x, y, z, rho, rows)
    e, f, s, err_e, err_f, err_s = _pair_errors(r2, self_, rho, dtype)
    if kind in ("energy", "rows"):
        S = np.abs(e).sum(axis=1)
        rows = err_e.sum(axis=1) + adds * uu * S
        if kind == "rows":
            return slack * (rows + uu * np.abs(e.sum(axis=1)))
        return slack * (LD(0.5) * (rows.sum() + adds * u64 * S.sum()) + uu * np.abs(LD(0.5) * e.sum()))
    d = (dx, dy, dz)
    if kind == "gradient":
        out = []
        for dc in d:
            term = np.abs(f * dc)
            out.append(2 * ((np.abs(dc) * err_f + 2 * uu * term).sum(axis=1) + adds * uu * term.sum(axis=1)))
        return slack * np.stack(out)
    if kind == "hvp":
        ul, vl, wl = (np.asarray(q, dtype=LD) for q in (u, v, w))
        r = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
        dd = (ul[r, None] - ul[None, :], vl[r, None] - vl[None, :], wl[r, None] - wl[None, :])
        terms = _hvp_term_errors(d, dd, f, s, err_f, err_s, uu)
        return slack * np.stack([2 * (err.sum(axis=1) + adds * uu * mag.sum(axis=1)) for err, mag in terms])
    if kind == "hessian":
        h = np.zeros((3 * n, 3 * n), dtype=LD)
        one, zero = np.ones_like(r2), np.zeros_like(r2)
        idx = np.arange(n)
        for b in range(3):                                   # the direction e_b of particle i: du = e_b exactly
            dd = tuple(one if c == b else zero for c in range(3))
            terms = _hvp_term_errors(d, dd, f, s, err_f, err_s, uu)
            for a, (err, mag) in enumerate(terms):
                h[a * n:(a + 1) * n, b * n:(b + 1) * n] = 2 * err
                h[a * n + idx, b * n + idx] = 2 * (err.sum(axis=1) + adds * uu * mag.sum(axis=1))
        return slack * h
    raise ValueError(kind)


def _hvp_term_errors(d, dd, f, s, err_f, err_s, uu):
    """[(err, |term|)] per component of the pair term f du_c + g d_c, g = 2 (overlap s): overlap's three products and two adds
    cost 5u of sum |d du| (differences u each, product u, adds u each); g: |s| of that + |overlap| err_s + |overlap s| u; the
    term: two products of rounded factors (2u each), the factors' own errors, and the addition (u)."""
    overlap = d[0] * dd[0] + d[1] * dd[1] + d[2] * dd[2]
    aover = np.abs(d[0] * dd[0]) + np.abs(d[1] * dd[1]) + np.abs(d[2] * dd[2])
    g = 2 * overlap * s
    err_g = 2 * (np.abs(s) * 5 * uu * aover + np.abs(overlap) * err_s + np.abs(overlap * s) * uu)
    out = []
    for dc, ddc in zip(d, dd):
        mag = np.abs(f * ddc) + np.abs(g * dc)
        err = np.abs(ddc) * err_f + np.abs(dc) * err_g + 2 * uu * mag + uu * np.abs(f * ddc + g * dc)
        out.append((err, mag))
    return out


# ------------------------------------------------------------------------------ fp64 forms for a minimiser
def energy_f64(p, rho):
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]; dz = z[:, None] - z[None, :]
    iu = np.triu_indices(n, 1)
    t = np.exp(rho * (1.0 - np.sqrt((dx * dx + dy * dy + dz * dz)[iu])))
    return float(np.sum(t * t - 2.0 * t))


def gradient_f64(p, rho):
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]; dz = z[:, None] - z[None, :]
    r = np.sqrt(dx * dx + dy * dy + dz * dz)
    np.fill_diagonal(r, 1.0)
    t = np.exp(rho * (1.0 - r))
    f = -rho * t * (t - 1.0) / r
    np.fill_diagonal(f, 0.0)
    return np.concatenate([2.0 * (f * d).sum(axis=1) for d in (dx, dy, dz)])


def minimize_f64(p, rho, max_steps=5000):
    """A local minimum below ``p`` in fp64: scipy's L-BFGS-B where scipy is importable, a plain numpy L-BFGS (history 10,
    backtracking on the energy) where it is not.  The callers polish the result with Newton steps."""
    try:
        from scipy.optimize import minimize
    except ImportError:
        minimize = None
    if minimize is not None:
        return minimize(energy_f64, p, args=(rho,), jac=gradient_f64, method="L-BFGS-B", options={"maxiter": max_steps, "ftol": 1e-16, "gtol": 1e-12}).x
    x, hist = np.asarray(p, dtype=np.float64).copy(), []
    e, g = energy_f64(x, rho), gradient_f64(x, rho)
    for _ in range(max_steps):
        if np.abs(g).max() <= 1e-11:
            break
        q, alphas = g.copy(), []
        for s_, y_ in reversed(hist):
            alphas.append((s_ @ q) / (s_ @ y_)); q -= alphas[-1] * y_
        if hist:
            q *= (hist[-1][0] @ hist[-1][1]) / (hist[-1][1] @ hist[-1][1])
        else:
            q *= 0.01
        for (s_, y_), a_ in zip(hist, reversed(alphas)):
            q += (a_ - (y_ @ q) / (s_ @ y_)) * s_
        d = -q if g @ q > 0 else -0.01 * g
        step = 1.0
        while step > 1e-20 and not energy_f64(x + step * d, rho) < e:
            step *= 0.5
        if step <= 1e-20:
            break
        xn = x + step * d
        en, gn = energy_f64(xn, rho), gradient_f64(xn, rho)
        if (xn - x) @ (gn - g) > 0:
            hist = (hist + [(xn - x, gn - g)])[-10:]
        x, e, g = xn, en, gn
    return x


@functools.lru_cache(maxsize=None)
def relaxed_icosahedron(rho):
    """The 13-atom icosahedron relaxed under Morse(rho) in fp64, polished by Newton steps on the twin's Hessian in the space
    orthogonal to its six zero modes: (point [x | y | z] as a tuple, energy)."""
    import pairwise_twin as lj
    p = np.concatenate(lj.icosahedron13())
    p = p / 1.08 * (0.98 if rho < 10 else 1.0)               # vertices about one pair distance from the centre
    p = minimize_f64(p, rho)
    for _ in range(4):
        h = hessian(p[:13], p[13:26], p[26:], rho).astype(np.float64)
        lam, vec = np.linalg.eigh(h)
        keep = np.abs(lam) > 1e-6 * np.abs(lam).max()
        g = gradient(p[:13], p[13:26], p[26:], rho).astype(np.float64).ravel()
        p = p - vec[:, keep] @ ((vec[:, keep].T @ g) / lam[keep])
    return tuple(p), float(energy(p[:13], p[13:26], p[26:], rho))
