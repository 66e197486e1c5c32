"""CPU twin of the Thomson problem on the device (csrc/dzo_sphere.hip): the Riesz (Coulomb, s = 1) energy of N points on the unit
sphere and the live LBFGSOptimizer with the unit sphere as its constraint_function! (src/DZOptimization.jl:107-154 with the hook
of :133-135, the constructor's projection :412-414).  A helper module for tests/test_sphere_twin.py (which pins it against
things it does not depend on) and tests/test_gpu_sphere.py (which holds the device kernels to it).  Not a conftest, no fixtures.

A point is [x | y | z] (3N values), the layout of every cluster unit; the legacy functions of legacy/ExampleFunctions.jl take a
(3, N) matrix, and the literal restatements below keep that.

Energy and gradient come three ways: in longdouble with the sum S of the absolute values of the terms (the method of
pairwise_twin), in T in the device's order, and as literal restatements of riesz_energy (:30-45), riesz_gradient! (:47-83) and
constrain_riesz_gradient_sphere! (:361-374).
"""
import numpy as np

import quench_twin as qt

LD = np.longdouble
U = qt.U
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = [np.float64, np.float32]


# ------------------------------------------------------------------------------ the two hooks, operation for operation
def project(p, dtype=np.float64):
    """constraint_function!: every particle of [x | y | z] divided by its norm; r = sqrt((x x + y y) + z z), three divisions,
    every operation one rounding in T."""
    p = np.asarray(p, dtype=dtype)
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z)
        return np.concatenate([x / r, y / r, z / r])


def tangent(p, g, dtype=np.float64):
    """constrain_riesz_gradient_sphere!: overlap = (x gx + y gy) + z gz, g - overlap p, unfused, in T."""
    p = np.asarray(p, dtype=dtype); g = np.asarray(g, dtype=dtype)
    n = len(p) // 3
    with np.errstate(all="ignore"):
        overlap = (p[:n] * g[:n] + p[n:2 * n] * g[n:2 * n]) + p[2 * n:] * g[2 * n:]
        return g - np.tile(overlap, 3) * p


# ------------------------------------------------------------------------------ in T, in the device's order
def pair_terms(p, dtype=np.float64):
    """(e, f, dx, dy, dz) as (N, N) arrays in T: the functor RieszRadial on r2 = (dx dx + dy dy) + dz dz; the diagonal is zero."""
    t = np.dtype(dtype).type
    p = np.asarray(p, dtype=dtype)
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    with np.errstate(all="ignore"):
        dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]; dz = z[:, None] - z[None, :]
        r2 = (dx * dx + dy * dy) + dz * dz
        inv_r = t(1) / np.sqrt(r2)
        e = inv_r
        f = t(-0.5) * (inv_r / r2)
        eye = np.eye(n, dtype=bool)
        return np.where(eye, t(0), e), np.where(eye, t(0), f), dx, dy, dz


def energy_gradient(p, dtype=np.float64, constrained=True):
    """(E, g) of the point as it is (not projected): rows summed over j ascending in T, rows added in fp64, one rounding; the
    gradient raw (riesz_gradient!) or tangent."""
    dtype = np.dtype(dtype)
    t = dtype.type
    p = np.asarray(p, dtype=dtype)
    n = len(p) // 3
    e, f, dx, dy, dz = pair_terms(p, dtype)
    with np.errstate(all="ignore"):
        row = np.zeros(n, dtype=dtype); a = np.zeros((3, n), dtype=dtype)
        for j in range(n):
            row = row + e[:, j]
            a[0] = a[0] + f[:, j] * dx[:, j]; a[1] = a[1] + f[:, j] * dy[:, j]; a[2] = a[2] + f[:, j] * dz[:, j]
        E = t(0.5 * np.sum(row.astype(np.float64)))
        g = (a + a).reshape(-1)
    return E, (tangent(p, g, dtype) if constrained else g)


# ------------------------------------------------------------------------------ in longdouble, with S
def exact(p, block=128, gradient=True):
    """(E, S, g, Srow) of a point [x | y | z] in longdouble: E = sum_{i<j} 1/r, S the same sum of absolute values (= E here:
    every term is positive); g (3, N) the raw gradient, Srow[i] = sum_j |term_ij| (the norms of the row's vector terms).
    Without `gradient` the last two stay zero."""
    p = np.asarray(p, dtype=LD)
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    E = LD(0); g = np.zeros((3, n), dtype=LD); Srow = np.zeros(n, dtype=LD)
    with np.errstate(all="ignore"):
        for a in range(0, n, block):
            r = np.arange(a, min(n, a + block))
            dx = x[r, None] - x[None, :]; dy = y[r, None] - y[None, :]; dz = z[r, None] - z[None, :]
            r2 = dx * dx + dy * dy + dz * dz
            self_ = r[:, None] == np.arange(n)[None, :]
            inv_r = np.where(self_, LD(0), LD(1) / np.sqrt(r2))
            E += inv_r.sum()
            if not gradient:
                continue
            c = np.where(self_, LD(0), inv_r / np.where(self_, LD(1), r2))     # 1 / r^3
            g[0, r] = -(c * dx).sum(axis=1); g[1, r] = -(c * dy).sum(axis=1); g[2, r] = -(c * dz).sum(axis=1)
            Srow[r] = (c * np.sqrt(r2)).sum(axis=1)
    E = LD(0.5) * E
    return E, E, g, Srow


def exact_energy(p):
    E, S, _, _ = exact(p, gradient=False)
    return E, S


def exact_tangent(p, g):
    """constrain_riesz_gradient_sphere! of a (3, N) gradient in longdouble."""
    p = np.asarray(p, dtype=LD).reshape(3, -1)
    return g - (p * g).sum(axis=0)[None, :] * p


# ------------------------------------------------------------------------------ the legacy functions, literally, on (3, N)
def legacy_energy(points):
    """riesz_energy, :30-45; rsqrt(d) is 1 / sqrt(d)."""
    t = points.dtype.type
    dimension, num_points = points.shape
    result = t(0)
    for j in range(1, num_points):
        for i in range(j):
            dist_sq = t(0)
            for k in range(dimension):
                dist = points[k, i] - points[k, j]
                dist_sq += dist * dist
            result += t(1) / np.sqrt(dist_sq)
    return result


def legacy_gradient(points, terms=None):
    """riesz_gradient!, :47-83.  `terms`: a dict that receives every dist * inv_dist_cubed as terms[(k, i, j)]."""
    t = points.dtype.type
    dimension, num_points = points.shape
    gradient = np.zeros_like(points)
    for j in range(num_points):
        for i in list(range(j)) + list(range(j + 1, num_points)):
            dist_sq = t(0)
            for k in range(dimension):
                dist = points[k, i] - points[k, j]
                dist_sq += dist * dist
            inv_dist = t(1) / np.sqrt(dist_sq)
            inv_dist_cubed = inv_dist / dist_sq
            for k in range(dimension):
                dist = points[k, i] - points[k, j]
                term = dist * inv_dist_cubed
                if terms is not None:
                    terms[(k, i, j)] = term
                gradient[k, j] += term
    return gradient


def legacy_constrain(grad, points):
    """constrain_riesz_gradient_sphere!, :361-374, in place."""
    t = points.dtype.type
    dim, num_points = points.shape
    for i in range(num_points):
        overlap = t(0)
        for k in range(dim):
            overlap += points[k, i] * grad[k, i]
        for k in range(dim):
            grad[k, i] -= overlap * points[k, i]
    return grad


# ------------------------------------------------------------------------------ derived bounds
# Energy.  The point is exact in T.  A term 1 / r: each difference one rounding (1 u), its square 2 u from the difference and 1 u
# of its own (3 u), the two additions of r2 one each, the first two squares passing through both: r2 within 5 u (relative; all
# terms positive); the square root halves that and adds its own: 3.5 u; the division: 4.5 u.  A row of N - 1 positive terms summed
# in order: at most N - 2 more on any term.  Rows in fp64 (a tree of at most 10 levels, in fp64: below one u of fp32, at most 10 u
# in fp64), the exact halving, one rounding to T.  Together at most (N - 2 + 4.5 + 10 + 1) u S = (N + 13.5) u S; second-order
# terms (at most (N + 14)^2 u^2, below u up to N = 1024 in fp32 and far below in fp64) are covered by c(N) = N + 16.
# Raw gradient, per component of row i, against Srow_i = sum_j |term_ij|: inv_r within 4.5 u, inv_r / r2: 4.5 + 5 + 1 = 10.5 u,
# the exact scaling, times the difference (one rounding) with one rounding: 12.5 u; N - 2 for the row's sum; the exact doubling:
# (N + 10.5) u Srow, again within c(N) = N + 16.
# Tangent gradient g - (p . g) p with |p|^2 within 8 u of one (below): an error delta of the raw gradient (each component at most
# c u Srow, its norm at most sqrt(3) of that) passes as delta - (p . delta) p, at most (1 + sqrt(3)) c u Srow per component; the
# overlap's five roundings add at most 3 u |g| |p_c|, the product and the subtraction 2 u (|g_c| + |g|); |g| <= sqrt(3) Srow.
# Together below (2.74 c + 12.2) u Srow <= (3 c + 13) u Srow.
def c_of(n):
    return LD(n + 16)


def bound_energy(n, dtype, S):
    return c_of(n) * U[np.dtype(dtype)] * S


def bound_gradient(n, dtype, Srow, constrained=True):
    c = LD(3) * c_of(n) + LD(13) if constrained else c_of(n)
    return c * U[np.dtype(dtype)] * Srow


# One normalisation.  r2 = (x x + y y) + z z: a square one rounding, two additions: within 3 u; r = sqrt(r2): 1.5 u + 1 u; each
# quotient one more: every component within 3.5 u of p_c / |p|, so |p|^2 within 7 u (+ second order) of one: 8 u.
def bound_norm(dtype):
    return LD(8) * U[np.dtype(dtype)]


# One tangent.  With o = p . g exactly, the stored gradient is g_c - o' p_c (1 + d1) rounded once more (d2), o' within 3 u A of o,
# A = sum |p_c g_c| <= |g|.  Then p . g_stored = o (1 - |p|^2) - (o' - o) |p|^2 + sum p_c (d1 o' p_c + d2 g_stored_c), at most
# u (8 |o| + 3 A + |o| + |g_stored|) (1 + 8 u) <= 13 u |g| + second order: 14 u |g|, |g| the norm of the particle's RAW gradient.
def bound_overlap(dtype, raw_norm):
    return LD(14) * U[np.dtype(dtype)] * raw_norm


def decision_margin(x_old, x_new, dtype, old=None):
    """(E_new - E_old, bound) in longdouble, bound = c(N) u (S_old + S_new): see quench_twin.decision_margin."""
    n = len(x_old) // 3
    e0, s0 = exact_energy(x_old) if old is None else old
    e1, s1 = exact_energy(x_new)
    return e1 - e0, bound_energy(n, dtype, s0 + s1)


# ------------------------------------------------------------------------------ the optimizer
class SphereQuench(qt.Quench):
    """quench_twin.Quench with the two hooks: the initial point and every trial are projected, every gradient is tangent.  The
    stuck test sees the unprojected trial (:128 comes before :133).  `trials` of the last step: [(h, f_trial)]."""

    def __init__(self, p0, initial_step_length=0.01, history_length=10, dtype=np.float64, max_halvings=4096):
        self.dtype = np.dtype(dtype)
        self.t = self.dtype.type
        self.m = int(history_length)
        self.max_halvings = int(max_halvings)
        self.x = project(np.array(p0, dtype=self.dtype), self.dtype)             # :412-414
        self.f, self.g = energy_gradient(self.x, self.dtype)
        with np.errstate(all="ignore"):
            norm = np.sqrt(qt._dot(self.g, self.g))                                # :381
            self.is_stuck = norm == 0.0
            self.d = np.zeros_like(self.x) if self.is_stuck else self.g * self.t(-(initial_step_length / norm))
        self.dx = np.zeros_like(self.x); self.dg = np.zeros_like(self.x)
        self.df = self.t(0)
        self.iteration_count = 0
        self.S, self.Y, self.rho = [], [], []
        self.last_halvings = 0
        self.trials = []

    def step(self):
        if self.is_stuck:
            return self
        t = self.t
        if self.iteration_count > 0:
            self.d = qt.direction(self.g, self.S, self.Y, self.rho, self.dtype)
        x_old = self.x.copy()
        step_size, h = t(1), 0
        self.trials = []
        while True:
            with np.errstate(all="ignore"):
                x_new = x_old + step_size * self.d                                 # :124
            stuck = np.array_equal(x_new, x_old, equal_nan=True)                   # :128, on the unprojected trial
            if not stuck:
                x_new = project(x_new, self.dtype)                                 # :133-135
                f_new, g_new = energy_gradient(x_new, self.dtype)
                self.trials.append((h, f_new))
                if f_new < self.f:                                                 # :139
                    break
                step_size = step_size * t(0.5)
                h += 1
                stuck = h >= self.max_halvings
            if stuck:
                self.is_stuck = True
                self.dx = x_old
                self.last_halvings = h
                return self
        self.last_halvings = h
        self.df = f_new - self.f; self.f = f_new
        self.x = x_new
        self.dx = x_new - x_old
        self.dg = g_new - self.g
        self.g = g_new
        self.S.insert(0, self.dx.copy()); self.Y.insert(0, self.dg.copy())
        self.rho.insert(0, qt._dot(self.dx, self.dg))
        del self.S[self.m:], self.Y[self.m:], self.rho[self.m:]
        self.iteration_count += 1
        return self


# ------------------------------------------------------------------------------ closed forms
PHI = (1.0 + np.sqrt(5.0)) / 2.0


def closed_form(n):
    """(points (3, N) in longdouble on the unit sphere, energy in longdouble) of the minimum for N = 2, 3, 4, 6, 12."""
    s = np.sqrt
    if n == 2:
        pts, E = [(0, 0, 1), (0, 0, -1)], LD(1) / 2
    elif n == 3:
        pts, E = [(1, 0, 0), (-LD(1) / 2, s(LD(3)) / 2, 0), (-LD(1) / 2, -s(LD(3)) / 2, 0)], s(LD(3))
    elif n == 4:
        pts, E = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], 3 * s(LD(6)) / 2
    elif n == 6:
        pts, E = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], 12 / s(LD(2)) + LD(3) / 2
    else:
        assert n == 12
        phi = (1 + s(LD(5))) / 2
        pts = [p for a in (1, -1) for b in (phi, -phi) for p in ((0, a, b), (a, b, 0), (b, 0, a))]
        E = None
    P = np.array(pts, dtype=LD).T
    P = P / np.sqrt((P * P).sum(axis=0))[None, :]
    if E is None:
        E = exact_energy(P.reshape(-1))[0]
    return P, E


E_ICOSAHEDRON = closed_form(12)[1]
CLOSED_N = (2, 3, 4, 6, 12)


# ------------------------------------------------------------------------------ the GPU tests' inputs
# (N, history_length); every case runs in both element types.  The paths are those of quench_checks.path.
CASES = [(2, 1), (3, 2), (4, 3), (12, 10), (61, 2), (63, 32), (64, 1),      # wave: smallest first; dropped padding pairs; full
         (65, 2), (256, 2), (257, 1), (513, 3),                             # block
         (97, 32), (98, 32),                                                # fp64: last in LDS / first in the slab
         (195, 32), (196, 32),                                              # fp32: last in LDS / first in the slab
         (1024, 1)]                                                         # largest
STEP = 0.01


def batch_of(n):
    return 3 if n < 513 else 2


def start(n, seed, dtype):
    """Random points on the sphere: Gaussian vectors of a seeded generator, projected on the host by the twin."""
    g = np.random.default_rng(1000 * n + seed).standard_normal(3 * n)
    return project(np.asarray(g, dtype=dtype), dtype)


def starts(n, dtype):
    return np.stack([start(n, s, dtype) for s in range(batch_of(n))])


def jittered(n, seed, dtype, jitter=0.05):
    """A closed form with every coordinate moved by a uniform draw of [-jitter, jitter), projected by the twin."""
    P = closed_form(n)[0].astype(np.float64).reshape(-1)
    P = P + np.random.default_rng(7000 * n + seed).uniform(-jitter, jitter, 3 * n)
    return project(np.asarray(P, dtype=dtype), dtype)


def random_starts(n, count, seed, dtype):
    g = np.random.default_rng(seed).standard_normal((count, 3 * n))
    return np.stack([project(np.asarray(r, dtype=dtype), dtype) for r in g])


# Minima.  Sixteen jittered copies (seeds 0..15) of each closed form, history 10, step 0.01, run to is_stuck by the twin: the
# worst of |E - closed form| over the stored objective and the longdouble energy of the final point, measured on the CPU
# (tests/test_sphere_twin.py::test_twin_reaches_the_minima repeats it).  The GPU test allows four times this, and at least
# the bound of one evaluation, bound_energy(N, T, E).  Every entry is below that floor, so the floor decides.
TWIN_WORST_CLOSED = {(2, F64): 7.94e-17, (3, F64): 5.45e-16, (4, F64): 7.70e-16, (6, F64): 2.53e-15, (12, F64): 1.24e-14,
                     (2, F32): 4.48e-8, (3, F32): 2.70e-7, (4, F32): 2.24e-7, (6, F32): 1.34e-6, (12, F32): 4.19e-6}
# Sixteen random starts, random_starts(N, 16, RANDOM_SEED, T): the twin brings all sixteen to the lowest energy (N = 12: the
# icosahedron's; N = 32: the twin's own lowest in fp64, 412.2612746505...).  The worst |E - lowest| of the twin, as above.
RANDOM_SEED = 1
E_LOWEST_32 = LD("412.26127465052930554")
TWIN_WORST_RANDOM = {(12, F64): 1.3e-14, (32, F64): 2.3e-13, (12, F32): 9.5e-6, (32, F32): 3.1e-5}


def tol_minimum(n, dtype, E, worst):
    return max(LD(4) * LD(worst), bound_energy(n, dtype, E))


def steps_before_the_second_look(n):
    return 1 if n <= 4 else 6


def window(n, dtype):
    """Steps from the start in which no trial may be undecided (tests/test_sphere_twin.py shows the twin alone meets it)."""
    f64 = np.dtype(dtype) == F64
    if n <= 4:
        return 3 if f64 else 2
    if n >= 513:
        return 3 if f64 else 2
    return 8 if f64 else 4
