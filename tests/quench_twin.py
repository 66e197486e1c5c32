"""CPU twin of the batched L-BFGS quench: a numpy restatement of the live LBFGSOptimizer of src/DZOptimization.jl
(take_backtracking_step! :107-154, the constructor :381-387, compute_lbfgs_step_direction! :430-451, step! :454-509) with
constraint_function! = nothing, on the Lennard-Jones energy and gradient of tests/pairwise_twin.py.  A helper module for
tests/test_quench_twin.py (which pins it against things it does not depend on) and tests/test_gpu_quench.py (which holds the
device kernels to it).  Not a conftest, no fixtures.

Element type: every vector operation is done in `dtype`; dots accumulate in fp64 and alpha, beta and the scale are rounded to
`dtype`, which is the library's rule for fp32.  rho holds s.y itself (fp64).  The history lists are newest first.
"""
import numpy as np

import pairwise_twin as tw

LD = np.longdouble
U = {np.dtype(np.float64): LD(2.0) ** -53, np.dtype(np.float32): LD(2.0) ** -24}


# ------------------------------------------------------------------------------ objective
def energy_gradient(p, dtype=np.float64):
    """(E, g) of the point p = [x | y | z].  fp64: the fp64 forms of pairwise_twin.  fp32: the same formulas with every
    operation in fp32 (rows summed over j in order, rows added in fp64, one rounding)."""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        p = np.asarray(p, dtype=np.float64)
        with np.errstate(all="ignore"):
            return np.float64(tw.energy_f64(p)), tw.gradient_f64(p)
    t = dtype.type
    p = np.asarray(p, dtype=dtype)
    n = len(p) // 3
    x, y, z = p[:n], p[n:2 * n], p[2 * n:]
    with np.errstate(all="ignore"):
        dx = x[:, None] - x[None, :]; dy = y[:, None] - y[None, :]; dz = z[:, None] - z[None, :]
        r2 = dx * dx + dy * dy + dz * dz
        inv_r2 = t(1) / r2
        inv_r4 = inv_r2 * inv_r2
        inv_r6 = inv_r4 * inv_r2
        inv_r8 = inv_r4 * inv_r4
        e = t(4) * (inv_r6 * inv_r6 - inv_r6)
        f = t(-12) * (inv_r8 * (inv_r6 + inv_r6) - inv_r8)
        eye = np.eye(n, dtype=bool)
        e = np.where(eye, t(0), e); f = np.where(eye, t(0), f)
        row = np.zeros(n, dtype=dtype); a = np.zeros((3, n), dtype=dtype)
        for j in range(n):
            row = row + e[:, j]
            a[0] = a[0] + f[:, j] * dx[:, j]; a[1] = a[1] + f[:, j] * dy[:, j]; a[2] = a[2] + f[:, j] * dz[:, j]
        E = t(0.5 * np.sum(row.astype(np.float64)))
        return E, (a + a).reshape(-1)


def exact_energy(p):
    """(E, S) in longdouble (pairwise_twin.energy) of a point [x | y | z]."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p) // 3
    return tw.energy(p[:n], p[n:2 * n], p[2 * n:])


def _dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


# ------------------------------------------------------------------------------ the recursion, :430-451
def direction(g, S, Y, rho, dtype=np.float64):
    """compute_lbfgs_step_direction! on explicit lists (newest first)."""
    t = np.dtype(dtype).type
    d = np.array(g, dtype=dtype)
    k = len(S)
    alpha = [t(0)] * k
    with np.errstate(all="ignore"):
        for i in range(k):
            alpha[i] = t(_dot(S[i], d) / rho[i])                 # :440
            d = d - alpha[i] * Y[i]                              # :441
        if k:
            d = d * t(-(rho[0] / _dot(Y[0], Y[0])))              # :444
        for i in reversed(range(k)):
            beta = t(_dot(Y[i], d) / rho[i])                     # :447
            d = d - (alpha[i] + beta) * S[i]                     # :448
    return d


def direction_dense(g, S, Y, rho):
    """-H g with H the dense inverse BFGS update of gamma I by the pairs, oldest first (fp64): what the two loops compute."""
    n = len(g)
    k = len(S)
    if k == 0:
        return np.array(g, dtype=np.float64)
    H = (rho[0] / _dot(Y[0], Y[0])) * np.eye(n)
    I = np.eye(n)
    for i in reversed(range(k)):
        s, y = S[i].astype(np.float64), Y[i].astype(np.float64)
        V = I - np.outer(y, s) / rho[i]
        H = V.T @ H @ V + np.outer(s, s) / rho[i]
    return -(H @ np.asarray(g, dtype=np.float64))


# ------------------------------------------------------------------------------ the optimizer
class Quench:
    """One instance of the live LBFGSOptimizer.  `trials` of the last step: [(h, f_trial)], the accepted one last."""

    def __init__(self, p0, initial_step_length=0.01, history_length=10, dtype=np.float64, max_halvings=4096):
        self.dtype = np.dtype(dtype)
        self.t = self.dtype.type
        self.m = int(history_length)
        self.max_halvings = int(max_halvings)
        self.x = np.array(p0, dtype=self.dtype)
        self.f, self.g = energy_gradient(self.x, self.dtype)
        self.g = np.asarray(self.g, dtype=self.dtype)
        with np.errstate(all="ignore"):
            norm = np.sqrt(_dot(self.g, self.g))                 # :381
            self.is_stuck = norm == 0.0                          # :382
            self.d = np.zeros_like(self.x) if self.is_stuck else self.g * self.t(-(initial_step_length / norm))   # :384-387
        self.dx = np.zeros_like(self.x); self.dg = np.zeros_like(self.x)
        self.df = self.t(0)
        self.iteration_count = 0
        self.S, self.Y, self.rho = [], [], []
        self.last_halvings = 0
        self.trials = []

    def step(self):
        if self.is_stuck:                                        # :456
            return self
        t = self.t
        if self.iteration_count > 0:                             # :463
            self.d = direction(self.g, self.S, self.Y, self.rho, self.dtype)
        x_old = self.x.copy()                                    # :118
        step_size, h = t(1), 0
        self.trials = []
        while True:
            with np.errstate(all="ignore"):
                x_new = x_old + step_size * self.d               # :124 (2^-h d is exact: the same bits as a fused multiply-add)
            if np.array_equal(x_new, x_old, equal_nan=True):     # :128
                self.is_stuck = True
                self.dx = x_old
                self.last_halvings = h
                return self
            f_new, g_new = energy_gradient(x_new, self.dtype)
            self.trials.append((h, f_new))
            if f_new < self.f:                                   # :139
                break
            step_size = step_size * t(0.5)                       # :152
            h += 1
            if h >= self.max_halvings:
                self.is_stuck = True
                self.dx = x_old
                self.last_halvings = h
                return self
        self.last_halvings = h
        self.df = f_new - self.f; self.f = f_new                 # :142-144
        self.x = x_new
        self.dx = x_new - x_old                                  # :145
        g_new = np.asarray(g_new, dtype=self.dtype)
        self.dg = g_new - self.g                                 # :478-480
        self.g = g_new
        self.S.insert(0, self.dx.copy()); self.Y.insert(0, self.dg.copy())   # :482-496
        self.rho.insert(0, _dot(self.dx, self.dg))               # :505
        del self.S[self.m:], self.Y[self.m:], self.rho[self.m:]
        self.iteration_count += 1                                # :507
        return self

    def run(self, max_steps=2000):
        k = 0
        while k < max_steps and not self.is_stuck:
            self.step()
            k += 1
        return k


# ------------------------------------------------------------------------------ decisions
def decision_margin(x_old, x_new, dtype, old=None):
    """(E_new - E_old, bound) in longdouble with bound = (N + 32) u (S_old + S_new): a trial whose |difference| is within the
    bound is one an evaluation correct to the derived error bound may decide either way.  `old`: exact_energy(x_old), where the
    caller has it from an earlier trial of the same step."""
    n = len(x_old) // 3
    e0, s0 = exact_energy(x_old) if old is None else old
    e1, s1 = exact_energy(x_new)
    return e1 - e0, LD(n + 32) * U[np.dtype(dtype)] * (s0 + s1)


def start(name, seed, dtype=np.float64):
    """The starts of the quench tests: the jittered icosahedron / octahedron of pairwise_twin, or a disordered 38-atom blob."""
    if name == "ico":
        return np.asarray(np.concatenate(tw.jittered(tw.icosahedron13(), seed)), dtype=dtype)
    if name == "oct":
        return np.asarray(np.concatenate(tw.jittered(tw.octahedron38(), seed)), dtype=dtype)
    assert name == "blob"
    return np.asarray(np.concatenate(tw.jittered(tw.octahedron38(), 100 + seed, jitter=0.25)), dtype=dtype)
