"""CPU twin of the batched basin hopping as include/dzo.h states it: the draws of a hop from tempering_twin.pcg_raw, the jump
ahead in Python integers, the proposal and the sphere test in T, the quench of tests/quench_twin.py and the decision classes of
tempering_twin.classify.  A helper module for tests/test_basin_twin.py and tests/test_gpu_basin_hopping.py.  Not a conftest, no
fixtures.

The decision compares delta = E_q - E, ONE subtraction in T of two values the replay holds bit for bit, so the twin's delta is
the device's: the bound handed to ``classify`` is zero and only the rounding of exp(-beta * delta) in T can leave a hop
undecided (a band of a few ulp around the threshold).
"""
import numpy as np

import quench_twin as qt
import tempering_twin as tt

_M64 = (1 << 64) - 1
CODE_REJECTED, CODE_ACCEPTED, CODE_NOT_FINITE = 0, 1, 2


# ------------------------------------------------------------------------------ the stream
def pcg_jump(state, k):
    """The state after k advances: s' = A_k s + C_k (mod 2^64), the affine map built by squaring from the bits of k."""
    a_k, c_k = 1, 0
    a, c = tt._MUL, tt._INC
    while k:
        if k & 1:
            a_k, c_k = (a_k * a) & _M64, (c_k * a + c) & _M64
        c = (c * (a + 1)) & _M64
        a = (a * a) & _M64
        k >>= 1
    return (a_k * state + c_k) & _M64


def draws_per_hop(n):
    return 4 * n + 1


def hop_draws(state, n, dtype, with_radii=False):
    """(normals (n, 3) of dtype by numpy's fp64 Box-Muller, u of dtype, the state after the hop): particle i takes draws
    4i .. 4i+3 as d1 .. d4 of the tempering rule, draw 4n is the acceptance uniform.  ``with_radii``: also the Box-Muller radii
    sqrt(-2 log u) behind each normal, (n, 3), which the error bound of a device normal needs."""
    raw, after = tt.pcg_raw(state, draws_per_hop(n))
    d = raw[:4 * n].astype(np.uint64).reshape(n, 4)
    nx, ny, r1 = tt.box_muller_f64(d[:, 0], d[:, 1])
    nz, _, r2 = tt.box_muller_f64(d[:, 2], d[:, 3])
    u = np.dtype(dtype).type(float(raw[4 * n]) * 2.0 ** -32)
    normals = np.stack([nx, ny, nz], axis=1).astype(dtype)
    return (normals, u, after, np.stack([r1, r1, r2], axis=1)) if with_radii else (normals, u, after)


# ------------------------------------------------------------------------------ pieces of one hop
def trial(point, radius, normals, constraining_radius, dtype):
    """The trial of the point [x | y | z]: old + radius * n per coordinate (a product and a sum in T); a particle whose trial
    position fails x^2 + y^2 + z^2 < R^2 (in T, left to right) keeps its old position.  Returns (trial, moved (n,) bool)."""
    t = np.dtype(dtype).type
    old = np.asarray(point, dtype=dtype).reshape(3, -1)
    nrm = np.asarray(normals, dtype=dtype)
    R = t(constraining_radius)
    with np.errstate(all="ignore"):
        new = old + t(radius) * nrm.T
        inside = new[0] * new[0] + new[1] * new[1] + new[2] * new[2] < R * R
    return np.where(inside[None, :], new, old).reshape(-1), inside


def decide(e_q, e, u, beta, dtype):
    """(class the device must be in, the twin's own code from a longdouble exp)"""
    t = np.dtype(dtype).type
    if not np.isfinite(e_q):
        return tt.MUST_REJECT, CODE_NOT_FINITE
    with np.errstate(all="ignore"):
        delta = t(e_q) - t(e)
    klass = tt.classify(delta, 0, u, t(beta), dtype)
    if not np.isfinite(delta):
        klass = tt.MUST_ACCEPT if delta < 0 else tt.MUST_REJECT      # -inf is accepted; +inf and NaN fail both comparisons
    with np.errstate(all="ignore"):
        own = bool(delta <= 0 or tt.LD(u) <= np.exp(-tt.LD(t(beta)) * tt.LD(delta)))
    return klass, CODE_ACCEPTED if own else CODE_REJECTED


def quench(point, initial_step_length, history_length, quench_steps, dtype, max_halvings=4096):
    q = qt.Quench(point, initial_step_length, history_length, dtype, max_halvings)
    q.run(quench_steps)
    return q


# ------------------------------------------------------------------------------ a walker on the twin's own decisions
class Walker:
    """One walker: ``hop()`` appends to ``log`` a dict with the draws, the trial, the quench's outcome and the decision."""

    def __init__(self, point, beta, radius, constraining_radius, seed, initial_step_length=0.01, history_length=10, quench_steps=400,
                 dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.n = len(point) // 3
        self.beta, self.radius, self.R = self.dtype.type(beta), self.dtype.type(radius), constraining_radius
        self.quench_args = (initial_step_length, history_length, quench_steps, self.dtype)
        self.state = tt.pcg_state(seed)
        q = quench(np.asarray(point, dtype=self.dtype), *self.quench_args)       # no draws, always kept
        self.x, self.e = q.x.copy(), q.f
        self.best_x, self.best_e = q.x.copy(), q.f
        self.num_accept = self.num_reject = self.hops = self.iterations = self.unfinished = 0
        self.log = []

    def hop(self):
        normals, u, after = hop_draws(self.state, self.n, self.dtype)
        tr, moved = trial(self.x, self.radius, normals, self.R, self.dtype)
        q = quench(tr, *self.quench_args)
        klass, code = decide(q.f, self.e, u, self.beta, self.dtype)
        self.log.append(dict(state=self.state, after=after, normals=normals, u=u, trial=tr, moved=moved, x_q=q.x.copy(), e_q=q.f,
                             iterations=q.iteration_count, stuck=q.is_stuck, klass=klass, code=code, e_before=self.e))
        self.state = after
        if code == CODE_ACCEPTED:
            self.x, self.e = q.x.copy(), q.f
        if np.isfinite(q.f) and q.f < self.best_e:
            self.best_x, self.best_e = q.x.copy(), q.f
        self.num_accept += code == CODE_ACCEPTED
        self.num_reject += code != CODE_ACCEPTED
        self.hops += 1
        self.iterations += q.iteration_count
        self.unfinished += not q.is_stuck
        return self
