"""CPU twin of the batched AdGD optimizer (dzo_adgd_batch_*): a numpy restatement of the live AdGDOptimizer of
src/DZOptimization.jl (the constructor :229-241, step! :274-312, take_backtracking_step! :107-154) with constraint_function! =
nothing, on the Lennard-Jones energy and gradient of tests/quench_twin.py -- the arithmetic include/dzo.h states for the handle.
A helper module for tests/test_adgd_batch_twin.py (which pins it against things it does not depend on) and
tests/test_gpu_adgd_batch.py (which holds the device kernels to it).  Not a conftest, no fixtures.

Element type: every operation of the step-size rule is done in `dtype` (IEEE division and square root); the sums of squares
accumulate in fp64 and are rounded to `dtype` once.  The trial point is one fused multiply-add per element
(pairwise_twin.fma, exact and rounded once).

It also holds the inputs the GPU tests run on (starts, seeds, step lengths, decision windows), so that
tests/test_adgd_batch_twin.py can show on the CPU what the GPU tests assume about them.
"""
import numpy as np

import pairwise_twin as tw
import quench_twin as qt

LD = np.longdouble
U = qt.U
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)


def fma(a, b, c, dtype):
    """a * b[k] + c[k] for every k, ONE rounding to dtype each (a scalar, b and c vectors)."""
    return np.array([tw.fma(a, bk, ck, dtype) for bk, ck in zip(b, c)], dtype=dtype)


def sum_of_squares(v):
    """sum v^2 in fp64"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.dot(v, v))


# ------------------------------------------------------------------------------ the step-size rule, :285-295
def step_size_candidates(dx, dg, current, previous, dtype):
    """(grown, cap) in dtype: current sqrt(1 + current / previous) of :290-291 and sqrt(1/2) |dx| / |dg| of :292-295 (None where
    |dg| is zero).  next_step_size is the smaller one."""
    t = np.dtype(dtype).type
    current, previous = t(current), t(previous)
    with np.errstate(all="ignore"):
        theta = current / previous                               # :290
        grown = current * np.sqrt(t(1) + theta)                  # :291
        dgn = np.sqrt(t(sum_of_squares(dg)))                     # :292
        if dgn == 0:                                             # :293
            return grown, None
        inv_l = np.sqrt(t(sum_of_squares(dx))) / dgn             # :294
        return grown, np.sqrt(t(0.5)) * inv_l


def next_step_size(dx, dg, current, previous, dtype):
    grown, cap = step_size_candidates(dx, dg, current, previous, dtype)
    return grown if cap is None or grown < cap else cap          # :295, as `grown < cap ? grown : cap`


# ------------------------------------------------------------------------------ the optimizer
class AdGD:
    """One instance of the live AdGDOptimizer.  `trials` of the last step: [(h, f_trial)], the accepted one last."""

    def __init__(self, p0, initial_step_length=0.01, dtype=np.float64, max_halvings=4096):
        self.dtype = np.dtype(dtype)
        self.t = t = self.dtype.type
        self.max_halvings = int(max_halvings)
        self.x = np.array(p0, dtype=self.dtype)
        self.f, g = qt.energy_gradient(self.x, self.dtype)
        self.g = np.asarray(g, dtype=self.dtype)
        with np.errstate(all="ignore"):
            ss = sum_of_squares(self.g)                          # :230
            self.is_stuck = ss == 0.0                            # :231
            s0 = t(0) if self.is_stuck else t(initial_step_length) / t(np.sqrt(ss))   # :232-233
        self.current_step_size = self.previous_step_size = s0    # :241
        self.dx = np.zeros_like(self.x); self.dg = np.zeros_like(self.x)
        self.df = t(0)
        self.iteration_count = 0
        self.last_halvings = 0
        self.trials = []

    def step(self):
        if self.is_stuck:                                        # :276
            return self
        t = self.t
        nxt = self.current_step_size                             # :287
        if self.iteration_count > 0:                             # :288
            nxt = next_step_size(self.dx, self.dg, self.current_step_size, self.previous_step_size, self.dtype)
        self.previous_step_size, self.current_step_size = self.current_step_size, nxt   # :298-299
        x_old = self.x.copy()                                    # :118
        step_size, h = t(nxt), 0
        self.trials = []
        while True:
            x_new = fma(-step_size, self.g, x_old, self.dtype)   # :124
            if np.array_equal(x_new.view(np.uint8), x_old.view(np.uint8)):   # isequal, :128
                self.is_stuck = True
                break
            f_new, g_new = qt.energy_gradient(x_new, self.dtype)
            self.trials.append((h, f_new))
            if f_new < self.f:                                   # :139
                break
            with np.errstate(all="ignore"):
                step_size = step_size * t(0.5)                   # :152
            h += 1
            if h >= self.max_halvings:
                self.is_stuck = True
                break
        self.last_halvings = h
        if self.is_stuck:
            self.dx = x_old                                      # the copy of :118 stays
            return self
        self.df = f_new - self.f; self.f = f_new                 # :142-144
        self.x = x_new
        self.dx = x_new - x_old                                  # :145
        g_new = np.asarray(g_new, dtype=self.dtype)
        self.dg = g_new - self.g                                 # :306-308
        self.g = g_new
        self.iteration_count += 1                                # :310
        return self

    def run(self, max_steps=5000):
        k = 0
        while k < max_steps and not self.is_stuck:
            self.step()
            k += 1
        return k


# ------------------------------------------------------------------------------ the inputs of the GPU tests
NS = [13, 38, 200]                                               # WAVE, WAVE, BLOCK
SEEDS = range(4)
# step length -> steps from the start in which no trial may be undecided, per element type.  Length 1.0 overshoots at the first
# step (the halving path); 0.01 is the quench's.
WINDOWS = {0.01: {F64: 20, F32: 5}, 1.0: {F64: 10, F32: 5}}


def start(n, seed, dtype):
    """The starts of the quench's GPU tests: jittered icosahedron (13), octahedron (38), else the jittered cubic lattice."""
    if n == 13:
        return qt.start("ico", seed, dtype)
    if n == 38:
        return qt.start("oct", seed, dtype)
    return np.asarray(np.concatenate(tw.lattice(n, seed=seed)), dtype=dtype)


def starts(n, seeds, dtype):
    return np.stack([start(n, s, dtype) for s in seeds])


# The shape edges: the smallest sizes at which the kernels can go wrong.  N = 2, 3, 4: the dropped padding pairs of the 4-unroll;
# 63, 64: the full wave; 65, 66: the first block shape, with waves that have no particle; 255, 256, 257: the first second
# particle of a thread; 1024: the LDS maximum.
EDGE_NS = [2, 3, 4, 63, 64, 65, 66, 255, 256, 257, 1024]
EDGE_STEPS = 6


def edge_batch(n):
    """Instances of an edge case: the longdouble replay is quadratic in N."""
    return 3 if n < 513 else 1


def edge_start(n, seed, dtype):
    """The jittered cubic lattice; up to four particles tighter (spacing 1.05, jitter 0.02), as in tests/quench_checks.py: at the
    default spacing they sit at the pair minimum, where every trial is a tie."""
    xyz = tw.lattice(n, seed, spacing=1.05, jitter=0.02) if n <= 4 else tw.lattice(n, seed)
    return np.asarray(np.concatenate(xyz), dtype=dtype)


def edge_starts(n, dtype):
    return np.stack([edge_start(n, s, dtype) for s in range(edge_batch(n))])


def count_undecided(p0, step_length, dtype, window):
    """The twin from p0 for `window` steps: (trials, undecided, rejected, halvings of the first step).  A trial is undecided
    when |E_trial - E_old| <= (N + 32) u (S_old + S_trial) in longdouble (quench_twin.decision_margin)."""
    q = AdGD(p0, step_length, dtype)
    trials = undecided = rejected = 0
    first = None
    old = qt.exact_energy(q.x)
    for _ in range(window):
        if q.is_stuck:
            break
        x_old, g_old = q.x.copy(), q.g.copy()
        q.step()
        if first is None:
            first = q.last_halvings
        for h, _f in q.trials:
            x_t = fma(-(q.current_step_size * q.t(2.0 ** -h)), g_old, x_old, dtype)
            diff, bound = qt.decision_margin(x_old, x_t, dtype, old)
            trials += 1
            undecided += int(abs(diff) <= bound)
        rejected += len(q.trials) - (0 if q.is_stuck else 1)
        if not q.is_stuck:
            old = qt.exact_energy(q.x)
    return trials, undecided, rejected, first
