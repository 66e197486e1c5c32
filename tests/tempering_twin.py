"""CPU twin of the parallel-tempering Monte Carlo of scripts/MonteCarlo.jl as the device runs it (include/dzo.h states the
random-number rule), written from the formulas.  A helper module for tests/test_tempering_twin.py (which checks it
against things it does not depend on) and tests/test_gpu_tempering.py.  Not a conftest, no fixtures.  The radial
function and the longdouble sums come from tests/pairwise_twin.py.

Two ways to run a replica:

* ``replay``: from the start coordinates with the device's recorded draws AND the device's recorded decisions.  Given the
  decisions the coordinates are reproducible bit for bit (the proposal is a product and a sum in T, the sphere test
  three squares and two sums in T: single-rounded operations numpy performs identically).  For every step the twin
  computes the exact delta (longdouble), the project's derived bound b = (N + 32) u (S_old + S_new) -- the bound
  tests/test_gpu_pairwise.py uses for energy_delta -- and classifies the step: the device MUST have accepted, MUST have
  rejected, or the twin cannot tell (``UNDECIDED``: the uniform lies within the error bars of the threshold).
* ``simulate``: on the twin's own decisions (exact delta, longdouble exp), for the CPU tests.
"""
import math

import numpy as np

import pairwise_twin as pw

LD = np.longdouble
U = {np.dtype(np.float64): LD(2.0) ** -53, np.dtype(np.float32): LD(2.0) ** -24}

MUST_REJECT, MUST_ACCEPT, UNDECIDED = 0, 1, -1
CODE_REJECTED, CODE_ACCEPTED, CODE_OUTSIDE = 0, 1, 2

_M64 = (1 << 64) - 1
_MUL, _INC = 0x5851F42D4C957F2D, 0x14057B7EF767814F


# ------------------------------------------------------------------------------ PCG32 XSH-RR, the stated rule
def pcg_state(seed):
    """the state of a stream right after it has been seeded"""
    return (_MUL * ((_INC + seed) & _M64) + _INC) & _M64


def pcg_raw(state, n):
    """(n draws as uint32, the state afterwards)"""
    out = np.empty(n, dtype=np.uint32)
    for i in range(n):
        v = (((state >> 18) ^ state) >> 27) & 0xFFFFFFFF
        r = state >> 59
        out[i] = ((v >> r) | (v << ((32 - r) & 31))) & 0xFFFFFFFF
        state = (_MUL * state + _INC) & _M64
    return out, state


def box_muller_f64(da, db):
    """numpy's fp64 sqrt(-2 log u1) (cos, sin)(2 pi u2) of the integers da, db: u = (d + 1/2) 2^-32 (exact)."""
    u1 = (np.asarray(da, dtype=np.float64) + 0.5) * 2.0 ** -32
    u2 = (np.asarray(db, dtype=np.float64) + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2), r


def step_draws(raw, n_particles, dtype):
    """raw: (steps, 6) uint32 -> (j, normals (steps, 3) of dtype from numpy's fp64 Box-Muller, u of dtype, r (steps, 2))."""
    raw = np.asarray(raw, dtype=np.uint64).reshape(-1, 6)
    j = ((raw[:, 0] * np.uint64(n_particles)) >> np.uint64(32)).astype(np.int64)
    nx, ny, r1 = box_muller_f64(raw[:, 1], raw[:, 2])
    nz, _, r2 = box_muller_f64(raw[:, 3], raw[:, 4])
    u = (raw[:, 5].astype(np.float64) * 2.0 ** -32).astype(dtype)
    return j, np.stack([nx, ny, nz], axis=1).astype(dtype), u, np.stack([r1, r1, r2], axis=1)


def swap_uniform(raw_one, dtype):
    return np.dtype(dtype).type(float(raw_one) * 2.0 ** -32)


# ------------------------------------------------------------------------------ pieces of one step
def propose(old, radius, normal, dtype):
    """x_old + radius * normal: a product and a sum, each rounded to dtype"""
    t = np.dtype(dtype).type
    return t(old) + t(radius) * t(normal)


def inside_sphere(xn, yn, zn, constraining_radius, dtype):
    t = np.dtype(dtype).type
    xn, yn, zn, R = t(xn), t(yn), t(zn), t(constraining_radius)
    return bool(xn * xn + yn * yn + zn * zn < R * R)


def exp_margin(arg, dtype):
    """relative error of exp(arg) computed in dtype from an argument that is itself one rounded product: the argument's
    rounding (|arg| u) plus exp's own (1 ulp <= 2 u), with 2 u to spare"""
    return (abs(LD(arg)) + LD(4)) * U[np.dtype(dtype)]


def classify(delta, b, u, beta, dtype):
    """what a device whose delta is within b of `delta` must have decided for the uniform u"""
    delta, b, u, beta = LD(delta), LD(b), LD(u), LD(beta)
    if not np.isfinite(delta) or not np.isfinite(b):
        return UNDECIDED
    if delta <= -b:
        return MUST_ACCEPT
    with np.errstate(all="ignore"):
        lo_arg, hi_arg = -beta * (delta + b), -beta * (delta - b)      # beta >= 0: lo_arg <= the device's argument <= hi_arg
        lo = np.exp(lo_arg) * (LD(1) - exp_margin(lo_arg, dtype))
        hi = np.exp(hi_arg) * (LD(1) + exp_margin(hi_arg, dtype))
    if u < lo:
        return MUST_ACCEPT
    if delta > b and u > hi:
        return MUST_REJECT
    return UNDECIDED


def fac(dtype):
    """ten successive square roots of two in dtype (:21-24)"""
    f = np.dtype(dtype).type(2)
    for _ in range(10):
        f = np.sqrt(f)
    return f


def adapt_radius(radius, num_accept, num_reject, dtype):
    """:77-81"""
    t = np.dtype(dtype).type
    radius = t(radius)
    if 3 * num_accept < num_reject:
        return radius / fac(dtype)
    if 3 * num_accept > num_reject:
        return min(t(1), radius * fac(dtype))
    return radius


def delta_bound(n, S, dtype):
    return LD(n + 32) * U[np.dtype(dtype)] * LD(S)


# ------------------------------------------------------------------------------ replay / simulate
class Trajectory:
    pass


def _run(xyz0, j, normals, u, radius, beta, constraining_radius, dtype, codes):
    """codes: the device's (replay) or None (simulate)."""
    t = np.dtype(dtype).type
    xyz = np.array(xyz0, dtype=dtype).reshape(3, -1).copy()
    n = xyz.shape[1]
    steps = len(j)
    tr = Trajectory()
    tr.delta = np.zeros(steps, dtype=LD); tr.bound = np.zeros(steps, dtype=LD)
    tr.klass = np.full(steps, UNDECIDED, dtype=np.int64)
    tr.inside = np.zeros(steps, dtype=bool)
    tr.code = np.zeros(steps, dtype=np.int8)
    tr.energy = np.zeros(steps, dtype=LD)            # the exact energy of the configuration after each step
    tr.energy_bound = np.zeros(steps, dtype=LD)      # what a trace accumulated in dtype may differ from it by
    e0, s0 = pw.energy(xyz[0], xyz[1], xyz[2])
    tr.initial_energy, tr.initial_bound = e0, delta_bound(n, s0, dtype)
    e, eb = e0, tr.initial_bound
    for i in range(steps):
        p = int(j[i])
        new = [propose(xyz[c, p], radius, normals[i, c], dtype) for c in range(3)]
        tr.inside[i] = inside_sphere(new[0], new[1], new[2], constraining_radius, dtype)
        code = CODE_OUTSIDE
        if tr.inside[i]:
            d, S = pw.energy_delta(xyz[0], xyz[1], xyz[2], p, *new)
            b = delta_bound(n, S, dtype)
            tr.delta[i], tr.bound[i] = d, b
            tr.klass[i] = classify(d, b, u[i], beta, dtype)
            if codes is not None:
                code = int(codes[i])
            else:
                with np.errstate(all="ignore"):
                    code = CODE_ACCEPTED if (d <= 0 or LD(u[i]) <= np.exp(-LD(beta) * d)) else CODE_REJECTED
            if code == CODE_ACCEPTED:
                xyz[:, p] = new
                e = e + d
                eb = eb + b + U[np.dtype(dtype)] * (abs(e) + eb)      # the addition energy += delta, rounded once
        elif codes is not None:
            code = int(codes[i])                     # kept as recorded; the test compares it with tr.inside
        tr.code[i] = code
        tr.energy[i], tr.energy_bound[i] = e, eb
    tr.final = xyz
    tr.num_accept = int(np.sum(tr.code == CODE_ACCEPTED))
    tr.num_reject = steps - tr.num_accept
    tr.radius = adapt_radius(t(radius), tr.num_accept, tr.num_reject, dtype)
    return tr


def replay(xyz0, j, normals, u, codes, radius, beta, constraining_radius, dtype):
    return _run(xyz0, j, normals, u, radius, beta, constraining_radius, dtype, codes)


def simulate(xyz0, j, normals, u, radius, beta, constraining_radius, dtype):
    return _run(xyz0, j, normals, u, radius, beta, constraining_radius, dtype, None)


def undecided_share(tr):
    return float(np.sum(tr.inside & (tr.klass == UNDECIDED))) / max(1, len(tr.klass))


# ------------------------------------------------------------------------------ swap (:114-131)
def swap_classify(xyz_a, xyz_b, beta_a, beta_b, u, dtype):
    """(class, exact log_prob, its bound) for the pair: the device's energies are within (N + 32) u S of the exact ones, the
    two subtractions and the product add three roundings"""
    n = np.asarray(xyz_a).reshape(3, -1).shape[1]
    a = np.asarray(xyz_a, dtype=dtype).reshape(3, -1); b = np.asarray(xyz_b, dtype=dtype).reshape(3, -1)
    ea, sa = pw.energy(a[0], a[1], a[2]); eb, sb = pw.energy(b[0], b[1], b[2])
    t = np.dtype(dtype).type
    db = LD(t(beta_a)) - LD(t(beta_b))
    lp = (ea - eb) * db
    ut = U[np.dtype(dtype)]
    err = (delta_bound(n, sa, dtype) + delta_bound(n, sb, dtype) + ut * (abs(ea) + abs(eb))) * abs(db) + 3 * ut * abs(lp)
    if lp >= err:
        return MUST_ACCEPT, lp, err
    with np.errstate(all="ignore"):
        lo = np.exp(lp - err) * (LD(1) - exp_margin(lp - err, dtype))
        hi = np.exp(lp + err) * (LD(1) + exp_margin(lp + err, dtype))
    if LD(u) < lo:
        return MUST_ACCEPT, lp, err
    if lp < -err and LD(u) > hi:
        return MUST_REJECT, lp, err
    return UNDECIDED, lp, err


# ------------------------------------------------------------------------------ analyze (:154-177)
def moments(energies):
    """(V1, V2, V3, mean|E|, mean|E^2|, mean|E^3|) of one replica's trace in longdouble"""
    e = np.asarray(energies, dtype=LD)
    e2 = e * e
    e3 = e2 * e
    n = LD(len(e))
    return e.sum() / n, e2.sum() / n, e3.sum() / n, np.abs(e).sum() / n, np.abs(e2).sum() / n, np.abs(e3).sum() / n


def heat_capacity(V1, V2, V3, inv_tau, dtype):
    """cv, cv_prime of :169-176 with every operation in dtype"""
    t = np.dtype(dtype).type
    V1, V2, V3, inv_tau = t(V1), t(V2), t(V3), t(inv_tau)
    inv_tau_2 = inv_tau * inv_tau
    inv_tau_4 = inv_tau_2 * inv_tau_2
    var = V2 - V1 * V1
    cov = V3 - V2 * V1
    two_var = var + var
    return inv_tau_2 * var, inv_tau_4 * (cov - (V1 + t(1) / inv_tau) * two_var)


# ------------------------------------------------------------------------------ inputs of the trajectory tests
TRAJECTORY_NS = [2, 13, 38, 64, 65, 200, 256, 257, 1024]      # from 257 on the block kernel's strided loops make a second trip
TRAJECTORY_REPLICAS = 3
TRAJECTORY_STEPS = 200
TRAJECTORY_SEED = 4242
UNDECIDED_CAP = {np.dtype(np.float32): 0.05, np.dtype(np.float64): 0.0}


def trajectory_inputs(n, dtype):
    """(replicas (R, 3, n) of dtype, inverse temperatures, radii, constraining radius): the configuration the pairwise GPU
    tests use for n particles, centred, with a little seeded jitter per replica; temperatures 0.35, 0.15, 0.05 (the
    script's range); a sphere that holds the cluster with room to spare."""
    base = np.stack(pw.cluster(n, seed=n))
    base = base - base.mean(axis=1, keepdims=True)
    reps = np.stack([np.stack(pw.jittered(tuple(base), 100 * n + k, 0.02)) for k in range(TRAJECTORY_REPLICAS)]).astype(dtype)
    beta = 1.0 / np.array([0.35, 0.15, 0.05])
    radii = np.array([0.06, 0.04, 0.02])
    R = float(np.sqrt((base ** 2).sum(axis=0)).max() + 0.6)
    return reps, beta, radii, R


def own_draws(seed, steps, n, dtype):
    raw, _ = pcg_raw(pcg_state(seed), 6 * steps)
    return step_draws(raw.reshape(steps, 6), n, dtype)


LJ38_TEMPERATURES = (0.05, 0.35)
