"""CPU twin of the eigenvector-following step (csrc/dzo_modefollow.hip; the step is specified in include/dzo.h), in numpy,
operation by operation.  A helper module for tests/test_modefollow_twin.py (which checks it against things it does not depend
on) and tests/test_gpu_modefollow.py (which checks the device against it).  Not a conftest, no fixtures.

``step`` runs in any element type numpy has: float32 and float64 are the device's, and ``numpy.longdouble`` is the wider
format that float64 results are measured against (the rounding error of a float64 run is invisible to a float64 reference).
Sums the header asks for "in fp64" are taken in ``wide(dtype)``: float64 for the device's two types, longdouble for longdouble.
Modes are taken as given (``step``) or from ``numpy.linalg.eigh`` of the twin Hessian of tests/hessian_twin.py (``modes``,
``run``).  Summation ORDERS are numpy's, not the device's: the GPU tests allow for that with a measured bound."""
import numpy as np

import hessian_twin as ht
import pairwise_twin as tw

ACTIVE, CONVERGED, FAILED = 0, 1, 2


def wide(dtype):
    return np.dtype(np.longdouble) if np.dtype(dtype) == np.dtype(np.longdouble) else np.dtype(np.float64)


def energy_gradient(p, dtype):
    """E and g of the point in ``dtype`` arithmetic (numpy's summation order)."""
    dt = np.dtype(dtype)
    q = np.asarray(p, dtype=dt)
    n = len(q) // 3
    x, y, z = q[:n], q[n:2 * n], q[2 * n:]
    with np.errstate(all="ignore"):
        d = [c[:, None] - c[None, :] for c in (x, y, z)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        np.fill_diagonal(r2, dt.type(1))
        inv_r2 = dt.type(1) / r2
        inv_r4 = inv_r2 * inv_r2
        inv_r6 = inv_r4 * inv_r2
        inv_r8 = inv_r4 * inv_r4
        e = dt.type(4) * (inv_r6 * inv_r6 - inv_r6)
        f = dt.type(-12) * (inv_r8 * (inv_r6 + inv_r6) - inv_r8)
        np.fill_diagonal(e, dt.type(0))
        np.fill_diagonal(f, dt.type(0))
        E = dt.type(wide(dt).type(0.5) * e.astype(wide(dt)).sum())
        g = np.concatenate([(f * c).sum(axis=1) for c in d])
        return E, (g + g).astype(dt)


def pair_term_magnitude(p):
    """sum over pairs of |4 (r^-12 - r^-6)| in fp64: what the rounding of an energy sum scales with."""
    q = np.asarray(p, dtype=np.float64)
    n = len(q) // 3
    c = q.reshape(3, n)
    d = c[:, :, None] - c[:, None, :]
    r2 = (d * d).sum(axis=0)
    iu = np.triu_indices(n, 1)
    inv_r6 = 1.0 / r2[iu] ** 3
    return float(np.abs(4.0 * (inv_r6 * inv_r6 - inv_r6)).sum())


def mode_steps(F, lam, zero_tol, followed, dtype):
    """Step 7: h[i] = s q / (1 + sqrt(1 + q q)), q = (F + F) / |lam|; zero modes 0; every operation in ``dtype``."""
    dt = np.dtype(dtype)
    F, lam = np.asarray(F, dtype=dt), np.asarray(lam, dtype=dt)
    one = dt.type(1)
    with np.errstate(all="ignore"):
        a = np.abs(lam)
        q = (F + F) / a
        h = q / (one + np.sqrt(one + q * q))
        s = np.full(len(F), -1.0).astype(dt)
        if followed >= 0:
            s[followed] = one
        return np.where(a <= dt.type(zero_tol), dt.type(0), s * h).astype(dt)


def step(point, lam, V, w=None, w_set=False, target_index=0, start_mode=0, max_step=0.2, zero_tol=1e-4, grad_tol=0.0, dtype=np.float64,
         sweeps=0):
    """One step from the modes given: V[:, i] belongs to lam[i], ascending.  Returns a dict: point, E, g, grms, index, zeros,
    status, F, h, followed, step_length, w, w_set, overlaps."""
    dt, wd = np.dtype(dtype), wide(dtype)
    x = np.asarray(point, dtype=dt)
    lam, V = np.asarray(lam, dtype=dt), np.asarray(V, dtype=dt)
    n = len(x)
    zt = dt.type(zero_tol)
    E, g = energy_gradient(x, dt)                                                     # 1
    with np.errstate(all="ignore"):
        gw = g.astype(wd)
        grms = float(np.sqrt((gw * gw).sum() / wd.type(n)))                           # 2
        zero = np.abs(lam) <= zt                                                      # 3
    out = dict(point=x.copy(), E=E, g=g, grms=grms, index=int((lam < -zt).sum()), zeros=int(zero.sum()), F=None, h=None, followed=-1,
               step_length=0.0, w=None if w is None else np.asarray(w, dtype=dt).copy(), w_set=bool(w_set), overlaps=None)
    if not (np.isfinite(E) and np.all(np.isfinite(g)) and np.all(np.isfinite(lam))) or sweeps < 0:   # 4
        out["status"] = FAILED
        return out
    if grms <= grad_tol:
        out["status"] = CONVERGED
        return out
    Vw = V.astype(wd)
    F = (Vw.T @ gw).astype(dt)                                                        # 5
    followed = -1
    if target_index == 1:                                                             # 6
        nonzero = np.flatnonzero(~zero)
        if not w_set:
            if len(nonzero) <= start_mode:
                out["status"] = FAILED
                return out
            followed = int(nonzero[start_mode])
        else:
            ov = np.abs(Vw.T @ np.asarray(w, dtype=dt).astype(wd))
            out["overlaps"] = ov
            if len(nonzero) == 0 or not np.all(np.isfinite(ov)):
                out["status"] = FAILED
                return out
            followed = int(nonzero[np.argmax(ov[nonzero])])                           # argmax: the first of equals
        out["w"], out["w_set"] = V[:, followed].copy(), True
    h = mode_steps(F, lam, zero_tol, followed, dt)                                    # 7
    hw = h.astype(wd)
    hn = float(np.sqrt((hw * hw).sum()))                                              # 8
    capped = hn > max_step
    if capped:
        h = h * dt.type(wd.type(max_step) / wd.type(hn))
    d = np.zeros(n, dtype=dt)                                                         # 9: columns ascending from +0
    for i in range(n):
        d = d + V[:, i] * h[i]
    out.update(point=(x + d).astype(dt), F=F, h=h, followed=followed, step_length=float(max_step) if capped else hn, status=ACTIVE)
    return out


def modes(point):
    """Ascending eigenvalues and eigenvectors (columns) of the fp64 twin Hessian at the point."""
    H = ht.hessian_f64(np.asarray(point, dtype=np.float64))
    return np.linalg.eigh(0.5 * (H + H.T))


def run(point, target_index=0, start_mode=0, max_step=0.2, zero_tol=1e-4, grad_tol=1e-10, max_steps=200, w=None, dtype=np.float64):
    """The handle's iteration on one instance: modes from ``modes`` at every step.  Returns the last step's dict with ``steps``
    (moves made) added."""
    dt = np.dtype(dtype)
    x = np.asarray(point, dtype=dt)
    w_set = w is not None
    r = None
    for k in range(max_steps + 1):
        lam, V = modes(x.astype(np.float64))
        r = step(x, lam.astype(dt), V.astype(dt), w, w_set, target_index, start_mode, max_step, zero_tol, grad_tol, dt)
        r["steps"] = k
        if r["status"] != ACTIVE or k == max_steps:
            break
        x, w, w_set = r["point"], r["w"], r["w_set"]
    return r


def random_start(n, seed, min_distance=0.85):
    """An asymmetric start of n particles as a point [x | y | z]: Gaussian coordinates scaled to the cluster's size, drawn again
    until every pair distance exceeds ``min_distance``."""
    rng = np.random.default_rng(seed)
    scale = 0.55 * n ** (1.0 / 3.0)
    while True:
        c = rng.normal(size=(3, n)) * scale
        d = c[:, :, None] - c[:, None, :]
        r = np.sqrt((d * d).sum(axis=0))
        if r[np.triu_indices(n, 1)].min() > min_distance:
            return c.reshape(-1)


def kicked(minimum, start_mode, kick, zero_tol=1e-4):
    """What ``dzo.find_saddles`` starts from: the minimum displaced by ``kick`` along its ``start_mode``-th non-zero mode, and
    that mode."""
    lam, V = modes(minimum)
    nonzero = np.flatnonzero(np.abs(lam) > zero_tol)
    v = V[:, nonzero[start_mode]]
    return np.asarray(minimum, dtype=np.float64) + kick * v, v.copy()
