"""CPU twin of the hybrid eigenvector-following step (csrc/dzo_hybridef.hip; the step is specified in include/dzo.h, "Batched
hybrid eigenvector following", items 1 .. 5), in numpy, operation by operation.  A helper module for
tests/test_hybridef_twin.py (which checks it against things it does not depend on) and tests/test_gpu_hybridef.py (which checks
the device against it).  Not a conftest, no fixtures.

``step`` runs in any element type numpy has: float32 and float64 are the device's, and ``numpy.longdouble`` is the wider format
that float64 results are measured against.  Sums the header asks for "in fp64" are taken in ``mt.wide(dtype)``: for the device's
two types that is float64 in the order of the sums (``lowmode_twin.psum``, dots by ``lowmode_twin.dot``); for longdouble plain
longdouble sums.  Energies and gradients are ``modefollow_twin.energy_gradient`` (numpy's summation order, not the device's:
the GPU tests allow for that with a measured bound).  ``run`` iterates the step with the mode refined by
``lowmode_twin.lowest_mode`` from the previous step's vector, as the handle does."""
import numpy as np

import lowmode_twin as lt
import modefollow_twin as mt

ACTIVE, CONVERGED, FAILED = 0, 1, 2
# searches of ``run`` (defaults, 200 steps at most) that end on an index-1 saddle from the 16 asymmetric LJ13 minima of
# tests/test_hybridef_twin.py, by the non-zero mode kicked along: measured there, and the device's yardstick in
# tests/test_gpu_hybridef.py (this count - 2)
TWIN_FOUND = {0: 16, 1: 14}
LONG = np.dtype(np.longdouble)


def _dot(a, b, dt):
    """a.b over the particles in wide(dt): a, b are points [x | y | z] of dt."""
    wd = mt.wide(dt)
    if wd == LONG:
        return (a.astype(wd) * b.astype(wd)).sum()
    return np.float64(lt.dot(a.reshape(3, -1), b.reshape(3, -1)))


def _fma(a, b, c, dt):
    """fma(a, b_e, c_e) in dt (longdouble: a product and a sum, the format is wider than either device type anyway)."""
    if dt == LONG:
        return a * b + c
    a = np.full(b.shape, a, dtype=dt)
    return (lt.fma64(a, b, c) if dt == np.float64 else lt.fma32(a, b, c)).astype(dt)


def uphill(F, lam, zero_tol, max_step, dtype):
    """Item 3: (h, a, h before the cap) from F = T(u.g) and lam, every operation in ``dtype``; the cap compares in wide."""
    dt = np.dtype(dtype)
    t, wd = dt.type, mt.wide(dt)
    F, lam, one = t(F), t(lam), t(1)
    with np.errstate(all="ignore"):
        a = np.abs(lam)
        q = (F + F) / a
        raw = t(0) if a <= t(zero_tol) else t(q / (one + np.sqrt(one + q * q)))
        h = raw
        if wd.type(np.abs(raw)) > wd.type(max_step):
            h = -t(max_step) if raw < 0 else t(max_step)
    return h, a, raw


def step(point, u, lam, max_step=0.1, tangent_steps=10, tangent_steps_convex=2, tangent_cap=0.05, tangent_first=0.01, zero_tol=1e-4,
         grad_tol=0.0, dtype=np.float64, mode_failed=False):
    """One step from the mode (u, lam) given.  Returns a dict: point, E, g, grms, status, F, h, tangent (iterations that moved
    the point), evaluations, and ``branches``: the values the step's decisions were taken from, as (name, value, threshold);
    s.y is given as the cosine of the angle between s and y."""
    dt = np.dtype(dtype)
    t, wd = dt.type, mt.wide(dt)
    x = np.asarray(point, dtype=dt).copy()
    u = np.asarray(u, dtype=dt)
    lam = t(lam)
    n = len(x)
    zt = t(zero_tol)
    E, g = mt.energy_gradient(x, dt)                                                  # 1
    with np.errstate(all="ignore"):
        gg = _dot(g, g, dt)
        grms = float(np.sqrt(gg / wd.type(n)))
    out = dict(point=x.copy(), E=E, g=g, grms=grms, F=t(0), h=t(0), tangent=0, evaluations=1, branches=[])
    if not (np.isfinite(E) and np.isfinite(gg) and np.isfinite(lam)) or mode_failed:   # 2
        out["status"] = FAILED
        return out
    if grms <= grad_tol:
        out["status"] = CONVERGED
        return out
    branches = [("grms", grms, grad_tol)]
    with np.errstate(all="ignore"):
        F = t(_dot(u, g, dt))                                                         # 3
        h, a, raw = uphill(F, lam, zero_tol, max_step, dt)
        branches += [("a", float(a), float(zt)), ("h", float(abs(raw)), float(max_step))]
        x = _fma(h, u, x, dt)
        tmax = tangent_steps if lam < -zt else tangent_steps_convex                   # 4
        made, evaluations = 0, 1
        xp = pp_ = None
        for k in range(tmax):
            _, gk = mt.energy_gradient(x, dt)
            evaluations += 1
            c = _dot(u, gk, dt)
            p = (gk.astype(wd) - c * u.astype(wd)).astype(dt)
            p2 = _dot(p, p, dt)
            prms = np.sqrt(p2 / wd.type(n))
            branches.append(("prms", float(prms), grad_tol))
            if prms <= grad_tol:
                break
            alpha = wd.type(tangent_first)
            if k > 0:
                s, y = x - xp, p - pp_
                ss, sy = _dot(s, s, dt), _dot(s, y, dt)
                branches.append(("sy", float(sy / np.sqrt(ss * _dot(y, y, dt))), 0.0))   # as a cosine: how far from 0
                if sy > 0:
                    alpha = ss / sy
            dn = alpha * np.sqrt(p2)
            branches.append(("dn", float(dn), float(tangent_cap)))
            if dn > tangent_cap:
                alpha = alpha * (wd.type(tangent_cap) / dn)
            xp, pp_ = x, p
            x = _fma(-t(alpha), p, x, dt)
            made = k + 1
    out.update(point=x, F=F, h=h, tangent=made, evaluations=evaluations, status=ACTIVE, branches=branches)
    return out


def run(point, u, max_step=0.1, tangent_steps=10, tangent_steps_convex=2, tangent_cap=0.05, tangent_first=0.01, krylov=8, mode_cycles=1,
        mode_tol=1e-3, zero_tol=1e-4, grad_tol=1e-10, max_steps=200, dtype=np.float64):
    """The handle's iteration on one instance (float32 or float64): per step ``lowmode_twin.lowest_mode`` from the previous
    step's vector with ``mode_cycles + 1`` cycles at most (``mode_cycles`` refine, the first product of one more measures),
    then ``step``.  Returns the last step's dict with ``steps`` (moves made), ``lam``, ``u``, ``products`` and cumulative
    ``evaluations`` added."""
    dt = np.dtype(dtype)
    x, u = np.asarray(point, dtype=dt), np.asarray(u, dtype=dt)
    products = evaluations = 0
    r = None
    for k in range(max_steps + 1):
        m = lt.lowest_mode(x, dt, True, krylov, mode_cycles + 1, mode_tol, start=u)
        products += m.products
        r = step(x, m.vector, m.eigenvalue, max_step, tangent_steps, tangent_steps_convex, tangent_cap, tangent_first, zero_tol, grad_tol, dt,
                 mode_failed=m.status == lt.FAILED)
        evaluations += r["evaluations"]
        r.update(steps=k, lam=m.eigenvalue, u=m.vector, products=products, evaluations=evaluations)
        if r["status"] != ACTIVE or k == max_steps:
            break
        x, u = r["point"], m.vector
    return r
