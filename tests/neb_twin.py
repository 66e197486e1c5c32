"""CPU twin of one iteration of the batched nudged elastic band (csrc/dzo_neb.hip; the iteration is specified in include/dzo.h,
"Batched nudged elastic band", items 1 .. 6), in numpy, operation by operation.  A helper module for tests/test_neb_twin.py
(which checks it against things it does not depend on) and tests/test_gpu_neb.py (which checks the device against it).  Not a
conftest, no fixtures.

``iterate`` runs in any element type numpy has: float32 and float64 are the device's, and ``numpy.longdouble`` is the wider
format that float64 results are measured against.  Sums the header asks for "in fp64" are taken in ``mt.wide(dtype)``: for the
device's two types that is float64 in the order of the sums (``lowmode_twin.psum``, dots by ``lowmode_twin.dot``); for
longdouble plain longdouble sums.  Energies and gradients are ``energy_gradient`` below: the pair terms of
``modefollow_twin.energy_gradient`` with the device's fused multiply-adds, added in the device's order.  ``run`` iterates as the handle does."""
import functools

import numpy as np

import hybridef_twin as hy
import lowmode_twin as lt
import modefollow_twin as mt

ACTIVE, CONVERGED, FAILED = 0, 1, 2
LONG = np.dtype(np.longdouble)
# the largest force_tol of 1e-5, 3e-5, 1e-4, ... at which the float32 twin converges on the three LJ7 bands of five images
# (tests/test_neb_twin.py finds it and asserts this value; tests/test_gpu_neb.py holds the device to it)
FP32_FORCE_TOL = 1e-5


def _dot(a, b, dt):
    """a.b over the particles in wide(dt): a, b are images [x | y | z] of dt."""
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


def energy_gradient(p, dtype):
    """E and g of the point in ``dtype`` arithmetic: the pair terms of ``modefollow_twin.energy_gradient``, in float32 and
    float64 with the fused multiply-add of the device's radial functions (csrc/dzo_pairwise.h), and the row sums of the device,
    added in ``dtype`` from +0 with j ascending (cl_wave_eval, cl_block_eval), the rows of the energy added in wide(dtype) in
    the order of the sums.  Here the energies steer the tangent through their differences, so the twin in T has
    to carry the rounding of a sequential sum in T, not that of numpy's pairwise sum in a wider type, for the difference
    between two formats to say what the device's rounding can be."""
    dt = np.dtype(dtype)
    wd = mt.wide(dt)
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
        if dt == LONG:
            e = dt.type(4) * (inv_r6 * inv_r6 - inv_r6)
            f = dt.type(-12) * (inv_r8 * (inv_r6 + inv_r6) - inv_r8)
        else:                                                # the device's radial functions fuse the last multiply-add
            fused = lt.fma64 if dt == np.float64 else lt.fma32
            e = dt.type(4) * fused(inv_r6, inv_r6, -inv_r6).astype(dt)
            f = dt.type(-12) * fused(inv_r8, inv_r6 + inv_r6, -inv_r8).astype(dt)
        np.fill_diagonal(e, dt.type(0))
        np.fill_diagonal(f, dt.type(0))
        rows = np.cumsum(e, axis=1, dtype=dt)[:, -1]
        total = rows.astype(wd).sum() if wd == LONG else lt.psum(rows.astype(np.float64))
        E = dt.type(wd.type(0.5) * total)
        g = np.concatenate([np.cumsum(f * c, axis=1, dtype=dt)[:, -1] for c in d])
        return E, (g + g).astype(dt)


def interpolate(a, b, n_images, dtype):
    """The straight band (M, 3N) between the points a and b: copies at the ends, fma(T(m / (M-1)), b - a, a) in between."""
    dt = np.dtype(dtype)
    a, b = np.asarray(a, dtype=dt), np.asarray(b, dtype=dt)
    band = np.empty((n_images, len(a)), dtype=dt)
    band[0], band[-1] = a, b
    for m in range(1, n_images - 1):
        band[m] = _fma(dt.type(np.float64(m) / np.float64(n_images - 1)), b - a, a, dt)
    return band


def tangent(x_prev, x, x_next, e_prev, e, e_next, dtype):
    """Item 2: (tau, d+, d-, branch, margins) of one interior image; branch 0: d+, 1: d-, 2: a d+ + b d-, 3: b d+ + a d-;
    margins: the pairs of energies the branch was chosen from, as (name, value, threshold)."""
    dt = np.dtype(dtype)
    wd = mt.wide(dt)
    dp, dm = x_next - x, x - x_prev
    margins = [("E+ against E", float(e_next), float(e)), ("E against E-", float(e), float(e_prev))]
    with np.errstate(all="ignore"):
        if e_next > e and e > e_prev:
            branch, t = 0, dp
        elif e_next < e and e < e_prev:
            branch, t = 1, dm
        else:
            ar, al = np.abs(e_next - e), np.abs(e_prev - e)
            hi, lo = (ar, al) if ar > al else (al, ar)
            margins.append(("E+ against E-", float(e_next), float(e_prev)))
            if e_next > e_prev:
                branch, t = 2, _fma(hi, dp, lo * dm, dt)
            else:
                branch, t = 3, _fma(lo, dp, hi * dm, dt)
        tn = np.sqrt(_dot(t, t, dt))
        tau = (t.astype(wd) / tn).astype(dt)
    return tau, dp, dm, branch, margins


def iterate(band, velocities, spring=1.0, dt=0.02, max_move=0.1, force_tol=0.0, climb=True, end_energies=None, dtype=np.float64):
    """One iteration of one band ``(M, 3N)`` from the velocities given; ``climb``: a climbing image exists.  Returns a dict:
    band, velocities (after the move), E (M,), g, F and tau (M, 3N; of the band before the move), frms (M,), residual, status,
    climbing, highest, and ``branches``: the values the decisions were taken from, as (name, value, threshold), and ``hit``:
    the set of branch names taken ("tangent0" .. "tangent3", "climbing", "plain", "p>0", "p<=0", "capped", "uncapped")."""
    et = np.dtype(dtype)
    t, wd = et.type, mt.wide(et)
    x = np.asarray(band, dtype=et).copy()
    v = np.asarray(velocities, dtype=et).copy()
    M, n = x.shape
    E, g = np.zeros(M, dtype=et), np.zeros((M, n), dtype=et)
    for m in range(M):                                                                # 1
        if 0 < m < M - 1 or end_energies is None:
            E[m], g[m] = energy_gradient(x[m], et)
        else:
            E[m] = end_energies[0 if m == 0 else 1]
    highest = 1
    branches, hit = [], set()
    for m in range(2, M - 1):
        branches.append(("highest", float(E[m]), float(E[highest])))
        if E[m] > E[highest]:
            highest = m
    climbing = highest if climb else -1
    F, tau, frms = np.zeros((M, n), dtype=et), np.zeros((M, n), dtype=et), np.zeros(M)
    ff = np.zeros(M, dtype=wd)
    with np.errstate(all="ignore"):
        for m in range(1, M - 1):
            tau[m], dp, dm, branch, margins = tangent(x[m - 1], x[m], x[m + 1], E[m - 1], E[m], E[m + 1], et)    # 2
            branches += margins
            hit.add("tangent%d" % branch)
            c = _dot(g[m], tau[m], et)                                                # 3
            gw, tw_ = g[m].astype(wd), tau[m].astype(wd)
            if m == climbing:
                F[m] = (-gw + (c + c) * tw_).astype(et)
                hit.add("climbing")
            else:
                w = wd.type(spring) * (np.sqrt(_dot(dp, dp, et)) - np.sqrt(_dot(dm, dm, et)))
                F[m] = (-(gw - c * tw_) + w * tw_).astype(et)
                hit.add("plain")
            ff[m] = _dot(F[m], F[m], et)
            frms[m] = float(np.sqrt(ff[m] / wd.type(n)))                              # 4
        residual = float(frms.max())
        out = dict(band=x, velocities=v, E=E, g=g, F=F, tau=tau, frms=frms, residual=residual, climbing=climbing, highest=highest,
                   branches=branches, hit=hit)
        if not (np.isfinite(E).all() and np.isfinite(ff).all()):
            out["status"] = FAILED
            return out
        branches.append(("residual", residual, float(force_tol)))
        if residual <= force_tol:
            out["status"] = CONVERGED
            return out
        x, v = x.copy(), v.copy()
        dtT = t(dt)
        for m in range(1, M - 1):                                                     # 5
            p = _dot(v[m], F[m], et)
            if v[m].any():                                                            # as a cosine; v = 0 gives p = 0 in any format
                branches.append(("p", float(p / np.sqrt(_dot(v[m], v[m], et) * ff[m])), 0.0))
            if p > 0:
                vp = ((p / ff[m]) * F[m].astype(wd)).astype(et)
                hit.add("p>0")
            else:
                vp = np.zeros(n, dtype=et)
                hit.add("p<=0")
            v[m] = _fma(dtT, F[m], vp, et)
            s = dtT * v[m]
            sn = np.sqrt(_dot(s, s, et))
            branches.append(("move", float(sn), float(max_move)))
            if sn > max_move:
                s = ((wd.type(max_move) / sn) * s.astype(wd)).astype(et)
                hit.add("capped")
            else:
                hit.add("uncapped")
            x[m] = x[m] + s
    out.update(band=x, velocities=v, status=ACTIVE)
    return out


def run(band, spring=1.0, dt=0.02, max_move=0.1, force_tol=1e-6, climb=True, climb_after=50, max_iterations=2000, dtype=np.float64):
    """The handle's iteration on one band (float32 or float64) from zero velocities.  Returns the last iteration's dict with
    ``iterations`` (moves made) added; ``climbing`` is -1 while no image climbs."""
    et = np.dtype(dtype)
    x = np.asarray(band, dtype=et)
    v = np.zeros_like(x)
    ends = [energy_gradient(x[0], et)[0], energy_gradient(x[-1], et)[0]]
    r = None
    for k in range(max_iterations + 1):
        r = iterate(x, v, spring, dt, max_move, force_tol, bool(climb) and k >= climb_after, ends, et)
        r["iterations"] = k
        if r["status"] != ACTIVE or k == max_iterations:
            break
        x, v = r["band"], r["velocities"]
    return r


@functools.lru_cache(maxsize=None)
def end_pairs(n, seeds, start_mode=0, displacement=0.05):
    """Pairs of minima of the n-particle cluster that a saddle joins, in one frame, in fp64, all on the CPU: per seed a minimum
    (``modefollow_twin.run`` from ``random_start``), a saddle (``hybridef_twin.run`` from that minimum kicked along a mode), and
    the two minima the saddle displaced by +-``displacement`` along its mode slides into (``modefollow_twin.run`` again).
    Returns (a, b, saddles, minima): four (len(seeds), 3n) arrays, minima the first minimum of every seed; a seed whose search
    does not end on a saddle with two different ends raises."""
    a, b, saddles, minima = [], [], [], []
    for seed in seeds:
        r = mt.run(mt.random_start(n, seed), max_steps=400)
        assert r["status"] == mt.CONVERGED and r["index"] == 0, seed
        x, v = mt.kicked(r["point"], start_mode, 0.05)
        s = hy.run(x, v, max_steps=300)
        assert s["status"] == hy.CONVERGED and float(s["lam"]) < -1e-4, seed
        u = np.asarray(s["u"], dtype=np.float64)
        ends = []
        for sign in (1.0, -1.0):
            e = mt.run(s["point"] + sign * displacement * u, max_steps=400)
            assert e["status"] == mt.CONVERGED and e["index"] == 0, seed
            ends.append(e["point"])
        assert np.abs(ends[0] - ends[1]).max() > 1e-3, seed
        a.append(ends[0]); b.append(ends[1]); saddles.append(s["point"]); minima.append(r["point"])
    out = np.stack(a), np.stack(b), np.stack(saddles), np.stack(minima)
    for arr in out:
        arr.setflags(write=False)
    return out
