"""The saddle searches of dzo.find_saddles and dzo.find_saddles_hybrid with the Morse functions of tests/morse_twin.py, in fp64
numpy.  The method twins of tests/modefollow_twin.py and tests/hybridef_twin.py evaluate Lennard-Jones through module-level
functions, so the part the Morse GPU tests need is restated here: the eigenvector-following iteration of include/dzo.h with
modes from numpy.linalg.eigh of the twin Hessian (``follow``; the per-mode step is modefollow_twin.mode_steps itself), and the
hybrid iteration with the EXACT lowest mode of the rigid-body-projected Hessian where the device refines it by Lanczos
(``hybrid``).  They serve one purpose: to choose kick, seed and N for tests/test_gpu_morse.py so that the method itself, free
of the device's rounding, ends on saddles from well over half of the starts.  A helper module; no fixtures."""
import numpy as np

import modefollow_twin as mf
import morse_twin as mt

ACTIVE, CONVERGED, FAILED = 0, 1, 2


def energy_gradient(p, rho):
    return mt.energy_f64(p, rho), mt.gradient_f64(p, rho)


def hessian(p, rho):
    n = len(p) // 3
    h = mt.hessian(p[:n], p[n:2 * n], p[2 * n:], rho).astype(np.float64)
    return 0.5 * (h + h.T)


def modes(p, rho):
    return np.linalg.eigh(hessian(np.asarray(p, dtype=np.float64), rho))


def minimum(start, rho):
    """The fp64 minimum below ``start`` (morse_twin.minimize_f64, then Newton steps off the zero modes)."""
    p = mt.minimize_f64(start, rho)
    for _ in range(3):
        lam, vec = modes(p, rho)
        keep = np.abs(lam) > 1e-6 * np.abs(lam).max()
        p = p - vec[:, keep] @ ((vec[:, keep].T @ mt.gradient_f64(p, rho)) / lam[keep])
    return p


def follow(point, rho, target_index=1, start_mode=0, w=None, max_step=0.1, zero_tol=1e-4, grad_tol=1e-10, max_steps=300):
    """Eigenvector following (include/dzo.h, steps 1-9) from ``point``; ``w``: the followed vector to start with.  Returns
    (status, point, index, steps)."""
    x = np.asarray(point, dtype=np.float64).copy()
    w_set = w is not None
    for k in range(max_steps + 1):
        _, g = energy_gradient(x, rho)
        lam, V = modes(x, rho)
        zero = np.abs(lam) <= zero_tol
        index = int((lam < -zero_tol).sum())
        if not np.all(np.isfinite(g)):
            return FAILED, x, index, k
        if np.sqrt((g * g).sum() / len(g)) <= grad_tol:
            return CONVERGED, x, index, k
        if k == max_steps:
            break
        F = V.T @ g
        followed = -1
        if target_index == 1:
            nonzero = np.flatnonzero(~zero)
            if not w_set:
                if len(nonzero) <= start_mode:
                    return FAILED, x, index, k
                followed = int(nonzero[start_mode])
            else:
                followed = int(nonzero[np.argmax(np.abs(V.T @ w)[nonzero])])
            w, w_set = V[:, followed].copy(), True
        h = mf.mode_steps(F, lam, zero_tol, followed, np.float64)
        hn = float(np.sqrt((h * h).sum()))
        if hn > max_step:
            h = h * (max_step / hn)
        x = x + V @ h
    return ACTIVE, x, index, max_steps


def kicked(minimum_, rho, start_mode, kick, zero_tol=1e-4):
    lam, V = modes(minimum_, rho)
    nonzero = np.flatnonzero(np.abs(lam) > zero_tol)
    v = V[:, nonzero[start_mode]]
    return np.asarray(minimum_, dtype=np.float64) + kick * v, v.copy()


def _rigid_projector(p):
    """The projector onto the complement of net translations and rotations at the point."""
    n = len(p) // 3
    c = p.reshape(3, n) - p.reshape(3, n).mean(axis=1, keepdims=True)
    basis = []
    for a in range(3):
        t = np.zeros((3, n)); t[a] = 1.0
        basis.append(t.ravel())
        e = np.zeros(3); e[a] = 1.0
        basis.append(np.cross(e, c.T).T.ravel())
    q, _ = np.linalg.qr(np.array(basis).T)
    return np.eye(3 * n) - q @ q.T


def lowest_vibration(p, rho):
    """(eigenvalue, vector) of the lowest mode of P H P in the range of P."""
    P = _rigid_projector(p)
    lam, V = np.linalg.eigh(P @ hessian(p, rho) @ P)
    ok = np.flatnonzero(np.abs(np.einsum("ij,ij->j", V, P @ V)) > 0.5)        # the eigenvectors inside the range of P
    k = ok[np.argmin(lam[ok])]
    return lam[k], V[:, k]


def hybrid(point, rho, u, max_step=0.1, tangent_steps=10, tangent_steps_convex=2, tangent_cap=0.05, tangent_first=0.01, zero_tol=1e-4,
           grad_tol=1e-10, max_steps=300):
    """Hybrid eigenvector following (include/dzo.h) with the exact lowest vibration as the mode: an uphill step
    h = q / (1 + sqrt(1 + q q)), q = 2 F / |lam| along it (capped at max_step), then steepest-descent steps orthogonal to it
    with a Barzilai-Borwein length capped at tangent_cap (the first one tangent_first).  Returns (status, point, lam, steps)."""
    x = np.asarray(point, dtype=np.float64).copy()
    lam = 0.0
    for k in range(max_steps + 1):
        _, g = energy_gradient(x, rho)
        lam, v = lowest_vibration(x, rho)
        if v @ u < 0:
            v = -v
        u = v
        if not np.all(np.isfinite(g)):
            return FAILED, x, lam, k
        if np.sqrt((g * g).sum() / len(g)) <= grad_tol:
            return CONVERGED, x, lam, k
        if k == max_steps:
            break
        F = float(u @ g)
        h = 0.0
        if abs(lam) > zero_tol:
            q = (F + F) / abs(lam)
            h = q / (1.0 + np.sqrt(1.0 + q * q))
            h = max(-max_step, min(max_step, h))
        x = x + h * u
        steps = tangent_steps if lam < -zero_tol else tangent_steps_convex
        g_old = x_old = None
        for t in range(steps):
            _, g = energy_gradient(x, rho)
            gt = g - (g @ u) * u
            if g_old is None:
                alpha = tangent_first
            else:
                s, y = x - x_old, gt - g_old
                alpha = abs(s @ y) and (s @ s) / abs(s @ y)
            step = alpha * gt
            ln = np.sqrt(step @ step)
            if ln > tangent_cap:
                step *= tangent_cap / ln
            x_old, g_old = x.copy(), gt
            x = x - step
    return ACTIVE, x, lam, max_steps
