"""CPU twin of the structure fingerprint and classifier (csrc/dzo_structure.hip) as include/dzo.h states them.  A helper module
for tests/test_structure_twin.py (which checks it against things it does not depend on) and tests/test_gpu_structure.py (which
holds the device kernels to it).  Not a conftest, no fixtures.

Two levels:

* ``fingerprint``: every operation in the element type and in the order the header names, so that a correct kernel reproduces
  it bit for bit: the pair term with the exact fused multiply-add of lowmode_twin, the rows summed over j ascending, the fp64
  sums over the particles in the tree of ``lowmode_twin.psum`` (the order of the device's wave and block sums).
* ``row_scales`` / ``distance_scales``: the sums of absolute values that scale the rounding bounds, from
  ``pairwise_twin.row_energies`` in longdouble; ``gamma`` is the factor n eps / (1 - n eps).
* ``matches`` / ``classify``: the match rule in fp64 and the greedy leader labels.
"""
import numpy as np

import lowmode_twin as lt
import pairwise_twin as tw

LD = np.longdouble
EPS = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}     # unit roundoff


def gamma(n, dtype):
    ne = n * EPS[np.dtype(dtype)]
    return ne / (1.0 - ne)


# ------------------------------------------------------------------------------ the fingerprint, bit for bit
def particle_energies(p, dtype):
    """e_i = sum_{j != i} e(r2_ij) of the point p = [x | y | z], summed in ``dtype`` from +0 with j ascending."""
    dtype = np.dtype(dtype)
    t = dtype.type
    P = np.asarray(p, dtype=dtype).reshape(3, -1)
    n = P.shape[1]
    with np.errstate(all="ignore"):
        d = P[:, :, None] - P[:, None, :]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        np.fill_diagonal(r2, t(1))                           # the self term is computed and dropped
        inv_r2 = t(1) / r2.ravel()
        inv_r4 = inv_r2 * inv_r2
        inv_r6 = inv_r4 * inv_r2
        e = (t(4) * lt._fma(inv_r6, inv_r6, -inv_r6, dtype).astype(dtype)).reshape(n, n)
        np.fill_diagonal(e, t(0))
        row = np.zeros(n, dtype=dtype)
        for j in range(n):
            row = row + e[:, j]
    return row


def centroid_distances(p, dtype):
    """d_i: the centroid summed in fp64 in the order of the sums, one division, one rounding; the squares added left to right."""
    dtype = np.dtype(dtype)
    P = np.asarray(p, dtype=dtype).reshape(3, -1)
    n = P.shape[1]
    with np.errstate(all="ignore"):
        c = [dtype.type(np.float64(lt.psum(P[k].astype(np.float64))) / np.float64(n)) for k in range(3)]
        dx, dy, dz = P[0] - c[0], P[1] - c[1], P[2] - c[2]
        return dx * dx + dy * dy + dz * dz


def fingerprint(p, dtype, parts=False):
    """(fingerprint (2N,), E) of the point p; with ``parts`` also the unsorted e and d."""
    dtype = np.dtype(dtype)
    e = particle_energies(p, dtype)
    d = centroid_distances(p, dtype)
    with np.errstate(all="ignore"):
        E = dtype.type(0.5 * np.float64(lt.psum(e.astype(np.float64))))
    fp = np.concatenate([np.sort(e), np.sort(d)])            # numpy sorts NaN last
    return (fp, E, e, d) if parts else (fp, E)


def fingerprints(points, n_particles, dtype):
    """Rows = instances of ``points`` (batch, 3N): (fingerprints (batch, 2N), energies (batch,))."""
    pts = np.asarray(points, dtype=dtype).reshape(-1, 3 * n_particles)
    out = [fingerprint(p, dtype) for p in pts]
    return np.stack([f for f, _ in out]), np.array([E for _, E in out], dtype=dtype)


# ------------------------------------------------------------------------------ what scales the rounding bounds
def row_scales(p):
    """(e_i, S_i = sum_j |e_ij|) in longdouble (pairwise_twin.row_energies) of the point p = [x | y | z] (fp64 values)."""
    P = np.asarray(p, dtype=np.float64).reshape(3, -1)
    return tw.row_energies(P[0], P[1], P[2])


def distance_scales(p):
    """(d_i, D_i) in longdouble: D_i = sum_c (|r_ic| + |c_c|)^2, the absolute values of the terms of d_i with the squares of
    r_ic - c_c written out."""
    P = np.asarray(p, dtype=np.float64).reshape(3, -1).astype(LD)
    c = P.sum(axis=1, keepdims=True) / LD(P.shape[1])
    return ((P - c) ** 2).sum(axis=0), ((np.abs(P) + np.abs(c)) ** 2).sum(axis=0)


# ------------------------------------------------------------------------------ the classifier
def relative_distance(a, b):
    """max_i |a_i - b_i| / max(1, |a_i|, |b_i|) in fp64: a and b match iff this is <= tol (up to the rounding of the product)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))))


def matches(a, B, tol):
    """Which rows of B (m, length) the vector a matches: |a_i - b_i| <= tol * max(1, |a_i|, |b_i|) for every i, in fp64."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64).reshape(-1, len(a))
    with np.errstate(all="ignore"):
        scale = np.maximum(1.0, np.maximum(np.abs(a)[None, :], np.abs(B)))
        ok = np.abs(a[None, :] - B) <= np.float64(tol) * scale
    return np.all(ok, axis=1) & np.all(np.isfinite(B), axis=1) & bool(np.all(np.isfinite(a)))


def classify(F, tol):
    """Greedy leader labels in index order of the rows of F: (labels int32, representatives)."""
    F = np.asarray(F)
    F = F.reshape(F.shape[0], -1).astype(np.float64)
    labels = np.full(F.shape[0], -1, dtype=np.int32)
    reps = []
    for k in range(F.shape[0]):
        if not np.all(np.isfinite(F[k])):
            continue
        hit = np.flatnonzero(matches(F[k], F[reps], tol)) if reps else []
        if len(hit):
            labels[k] = reps[hit[0]]
        else:
            labels[k] = k
            reps.append(k)
    return labels, np.array(reps, dtype=np.int64)


# ------------------------------------------------------------------------------ generators
def image(p, seed, reflect=None, shift=1.0):
    """The point p = [x | y | z] under a random orthogonal matrix (a reflection when ``reflect``; random when None), a
    translation of at most ``shift`` per coordinate and a random relabelling, computed in longdouble and rounded to fp64."""
    rng = np.random.default_rng(seed)
    P = np.asarray(p, dtype=np.float64).reshape(3, -1)
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(R))
    want = -1.0 if (rng.integers(2) == 1 if reflect is None else reflect) else 1.0
    if np.linalg.det(Q) * want < 0:
        Q[:, 0] = -Q[:, 0]
    Ql = Q.astype(LD)
    for _ in range(2):                                       # Newton-Schulz steps: orthogonal to longdouble rounding
        Ql = LD(1.5) * Ql - LD(0.5) * Ql @ (Ql.T @ Ql)
    out = Ql @ P.astype(LD) + rng.uniform(-shift, shift, size=(3, 1)).astype(LD)
    return np.asarray(out[:, rng.permutation(P.shape[1])], dtype=np.float64).reshape(-1)
