"""CPU twin of the alignment unit (dzo_align_batch_assign / dzo_align_batch_pairs), written from the rule include/dzo.h states:
the shortest augmenting path with its row order and tie rules, the starts in their order, the PCG32 draws of the random ones,
the cyclic Jacobi, Horn's quaternion.  fp64 throughout.  A helper module for tests/test_align_twin.py (which checks it against
things it does not depend on) and tests/test_gpu_align.py.  Not a conftest, no fixtures.

Two things differ from the device on purpose.  The costs c(i, j) are formed once per assignment as an N x N array (the same
values the device forms on the fly; ``lowmode_twin.fma64`` is the exact fused multiply-add).  Sums over the particles run in
plain index order here and lane by lane, then up the wave tree, on the device: the tests allow for that."""
import math

import numpy as np

from lowmode_twin import fma64
from tempering_twin import pcg_raw, pcg_state

TRIAL_IDENTITY, TRIAL_PRINCIPAL = 1, 2
CONVERGED, CYCLE_LIMIT, FAILED = 0, 1, 2
MAX_RANDOM_TRIALS = 64
SWEEPS = 12
SIGNS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))
_M64 = (1 << 64) - 1
_MUL, _INC = 0x5851F42D4C957F2D, 0x14057B7EF767814F


def split(points, n):
    """(N, 3) fp64 array of one point ``[x | y | z]``."""
    return np.asarray(points, dtype=np.float64).reshape(3, n).T.copy()


def join(xyz):
    """``[x | y | z]`` of an (N, 3) array."""
    return np.ascontiguousarray(np.asarray(xyz).T).reshape(-1)


def seq_sum(v):
    """the sum of a vector in index order"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def cost_matrix(a, b):
    """c(i, j) = fma(dz, dz, fma(dy, dy, dx dx)) of the (N, 3) arrays a and b"""
    d = a[:, None, :] - b[None, :, :]
    c = d[..., 0] * d[..., 0]
    c = fma64(d[..., 1].ravel(), d[..., 1].ravel(), c.ravel())
    c = fma64(d[..., 2].ravel(), d[..., 2].ravel(), c)
    return c.reshape(len(a), len(b))


def assign_costs(c):
    """The shortest augmenting path on the cost matrix c (N x N).  Returns (perm, u, v): perm[i] the column of row i."""
    n = len(c)
    u, v = np.zeros(n), np.zeros(n)
    rowof = np.full(n + 1, -1, dtype=np.int64)               # column n is the virtual one
    for i in range(n):
        slack = np.full(n, np.inf)
        way = np.full(n, n, dtype=np.int64)
        used = np.zeros(n, dtype=bool)
        rowof[n] = i
        j0 = n
        for _ in range(n + 1):
            i0 = rowof[j0]
            if j0 < n:
                used[j0] = True
            free = ~used
            cur = (c[i0] - u[i0]) - v
            better = free & (cur < slack)
            slack[better] = cur[better]
            way[better] = j0
            cand = np.where(free, slack, np.inf)
            j1 = int(np.argmin(cand))                        # the first among equal values
            if not free[j1]:                                 # (cannot happen with finite costs)
                j1 = int(np.flatnonzero(free)[0])
            delta = slack[j1]
            rows = rowof[:n][used]
            u[rows] += delta
            u[i] += delta
            v[used] -= delta
            slack[free] -= delta
            j0 = j1
            if rowof[j0] < 0:
                break
        while j0 != n:
            j1 = way[j0]
            rowof[j0] = rowof[j1]
            j0 = j1
    perm = np.empty(n, dtype=np.int64)
    perm[rowof[:n]] = np.arange(n)
    return perm, u, v


def assign(a, b):
    """(perm, cost) of the (N, 3) arrays a and b in the frames given; the cost is summed over i ascending."""
    c = cost_matrix(a, b)
    perm, _, _ = assign_costs(c)
    return perm, seq_sum(c[np.arange(len(a)), perm])


def jacobi(m):
    """(eigenvalues, V) of a small symmetric matrix by the cyclic Jacobi of the header; python floats."""
    d = len(m)
    a = [[float(m[i][j]) for j in range(d)] for i in range(d)]
    v = [[1.0 if i == j else 0.0 for j in range(d)] for i in range(d)]
    for _ in range(SWEEPS):
        moved = False
        for p in range(d - 1):
            for q in range(p + 1, d):
                apq = a[p][q]
                if apq == 0.0 or apq != apq:
                    continue
                moved = True
                theta = (a[q][q] - a[p][p]) / (apq + apq)
                root = math.sqrt(theta * theta + 1.0)
                t = 1.0 / (theta + root) if theta >= 0.0 else -1.0 / (root - theta)
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(d):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
                for k in range(d):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
                a[p][q] = a[q][p] = 0.0
        if not moved:
            break
    return [a[i][i] for i in range(d)], v


def quat_rotation(w, x, y, z):
    n = math.sqrt((w * w + x * x) + (y * y + z * z))
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[(w * w + x * x) - (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), (w * w - x * x) + (y * y - z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), (w * w - x * x) - (y * y - z * z)]])


def principal_frame(p):
    """the right-handed principal frame (columns) of the centred (N, 3) array p"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    xx, xy, xz, yy, yz, zz = (seq_sum(s) for s in (x * x, x * y, x * z, y * y, y * z, z * z))
    e, v = jacobi([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    order = sorted(range(3), key=lambda k: (e[k], k))
    f = np.array([[v[r][k] for k in order] for r in range(3)])
    det = (f[0][0] * (f[1][1] * f[2][2] - f[2][1] * f[1][2]) - f[1][0] * (f[0][1] * f[2][2] - f[2][1] * f[0][2])
           + f[2][0] * (f[0][1] * f[1][2] - f[1][1] * f[0][2]))
    if det < 0.0:
        f[:, 2] = -f[:, 2]
    return f, sorted(e)


def principal_rotations(a, b):
    fa, _ = principal_frame(a)
    fb, _ = principal_frame(b)
    out = []
    for d0, d1, d2 in SIGNS:
        out.append(np.array([[(d0 * fa[r][0] * fb[c][0] + d1 * fa[r][1] * fb[c][1]) + d2 * fa[r][2] * fb[c][2] for c in range(3)]
                             for r in range(3)]))
    return out


def _jump(state, k):
    """k advances of the LCG at once"""
    ra, rc, a, c = 1, 0, _MUL, _INC
    while k:
        if k & 1:
            ra, rc = (ra * a) & _M64, (rc * a + c) & _M64
        c = (c * (a + 1)) & _M64
        a = (a * a) & _M64
        k >>= 1
    return (ra * state + rc) & _M64


def random_rotation(seed, r):
    """random trial r (of every pair): four draws at position 4 r of the stream of `seed`"""
    state = _jump(pcg_state(int(seed) & _M64), 4 * int(r))
    d, _ = pcg_raw(state, 4)
    u = (d.astype(np.float64) + 0.5) * 2.0 ** -32
    r1, r2 = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
    return quat_rotation(r1 * math.cos(2.0 * math.pi * u[1]), r1 * math.sin(2.0 * math.pi * u[1]),
                         r2 * math.cos(2.0 * math.pi * u[3]), r2 * math.sin(2.0 * math.pi * u[3]))


def rotate(rot, p):
    """(R0 x + R1 y) + R2 z of every row of p"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(rot[k][0] * x + rot[k][1] * y) + rot[k][2] * z for k in range(3)], axis=1)


def horn(a, bp):
    """the proper rotation that brings the rows of bp onto the rows of a best"""
    s = [[seq_sum(bp[:, u] * a[:, v]) for v in range(3)] for u in range(3)]
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = s
    h = [[(sxx + syy) + szz, syz - szy, szx - sxz, sxy - syx],
         [syz - szy, (sxx - syy) - szz, sxy + syx, szx + sxz],
         [szx - sxz, sxy + syx, (syy - sxx) - szz, syz + szy],
         [sxy - syx, szx + sxz, syz + szy, (szz - sxx) - syy]]
    e, v = jacobi(h)
    top = 0
    for k in range(1, 4):
        if e[k] > e[top]:
            top = k
    return quat_rotation(v[0][top], v[1][top], v[2][top], v[3][top])


def distance(a, rot, bp):
    d = a - rotate(rot, bp)
    c = d[:, 0] * d[:, 0]
    c = fma64(d[:, 1], d[:, 1], c)
    c = fma64(d[:, 2], d[:, 2], c)
    return math.sqrt(seq_sum(c))


def run_start(a, b0, rot, max_cycles):
    """one alternation from `rot` on the centred arrays.  Returns (distance, perm, rot, cycles, status, distances per cycle)."""
    prev, status, history = None, CYCLE_LIMIT, []
    cycles = 0
    for _ in range(max_cycles):
        perm, _ = assign(a, rotate(rot, b0))
        rot = horn(a, b0[perm])
        cycles += 1
        history.append(distance(a, rot, b0[perm]))
        if prev is not None and np.array_equal(prev, perm):
            status = CONVERGED
            break
        prev = perm
    return history[-1], perm, rot, cycles, status, history


# ------------------------------------------------------------------------------ inputs the tests share
RECOVERY_SIZES = (2, 3, 5, 13, 38, 65)
ICOSAHEDRON_SEED = 5                                         # with 8 random trials every case of icosahedron_cases() is recovered
ICOSAHEDRON_CASES = 6


def ball_points(rng, n):
    """n points uniform in the unit ball, (N, 3)"""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * rng.random(n)[:, None] ** (1.0 / 3.0)


def proper_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def scramble(xyz, rng, invert=False):
    """(b, planted): b_i = s R xyz[planted[i]] + t"""
    n = len(xyz)
    planted = rng.permutation(n)
    rot, shift = proper_rotation(rng), rng.standard_normal(3)
    return (-1.0 if invert else 1.0) * xyz[planted] @ rot.T + shift, planted


def two_answers(n, inverted):
    """(the permutation, the sign of the determinant) is not unique for a planted motion.  A centred pair of points is swapped
    by a half turn, so N = 2 has two exact permutations.  Up to three centred points lie in a plane through the origin, where
    the inversion IS a proper rotation (the half turn about the normal), so an inverted input of N <= 3 has two exact signs."""
    return n == 2, inverted and n <= 3


def icosahedron():
    """the 13-atom icosahedron (centre and 12 vertices at distance 1): every second-moment eigenvalue is the same"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(0, s1, s2 * g) for s1 in (-1, 1) for s2 in (-1, 1)]
    v = v + [(y, z, x) for x, y, z in v] + [(z, x, y) for x, y, z in v]
    v = np.array(v, dtype=np.float64) / math.sqrt(1.0 + g * g)
    return np.vstack([np.zeros((1, 3)), v])


def icosahedron_cases():
    """[(a, b, planted)]: the icosahedron and scrambled copies of it, ``[x | y | z]`` arrays"""
    rng = np.random.default_rng(1313)
    ico = icosahedron()
    out = []
    for _ in range(ICOSAHEDRON_CASES):
        b, planted = scramble(ico, rng)
        out.append((join(ico), join(b), planted))
    return out


def recovery_cases(sizes=RECOVERY_SIZES, seed=2024):
    """[(n, inverted, a, b, planted)] of random ball points and scrambled copies, with and without inversion"""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        for inverted in (False, True):
            a = ball_points(rng, n)
            b, planted = scramble(a, rng, inverted)
            out.append((n, inverted, join(a), join(b), planted))
    return out


class Result:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def align(a_points, b_points, n, trials=TRIAL_IDENTITY | TRIAL_PRINCIPAL, random_trials=8, max_cycles=20, allow_inversion=False,
          seed=0):
    """The rule of dzo_align_batch_pairs for ONE pair (``[x | y | z]`` arrays).  Returns a Result with aligned (fp64, unrounded), perm, rotation (3 x 3, sign folded in), distance,
    best_trial, cycles, status, trial_distances and histories."""
    a_raw, b_raw = split(a_points, n), split(b_points, n)
    if not (np.isfinite(a_raw).all() and np.isfinite(b_raw).all()):
        n_orient = (trials & 1) + 4 * ((trials >> 1) & 1) + random_trials
        return Result(aligned=np.asarray(b_points, dtype=np.float64).copy(), perm=np.arange(n), rotation=np.eye(3), distance=np.nan,
                      best_trial=0, cycles=0, status=FAILED, trial_distances=np.full((2 if allow_inversion else 1) * n_orient, np.nan),
                      histories=[])
    ca = np.array([seq_sum(a_raw[:, k]) / n for k in range(3)])
    cb = np.array([seq_sum(b_raw[:, k]) / n for k in range(3)])
    a, b = a_raw - ca, b_raw - cb
    runs = []
    for sign in ((1.0, -1.0) if allow_inversion else (1.0,)):
        b0 = sign * b
        rotations = []
        if trials & TRIAL_IDENTITY:
            rotations.append(np.eye(3))
        if trials & TRIAL_PRINCIPAL:
            rotations += principal_rotations(a, b0)
        rotations += [random_rotation(seed, r) for r in range(random_trials)]
        for rot in rotations:
            runs.append((sign,) + run_start(a, b0, rot, max_cycles))
    dists = np.array([r[1] for r in runs])
    best = 0
    for t in range(1, len(runs)):
        if dists[t] < dists[best]:
            best = t
    sign, dist, perm, rot, cycles, status, _ = runs[best]
    srot = sign * rot
    aligned = rotate(srot, b[perm]) + ca
    return Result(aligned=join(aligned), perm=perm, rotation=srot, distance=dist, best_trial=best, cycles=cycles, status=status,
                  trial_distances=dists, histories=[r[6] for r in runs])
