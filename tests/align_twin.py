"""CPU twin of the alignment unit (dzo_align_batch_assign / dzo_align_batch_pairs), written from the rule include/dzo.h states:
the shortest augmenting path with its row order and tie rules, the starts in their order, the PCG32 draws of the random ones,
the cyclic Jacobi, Horn's quaternion.  fp64 throughout.  A helper module for tests/test_align_twin.py (which checks it against
things it does not depend on) and tests/test_gpu_align.py.  Not a conftest, no fixtures.

One thing differs from the device on purpose.  The costs c(i, j) are formed once per assignment as an N x N array (the same
values the device forms on the fly; ``lowmode_twin.fma64`` is the exact fused multiply-add).

Every sum over the particles takes ``order``.  ``"index"`` (the default) adds in plain index order, rows ascending where the sum
is over rows.  ``"device"`` is "THE ORDER OF EVERY SUM" of the header: column j belongs to lane j mod 64, a lane adds its
columns l, l + 64, ... in that order onto 0, lanes without a column hold 0, the 64 lane sums go up the xor tree (32, 16, 8, 4,
2, 1), and a sum over rows i is taken over the columns j = p(i) in that order.  With it, and the deterministic starts, the twin
replays the device bit for bit (the random starts call log, cospi and sinpi, which no header pins)."""
import math

import numpy as np

from lowmode_twin import fma64
from tempering_twin import pcg_raw, pcg_state
from vec_twin import _wave_sum_all

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


def wave_sum(v):
    """the sum of a vector indexed by column in the device's order: lane by lane, then the wave tree"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    lanes = np.zeros(64)
    for j0 in range(0, v.size, 64):
        chunk = v[j0:j0 + 64]
        lanes[:chunk.size] = lanes[:chunk.size] + chunk
    return float(_wave_sum_all(lanes)[0])


def particle_sum(v, order="index"):
    """the sum of one term per particle, ``v`` in the order of the particles the sum runs over"""
    assert order in ("index", "device"), order
    return seq_sum(v) if order == "index" else wave_sum(v)


def inverse(perm):
    """rowof: the row of every column of the permutation row -> column"""
    rowof = np.empty(len(perm), dtype=np.int64)
    rowof[np.asarray(perm)] = np.arange(len(perm))
    return rowof


def cost_matrix(a, b):
    """c(i, j) = fma(dz, dz, fma(dy, dy, dx dx)) of the (N, 3) arrays a and b"""
    d = a[:, None, :] - b[None, :, :]
    c = d[..., 0] * d[..., 0]
    c = fma64(d[..., 1].ravel(), d[..., 1].ravel(), c.ravel())
    c = fma64(d[..., 2].ravel(), d[..., 2].ravel(), c)
    return c.reshape(len(a), len(b))


def assign_costs(c, count=False):
    """The shortest augmenting path on the cost matrix c (N x N).  Returns (perm, u, v): perm[i] the column of row i.  With
    ``count`` a fourth value follows: ``{"scans": scans of every row (N,), "longest": the most scans of one row, "total":
    all scans, "tied": the scans at which more than one unvisited column holds the smallest slack}``."""
    n = len(c)
    u, v = np.zeros(n), np.zeros(n)
    rowof = np.full(n + 1, -1, dtype=np.int64)               # column n is the virtual one
    scans, tied = np.zeros(n, dtype=np.int64), 0
    for i in range(n):
        slack = np.full(n, np.inf)                           # a visited column's slack is never read again: it is put back to +inf
        way = np.full(n, n, dtype=np.int64)
        used, free = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
        rows = np.zeros(n, dtype=bool)                       # the rows of the visited columns, and row i
        rows[i] = True
        rowof[n] = i
        j0 = n
        for _ in range(n + 1):
            i0 = rowof[j0]
            if j0 < n:
                used[j0], free[j0], rows[i0], slack[j0] = True, False, True, np.inf
            cur = (c[i0] - u[i0]) - v
            better = cur < slack
            better &= free
            np.copyto(slack, cur, where=better)
            np.copyto(way, j0, where=better)
            j1 = int(np.argmin(slack))                       # the first among equal values
            if not free[j1]:                                 # (cannot happen with finite costs)
                j1 = int(np.flatnonzero(free)[0])
            delta = slack[j1]
            if count:
                scans[i] += 1
                tied += int(np.count_nonzero(slack == delta) > 1)
            np.add(u, delta, out=u, where=rows)
            np.subtract(v, delta, out=v, where=used)
            np.subtract(slack, delta, out=slack, where=free)
            j0 = j1
            if rowof[j0] < 0:
                break
        while j0 != n:
            j1 = way[j0]
            rowof[j0] = rowof[j1]
            j0 = j1
    perm = np.empty(n, dtype=np.int64)
    perm[rowof[:n]] = np.arange(n)
    if count:
        return perm, u, v, {"scans": scans, "longest": int(scans.max()), "total": int(scans.sum()), "tied": tied}
    return perm, u, v


def matched_cost(c, perm, order="index"):
    """sum_i c(i, p(i)): over i ascending, or over the columns j = p(i) in the device's order"""
    if order == "index":
        return seq_sum(c[np.arange(len(perm)), perm])
    return particle_sum(c[inverse(perm), np.arange(len(perm))], order)


def assign(a, b, order="index"):
    """(perm, cost) of the (N, 3) arrays a and b in the frames given"""
    c = cost_matrix(a, b)
    perm, _, _ = assign_costs(c)
    return perm, matched_cost(c, perm, order)


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


def principal_frame(p, order="index"):
    """the right-handed principal frame (columns) of the centred (N, 3) array p"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    xx, xy, xz, yy, yz, zz = (particle_sum(s, order) for s in (x * x, x * y, x * z, y * y, y * z, z * z))
    e, v = jacobi([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    order = sorted(range(3), key=lambda k: (e[k], k))
    f = np.array([[v[r][k] for k in order] for r in range(3)])
    det = (f[0][0] * (f[1][1] * f[2][2] - f[2][1] * f[1][2]) - f[1][0] * (f[0][1] * f[2][2] - f[2][1] * f[0][2])
           + f[2][0] * (f[0][1] * f[1][2] - f[1][1] * f[0][2]))
    if det < 0.0:
        f[:, 2] = -f[:, 2]
    return f, sorted(e)


def principal_rotations(a, b, order="index"):
    fa, _ = principal_frame(a, order)
    fb, _ = principal_frame(b, order)
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


def horn(a, bp, order="index"):
    """the proper rotation that brings the rows of bp onto the rows of a best.  The nine sums run over the rows of the two
    arrays as they are given: for ``order="device"`` pass them by column, ``horn(a[rowof], b0, "device")``."""
    s = [[particle_sum(bp[:, u] * a[:, v], order) for v in range(3)] for u in range(3)]
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


def distance(a, rot, bp, order="index"):
    """sqrt(sum |a_i - R bp_i|^2) over the rows of the two arrays as they are given (by column for ``order="device"``)"""
    d = a - rotate(rot, bp)
    c = d[:, 0] * d[:, 0]
    c = fma64(d[:, 1], d[:, 1], c)
    c = fma64(d[:, 2], d[:, 2], c)
    return math.sqrt(particle_sum(c, order))


def run_start(a, b0, rot, max_cycles, order="index"):
    """one alternation from `rot` on the centred arrays.  Returns (distance, perm, rot, cycles, status, distances per cycle)."""
    prev, status, history = None, CYCLE_LIMIT, []
    cycles = 0
    for _ in range(max_cycles):
        perm, _ = assign(a, rotate(rot, b0))
        if order == "index":
            ai, bj = a, b0[perm]                             # by row
        else:
            ai, bj = a[inverse(perm)], b0                    # by column: the term of column j has row rowof[j]
        rot = horn(ai, bj, order)
        cycles += 1
        history.append(distance(ai, rot, bj, order))
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


# Exact assignment inputs, (a, b) as (N, 3) arrays.  Every coordinate is an integer of magnitude <= 1024, so every cost
# (<= 3 * 2048^2), potential and slack (sums and differences of at most 2 N + 1 costs) and the matched cost (N costs) is an
# integer below 2^37: exact in fp64 in any order of summation, and the inputs are exact in fp32.
def line(n):
    """a_i = (i + 1, 0, 0), b_j = (-(j + 1), 0, 0): c(i, j) = (i + j + 2)^2, the assignment problem of the product matrix
    (i + 1)(j + 1).  The optimum is the reversal (the rearrangement inequality, strict), its cost n (n + 1)^2; row i finds its
    column only after a path through every matched one."""
    k = np.arange(1.0, n + 1.0)
    zero = np.zeros(n)
    return np.stack([k, zero, zero], axis=1), np.stack([-k, zero, zero], axis=1)


def line_cost(n):
    """sum_i (i + (n - 1 - i) + 2)^2"""
    return float(n * (n + 1) ** 2)


def _cube_side(n):
    side = 1
    while side ** 3 < n:
        side += 1
    return side + 1                                          # ceil(n^(1/3)) + 1


def lattice(n, seed):
    """n distinct points for a, and n for b, drawn without replacement from the integer cube of side ceil(n^(1/3)) + 1: few
    distinct costs, so most scans find their smallest slack on several columns"""
    rng = np.random.default_rng(seed)
    side = _cube_side(n)
    out = []
    for _ in range(2):
        cells = rng.choice(side ** 3, size=n, replace=False)
        out.append(np.stack([cells // (side * side), (cells // side) % side, cells % side], axis=1).astype(np.float64))
    return out[0], out[1]


def all_tie(n, seed=0):
    """every b_j is the same point, a small random integers: c(i, j) does not depend on j, every unvisited column ties at
    every scan, and the lowest-column rule gives the identity"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (n, 3)).astype(np.float64)
    return a, np.tile(np.array([3.0, -2.0, 5.0]), (n, 1))


def lane_tie(n, seed=0):
    """b_j.x = (j mod 64) mod 7, zero elsewhere, a small random integers: the columns l and l + 64 q of one lane are the same
    point, and seven classes of lanes tie with each other"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (n, 3)).astype(np.float64)
    b = np.zeros((n, 3))
    b[:, 0] = (np.arange(n) % 64) % 7
    return a, b


EXACT_KINDS = ("line", "lattice", "all_tie", "lane_tie")


def exact_case(kind, n):
    """(a, b) of one of EXACT_KINDS with the seeds the tests share"""
    return {"line": lambda: line(n), "lattice": lambda: lattice(n, 9000 + n), "all_tie": lambda: all_tie(n, 9100 + n),
            "lane_tie": lambda: lane_tie(n, 9200 + n)}[kind]()


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
          seed=0, order="index"):
    """The rule of dzo_align_batch_pairs for ONE pair (``[x | y | z]`` arrays).  Returns a Result with aligned (fp64, unrounded), perm, rotation (3 x 3, sign folded in), distance,
    best_trial, cycles, status, trial_distances and histories."""
    a_raw, b_raw = split(a_points, n), split(b_points, n)
    if not (np.isfinite(a_raw).all() and np.isfinite(b_raw).all()):
        n_orient = (trials & 1) + 4 * ((trials >> 1) & 1) + random_trials
        return Result(aligned=np.asarray(b_points, dtype=np.float64).copy(), perm=np.arange(n), rotation=np.eye(3), distance=np.nan,
                      best_trial=0, cycles=0, status=FAILED, trial_distances=np.full((2 if allow_inversion else 1) * n_orient, np.nan),
                      histories=[])
    ca = np.array([particle_sum(a_raw[:, k], order) / n for k in range(3)])
    cb = np.array([particle_sum(b_raw[:, k], order) / n for k in range(3)])
    a, b = a_raw - ca, b_raw - cb
    runs = []
    for sign in ((1.0, -1.0) if allow_inversion else (1.0,)):
        b0 = sign * b
        rotations = []
        if trials & TRIAL_IDENTITY:
            rotations.append(np.eye(3))
        if trials & TRIAL_PRINCIPAL:
            rotations += principal_rotations(a, b0, order)
        rotations += [random_rotation(seed, r) for r in range(random_trials)]
        for rot in rotations:
            runs.append((sign,) + run_start(a, b0, rot, max_cycles, order))
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
