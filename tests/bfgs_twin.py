"""CPU twin of the dense BFGS update (``update_inverse_hessian!`` + the ``mul!`` behind it, legacy/DZOptimization.jl:864-889 and
:958-960) as csrc/dzo_bfgs.hip runs it.  A helper module for tests/test_bfgs_twin.py (which checks it against the CPU oracle and
against deliberately wrong results) and tests/test_gpu_bfgs_shapes.py (which checks the device kernels with it).  Pure numpy,
no fixtures, not a conftest.

Three tools:

* ``replay_update``: the rank-2 update ``H0 + (delta*(s_i*s_j) - (t_i*s_j + s_i*t_j))`` has one rounding per operation in the
  element type T, which is what numpy's elementwise arithmetic does.  Given the ``t = H0*dg`` the kernel stored, everything in
  it is known except two scalars, ``overlap`` (through ``s = d * (1/overlap)``, :874) and ``delta`` (:876), and both are sums
  whose order the kernel is free to choose.  So the checker searches the few values of T each of them can take (windows derived
  from the a-priori error of the sum, below) and passes iff some pair reproduces EVERY element of the new H bit for bit.
* ``sum_bound``: the error bound of a double-accumulated product ``H*v`` rounded once to T, for t and for the fused direction.
* ``mfma_bound``: the elementwise bound of the MFMA form of the update, which rounds as an fma chain.

and the shape tables ``FULL_F64`` / ``FULL_F32`` / ``TRI`` / ``MFMA`` with the path functions ``takes_vec`` / ``takes_tri`` that
say which kernel instantiation a shape runs.
"""
import collections
import math

import numpy as np

LD = np.longdouble
CAP = 4096                      # candidates per scalar and side: a case whose a-priori window is wider is a badly chosen input


def unit_roundoff(dtype):
    """u_T = 2^-24 (fp32) / 2^-53 (fp64)."""
    return float(np.finfo(np.dtype(dtype)).eps) / 2.0


def ulp(x, dtype):
    """Spacing of T at |x| (x any real, taken in longdouble): 2^(e - p + 1) for 2^e <= |x| < 2^(e+1)."""
    fi = np.finfo(np.dtype(dtype))
    ax = abs(LD(x))
    if ax < LD(fi.tiny):
        return float(fi.tiny) * float(fi.eps)
    e = math.frexp(float(ax))[1] - 1                    # (float(): a longdouble within a rounding of a power of two may move
    if LD(2.0) ** e > ax:                               #  across it; put it back)
        e -= 1
    return math.ldexp(float(fi.eps), e)


# ------------------------------------------------------------------------------ neighbours of a value of T
def _ordered(x):
    """float array -> int64 keys that count the values of the type in order (sign-magnitude bits unfolded)."""
    it = np.int32 if x.dtype == np.float32 else np.int64
    b = x.view(it).astype(np.int64)
    return np.where(b >= 0, b, np.int64(np.iinfo(it).min) - b)


def _unordered(k, dtype):
    it = np.int32 if np.dtype(dtype) == np.float32 else np.int64
    b = np.where(k >= 0, k, np.int64(np.iinfo(it).min) - k)
    return b.astype(it).view(dtype)


def candidates(exact, W, dtype):
    """The value of T nearest ``exact``, then its neighbours outward, W on each side: 2 W + 1 values of T."""
    dtype = np.dtype(dtype)
    x0 = np.array([LD(exact)]).astype(dtype)
    assert np.isfinite(x0[0]), "overflow"
    off = np.zeros(2 * W + 1, np.int64)
    off[1::2] = np.arange(1, W + 1)
    off[2::2] = -np.arange(1, W + 1)
    return _unordered(_ordered(x0)[0] + off, dtype)


# ------------------------------------------------------------------------------ the replay
Replay = collections.namedtuple("Replay", "ok overlap delta tried window_overlap window_delta reason")


def overlap_window(d, dg, acc_bits):
    """(exact, W): overlap = sum d_i dg_i in longdouble and the a-priori window of a length-n fma sum accumulated with
    ``acc_bits`` of mantissa and rounded to T: |error| <= n 2^-acc_bits sum |d_i dg_i| to first order, plus the final
    rounding, which moves the result by at most one more value."""
    T = d.dtype
    terms = d.astype(LD) * dg.astype(LD)
    exact = terms.sum()
    W = int(math.ceil(float(d.size * LD(2.0) ** -acc_bits * np.abs(terms).sum()) / ulp(exact, T))) + 1
    return exact, W


def overlap_candidates(d, dg, acc_bits, d_scaled=None):
    """Values of T the kernel's overlap (:873) can have, nearest first.  With ``d_scaled`` (the direction as :874 left it) only
    those whose reciprocal reproduces it bit for bit -- a check of :874 by itself.  Returns (candidates, W)."""
    T = d.dtype
    exact, W = overlap_window(d, dg, acc_bits)
    if W > CAP or exact == 0:
        return np.zeros(0, T), W
    c = candidates(exact, W, T)
    c = c[c != 0]
    if d_scaled is not None:
        inv = T.type(1) / c
        m = int(np.argmax(np.abs(d)))
        c = c[d[m] * inv == d_scaled[m]]                       # (one element first: cheap)
        c = np.array([x for x in c if np.array_equal(d * (T.type(1) / x), d_scaled)], T)
    return c, W


def update_expression(H0, s, t, delta):
    """H0 + (delta*(s_i*s_j) - (t_i*s_j + s_i*t_j)), one rounding per operation in T (:882-884 as written)."""
    T = H0.dtype
    assert s.dtype == T and t.dtype == T and np.dtype(type(delta)) == T
    return H0 + (delta * np.multiply.outer(s, s) - (np.multiply.outer(t, s) + np.multiply.outer(s, t)))


def replay_update(H0, d, dg, t, H_new, d_scaled=None, lam=None, acc_bits=53, lam_rel=0.0):
    """Does some (overlap, delta) reproduce every element of ``H_new`` bit for bit?

    H0, H_new: (n, n) arrays of T indexed [i, j]; d: the UNSCALED direction; dg; t: the H0*dg the kernel stored (its rounding
    is not at issue here, ``sum_bound`` is for that).

    For each overlap candidate c (``overlap_candidates``): inv = T(1)/c, s = d*inv.  delta is fitted from the element with
    the largest |s_i s_j| (the diagonal one at i = j = argmax |s|), in longdouble,
        est = ((H_new_ij - H0_ij) + (t_i s_j + s_i t_j)) / (s_i s_j).
    The expression rounds six times (s_i s_j, delta *, the two products, their sum, the difference) and the sum into H0 once
    more; every one of these errors is at most u_T times a quantity below A_ij = |H_new_ij| + |H0_ij| + 2(|t_i s_j| + |s_i t_j|)
    (|delta s_i s_j| <= |H_new - H0| + |t s| + |s t| up to rounding), so |est - delta| <= 4 u_T A_ij / |s_i s_j| and the
    window is W_delta = ceil(4 u_T A_ij / (|s_i s_j| ulp_T(est))) + 1.  Every delta candidate is tried on column j alone, a
    survivor on the whole matrix.

    Afterwards, with ``lam`` known: the fitted delta must lie within
        (n + 4) 2^-acc_bits (|lam| sum|d dg| + sum|dg t|) + 2 ulp_T + lam_rel |lam c|
    of lam*c + sum dg_i t_i (:876: n fma steps of the sum, the product, the sum of the two and the rounding of the sum to T;
    ``lam_rel`` is the relative uncertainty of a lam the caller could only estimate).

    Returns Replay(ok, overlap, delta, tried, window_overlap, window_delta, reason); ``tried`` counts (c, delta) pairs."""
    T = H0.dtype
    one = T.type(1)
    n = d.size
    assert H0.shape == (n, n) and H_new.shape == (n, n)
    for a in (d, dg, t, H_new) + ((d_scaled,) if d_scaled is not None else ()):
        assert a.dtype == T
    H0, H_new = np.ascontiguousarray(H0), np.ascontiguousarray(H_new)
    u = unit_roundoff(T)
    cands, W = overlap_candidates(d, dg, acc_bits, d_scaled)
    if W > CAP:
        return Replay(False, None, None, 0, W, 0, "overlap window %d exceeds the cap: badly chosen input" % W)
    if cands.size == 0:
        return Replay(False, None, None, 0, W, 0, "no overlap candidate reproduces d_scaled" if d_scaled is not None else "overlap is zero")
    tried, wd_max, seen = 0, 0, set()
    with np.errstate(all="ignore"):
        for c in cands:
            inv = one / c
            if inv.tobytes() in seen or not np.isfinite(inv):
                continue
            seen.add(inv.tobytes())
            s = d * inv
            m = int(np.argmax(np.abs(s)))
            ss = LD(s[m]) * LD(s[m])
            if ss == 0:
                continue
            ts = LD(t[m]) * LD(s[m])
            est = ((LD(H_new[m, m]) - LD(H0[m, m])) + (ts + ts)) / ss
            A = abs(LD(H_new[m, m])) + abs(LD(H0[m, m])) + 4 * abs(ts)
            if not np.isfinite(est):
                continue
            Wd = int(math.ceil(float(4 * u * A / ss) / ulp(est, T))) + 1
            wd_max = max(wd_max, Wd)
            if Wd > CAP:
                return Replay(False, c, None, tried, W, Wd, "delta window %d exceeds the cap: badly chosen input" % Wd)
            dc = candidates(est, Wd, T)
            tried += dc.size
            col = H0[:, m][None, :] + (dc[:, None] * (s * s[m])[None, :] - (t * s[m] + s * t[m])[None, :])
            want_col = np.ascontiguousarray(H_new[:, m]).view(np.uint8)
            for k in np.nonzero((np.ascontiguousarray(col).view(np.uint8) == want_col[None, :]).all(axis=1))[0]:
                delta = dc[k]
                full = update_expression(H0, s, t, delta)
                if not np.array_equal(full.view(np.uint8), H_new.view(np.uint8)):
                    continue
                if lam is not None:
                    terms = dg.astype(LD) * t.astype(LD)
                    want = LD(lam) * LD(c) + terms.sum()
                    bound = (n + 4) * LD(2.0) ** -acc_bits * (abs(LD(lam)) * np.abs(d.astype(LD) * dg.astype(LD)).sum() + np.abs(terms).sum()) \
                        + 2 * ulp(want, T) + lam_rel * abs(LD(lam) * LD(c))
                    if not abs(LD(delta) - want) <= bound:
                        return Replay(False, c, delta, tried, W, wd_max,
                                      "delta %r is %g from lam*overlap + dg.t = %r, bound %g" % (delta, float(abs(LD(delta) - want)), float(want), float(bound)))
                return Replay(True, c, delta, tried, W, wd_max, "")
    return Replay(False, None, None, tried, W, wd_max, "no (overlap, delta) among %d pairs reproduces H_new" % tried)


# ------------------------------------------------------------------------------ sums
def exact_matvec(H, v):
    """H*v in longdouble (64-bit mantissa on x86) and, per row, sum_j |H_ij v_j|."""
    terms = H.astype(LD) * v.astype(LD)[None, :]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def sum_bound(H, v, n, dtype):
    """Per row: ((n + 2) 2^-53 + u_T) sum_j |H_ij v_j|.

    The kernels convert both factors to double (exact), accumulate with fma in double -- per thread, then across the wave,
    then across the block, for the lower-triangle path further across its row and column partials, all in double -- and
    round the total once to T.  A sum of n terms by n - 1 additions in ANY order has error at most (n - 1) 2^-53 sum |terms|
    to first order (each term passes through at most n - 1 roundings, each relative 2^-53); the fma folds the product's
    rounding into the addition's, a term that starts a chain is rounded once as a product: n 2^-53 covers both, and (n + 2)
    leaves room for the second-order terms and for the 2^-64 of the longdouble reference itself.  The final rounding to T adds
    u_T |sum| <= u_T sum |terms|.  The exact value is the longdouble product with the matrix the device actually holds."""
    _, S = exact_matvec(H, v)
    return ((n + 2) * LD(2.0) ** -53 + LD(unit_roundoff(dtype))) * S


def mfma_bound(H0, d_scaled, t, lam, overlap, dg):
    """(exact, bound) per element for the MFMA form H += [d' t] [delta d' - t, -d']^T (fp64).

    exact_ij = H0_ij + delta_LD d'_i d'_j - (t_i d'_j + d'_i t_j) in longdouble, delta_LD = lam overlap + sum dg t, from the
    device's own d', t and overlap.  The kernel forms a_j = delta d'_j - t_j (two roundings: 2 u (|delta d'_j| + |t_j|), carried
    into the element times |d'_i|), then accumulates H0 + d'_i a_j + t_i (-d'_j) as fused multiply-adds onto H0, at most one
    rounding per step, each of a partial sum no larger than |H0| + (|delta d'_j| + |t_j|) |d'_i| + |d'_j| |t_i|: together below
    4 u times that.  Its delta is T(lam overlap + T(sum dg t)) with the sum of n fma steps in double: (n + 4) 2^-53 (|lam ov| +
    sum |dg t|), carried into the element times |d'_i d'_j|.  u = 2^-53."""
    n = t.size
    u = LD(2.0) ** -53
    dl, tl = d_scaled.astype(LD), t.astype(LD)
    terms = dg.astype(LD) * tl
    delta = LD(lam) * LD(overlap) + terms.sum()
    dd = np.multiply.outer(dl, dl)
    exact = H0.astype(LD) + (delta * dd - (np.multiply.outer(tl, dl) + np.multiply.outer(dl, tl)))
    aj = np.abs(delta * dl) + np.abs(tl)
    bound = 4 * u * (np.abs(H0.astype(LD)) + np.abs(dl)[:, None] * aj[None, :] + np.abs(tl)[:, None] * np.abs(dl)[None, :]) \
        + (n + 4) * u * (abs(LD(lam) * LD(overlap)) + np.abs(terms).sum()) * np.abs(dd)
    return exact, bound


# ------------------------------------------------------------------------------ shapes
# Full storage: a block is 256 threads, each takes 16 bytes per iteration (2 doubles, 4 floats) when the VEC instantiation
# runs and one element otherwise; a block owns a group of 4 columns, so n mod 4 is the ragged last group.
FULL_F64 = [
    1, 2, 3, 4,     # the four column-group tails n mod 4 = 1, 2, 3, 0; n = 1: a single thread has work; 2, 4: one vector / two
    5, 7,           # a second column group with 1 / 3 columns; scalar path
    127, 128, 129,  # two waves of double2 (64 lanes x 2) exactly, and one element either side
    511, 512, 513,  # one block stride of the vector path (256 threads x 2), -1 / +1 element: 513 is the scalar path's third trip
    514,            # the stride + one vector: the second trip has one active thread
    1025,           # two strides + 1, scalar, n mod 4 = 1
]
FULL_F32 = [
    1, 2, 3, 4,     # column-group tails; 4: exactly one float4
    5, 7, 8,        # second group with 1 / 3 columns (scalar: n mod 4 != 0); 8: two vectors
    255, 256, 257,  # one wave of float4 (64 lanes x 4) exactly, and one element either side
    1020,           # the block stride - one vector: the last thread idle
    1023, 1024, 1025,   # one block stride (256 threads x 4), -1 / +1 element
    1028,           # the stride + one vector
]
# Lower triangle (even n): 32-column windows, 256-row panels, interior tiles (a whole window left of a whole panel inside the
# matrix) in a separate code form, 32-row reduce blocks whose 8 groups each keep 8 window loads in flight (64 windows = 2048
# columns per trip of the reduce kernel's loop).
TRI = [
    2,              # one row pair
    30, 32, 34,     # the first window's edge: short of it, exact, a second window of 2 columns
    62, 64, 66,     # the second window's edge
    254, 256, 258,  # the first panel's edge: short of it, exact, a second panel with a single row pair
    286, 288,       # second panel, its diagonal window (columns 256..287) cut at 286 / whole at 288
    510, 512, 514,  # 512: the first size with interior tiles (panel 1, windows 0..7); 510 the last without, 514 a third panel
    770,            # three panels and a ragged fourth (2 rows), 25th window of 2 columns; interior tiles in two panels
    2050,           # 65 windows: the reduce kernel's window loop runs a second time for rows >= 2048, ragged 9th panel
]
MFMA = [16, 48, 80, 112, 256]   # 1, 3, 5, 7, 16 tiles per dimension: a wave walks the column tiles 4 at a time, so with 3, 5 and 7
#                                 the last job of a strip ends early (3, 1, 3 tiles) -- at 5 and 7 with full jobs in front of it

# operands whose 16-byte alignment each launcher asks for before it takes the VEC instantiation (names as in
# launch_bfgs_update / launch_bfgs_update_fused; the standalone update calls launch_symv with v = dg)
VEC_OPERANDS = {
    "symv": ("H", "v"),
    "update": ("H", "d", "scratch", "g"),                  # g only when given
    "fused": ("H", "d", "dg", "scratch", "g"),             # both kernels of the fused pair
}
TRI_DEFAULT_BYTES = 128 << 20
TRI_MAX_N = 65535 * 32


def takes_vec(n, dtype, launcher, misaligned=()):
    """True when ``launcher`` ("symv", "update", "fused") runs its VEC = true instantiation for n elements of dtype with the
    operands named in ``misaligned`` NOT 16-byte aligned."""
    per = 16 // np.dtype(dtype).itemsize
    return n % per == 0 and not (set(misaligned) & set(VEC_OPERANDS[launcher]))


def takes_tri(n, dtype, tri_min_n=None):
    """True when step! keeps the lower triangle only (o->tri): even n, below the grid limit, and at least
    DZO_TUNE_BFGS_TRI_MIN_N when that is set, else H of 128 MiB or more."""
    big = n >= tri_min_n if tri_min_n is not None else n * n * np.dtype(dtype).itemsize >= TRI_DEFAULT_BYTES
    return n % 2 == 0 and big and n < TRI_MAX_N


# ------------------------------------------------------------------------------ inputs
def spd(n, seed, dtype):
    """A symmetric (bit for bit) positive definite H0 of T."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    H = M @ M.T / n + np.eye(n)
    return (0.5 * (H + H.T)).astype(dtype)


def update_inputs(n, dtype, seed=None):
    """(H0, d, dg, g, lam) for the standalone update: dg = d o w with w uniform in [0.5, 1.5], so every term of the overlap
    has one sign and its window stays small; lam > 0 and H0 positive definite, so lam*overlap and dg.t add without cancelling
    and the 2 ulp of the delta check are 2 ulp of either."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    H0 = spd(n, n if seed is None else seed, dtype)
    d = rng.standard_normal(n).astype(dtype)
    d[d == 0] = 1
    dg = (d * rng.uniform(0.5, 1.5, n).astype(dtype)).astype(dtype)
    g = rng.standard_normal(n).astype(dtype)
    return H0, d, dg, g, np.dtype(dtype).type(0.37)


def device_norm(d):
    """||d|| for the estimate lam = -last_step_length / ||d|| of the step path: the sum of squares (here in longdouble; step!
    sums in double, in its own order), rounded to T, the square root in T, as step! does before it keeps the norm as a host double
    and stores last_step_length = T(t_b * norm).  An APPROXIMATION of the device's norm: the two sums can differ in the last bits,
    and lam = T(-t_b) and the step length are rounded once more each.  The caller allows 3 u_T for all of it (lam_rel)."""
    T = d.dtype
    return np.sqrt(np.array([(d.astype(LD) ** 2).sum()]).astype(T))[0]
