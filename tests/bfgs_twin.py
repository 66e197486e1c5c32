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

For the batched kernel of csrc/dzo_batch.hip (tests/test_gpu_bfgs_batch_shapes.py), which keeps t = H0*dg in LDS: the table
``BATCH`` with ``batch_form``, the elementwise bound ``batch_update_bound`` of the update computed from its inputs alone, and for
fp32 ``t_rounded`` (the device's t is the rounding of the exact sum, up to a few undecided rows) with ``replay_update_undecided``.
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


# ------------------------------------------------------------------------------ the batched kernel (csrc/dzo_batch.hip)
BatchForm = collections.namedtuple("BatchForm", "rp wide uj lds_bytes needs_attribute")
BATCH_LDS_DEFAULT = 48 * 1024       # dynamic LDS a kernel may ask for before hipFuncAttributeMaxDynamicSharedMemorySize is needed
BATCH_WIDE_ABOVE = 448              # RP = 2: two columns in flight at two blocks per CU up to here, four at one block beyond
BATCH_FORMS = ("rp1", "rp2 narrow", "rp2 wide", "rp4")


def batch_form(n, dtype):
    """(rp, wide, uj, lds_bytes, needs_attribute) of batch_step_kernel for an even n in 2..1024, as batch_create_impl and the
    kernel's ``UJ`` line choose them: rp row pairs per thread (n <= 256 rp), the wide form of rp = 2 above 448, uj columns per
    chunk of the two-deep pipeline, and the dynamic LDS: nine vectors of T, then in double the half-combine scratch, four
    waves' column parts and 16 scalars, then a flag."""
    assert n % 2 == 0 and 2 <= n <= 1024
    rp = 1 if n <= 256 else (2 if n <= 512 else 4)
    wide = rp == 2 and n > BATCH_WIDE_ABOVE
    uj = 4 if rp == 1 else ((4 if wide else 2) if rp == 2 else 2)
    np_ = (n + 1) & ~1
    lds = 9 * np_ * np.dtype(dtype).itemsize + (5 * np_ + 16) * 8 + 16
    return BatchForm(rp, wide, uj, lds, lds > BATCH_LDS_DEFAULT)


def batch_form_name(n, dtype):
    f = batch_form(n, dtype)
    return "rp1" if f.rp == 1 else ("rp4" if f.rp == 4 else ("rp2 wide" if f.wide else "rp2 narrow"))


# Even n.  A thread owns the row pairs 2 (lane + 128 r), r < rp; the two 128-thread halves take the even / the odd columns, so a
# half has n / 2 columns, walks them uj at a time and two chunks (2 uj columns) per trip of the pipeline loop.
BATCH = [
    2,              # one row pair, one column per half: a chunk with 1 live column
    4, 6, 8,        # 2, 3, 4 live columns in the first chunk (uj = 4); the pair (j - 1, j) of every odd column straddles the diagonal
    10,             # 5 columns per half: a second chunk with one live column
    14, 16, 18,     # 7 / 8 / 9 columns per half: short of one whole pipeline trip (2 uj = 8), exactly one, one column more
    30, 32, 34,     # two trips' edge
    62, 64, 66,     # 32 row pairs: half a wave of each half has work; 66: 33 columns, a fifth trip with one column
    126, 128, 130,  # 64 row pairs = one whole wave per half; 130: the lane that starts the second wave of a half
    254, 256,       # 256: every thread of a half owns a pair, the last size of rp 1 (fp64: 28816 bytes of LDS)
    258,            # rp 2 narrow (uj = 2): the first thread with a second pair
    260, 262, 264, 266,   # 130 .. 133 columns per half against trips of 4: the last trip holds 2, 3, 4 (whole) and 1 columns
    384,            # the benchmarked size
    436, 438,       # fp64: 48976 / 49200 bytes of LDS, either side of the 48 KiB above which the attribute must be set
    446, 448,       # the last narrow sizes
    450,            # rp 2 wide (uj = 4): the first size of the form
    510, 512,       # 255 / 256 columns per half; 512: every thread owns two pairs, the last size of rp 2
    514, 516,       # rp 4 (uj = 2): one / two threads in the third row pair
    644, 646,       # fp32: 49088 / 49240 bytes of LDS, either side of 48 KiB
    768, 770,       # three whole row pairs per thread; 770: one thread in the fourth
    1022, 1024,     # the last sizes: 1024 is every thread with four pairs (fp64: 114832 bytes of LDS)
]
BATCH_ONE_PER_FORM = [130, 262, 450, 770]   # ragged in every form: a lone lane in the second wave, a last trip of 3 columns, the
#                                             first wide size, one thread in the fourth row pair
BATCH_SEEDS = (1000, 1003, 1006)            # starts of the trajectories: instance b of start k is pcg_fill(n, BATCH_SEEDS[k] + b)
UNDECIDED_CAP = 2                           # rows of t = H0*dg per step whose fp32 rounding the replay may have to search


def batch_update_bound(H0, d, dg, lam, dtype, lam_rel=0.0):
    """(exact, bound) per element [i, j] of the batched kernel's update H0 + (delta*(s_i*s_j) - (t_i*s_j + s_i*t_j)), first order.

    exact: in longdouble from H0, the UNSCALED direction d, dg and lam = -t_b alone: ov = sum d dg, t = H0 dg, q = sum dg t,
    delta = lam ov + q, s = d / ov.  Nothing the kernel computed enters it, so a wrong t, overlap or delta is seen as well as a
    wrong element.

    bound: the build uses -ffp-contract=off, so every operation of the element type T rounds once, relative error at most
    u = u_T; the three sums are accumulated in double in an order the kernel is free to choose and rounded once to T, so each
    is within a sum |terms| + u |sum| of the exact sum OF THE TERMS IT WAS GIVEN, a = (n + 2) 2^-53 (see ``sum_bound``).  Hats
    are the device's values.
      ov^ :  |ov^ - ov| <= a Sov + u |ov| = e_ov                                                 (Sov = sum |d dg|)
      s^_i = T(d_i T(1 / ov^)) = s_i (ov / ov^) (1 + e1)(1 + e2):  |s^_i - s_i| <= rho |s_i|,  rho = e_ov / |ov| + 2 u
      t^_i:  |t^_i - t_i| <= a St_i + u |t_i| = tau_i                                            (St_i = sum_j |H0_ij dg_j|)
      q^ = T(sum dg_i t^_i): the terms carry tau, the sum its own error: e_q = a Sq + sum |dg_i| tau_i + u |q|   (Sq = sum |dg t|)
      delta^ = T(T(lam ov^) + q^): |lam| e_ov + u |lam ov| from the product, e_q, and u |delta| <= u (|lam ov| + |q|) from the
               sum: e_delta = |lam| e_ov + e_q + 2 u (|lam ov| + |q|) (+ lam_rel |lam ov| for a lam known to lam_rel only)
    and for the element, with P = |delta s_i s_j|, Q = |t_i s_j| + |s_i t_j|:
      T(s^_i s^_j)               relative 2 rho + u
      T(delta^ . )               |s_i s_j| e_delta + (2 rho + 2 u) P
      T(t^_i s^_j), T(s^_i t^_j) tau_i |s_j| + tau_j |s_i| + (rho + u) Q
      their sum                  + u Q
      the difference             + u (P + Q)
      the sum into H0            + u (|H0_ij| + P + Q)
    in all  |s_i s_j| (e_delta + 2 rho |delta|) + tau_i |s_j| + tau_j |s_i| + rho Q + u (|H0_ij| + 4 P + 4 Q), and the last
    term is rounded up to 4 u (|H0_ij| + P + Q): the three spare u |H0_ij| stand for the second-order terms.  The bound is
    symmetric in i and j, as the expression is."""
    n = d.size
    u = LD(unit_roundoff(dtype))
    a = (n + 2) * LD(2.0) ** -53
    H, dl, yl, lam = H0.astype(LD), d.astype(LD), dg.astype(LD), LD(lam)
    ov_terms = dl * yl
    ov, Sov = ov_terms.sum(), np.abs(ov_terms).sum()
    t_terms = H * yl[None, :]
    t, St = t_terms.sum(axis=1), np.abs(t_terms).sum(axis=1)
    q_terms = yl * t
    q, Sq = q_terms.sum(), np.abs(q_terms).sum()
    delta = lam * ov + q
    s = dl / ov
    e_ov = a * Sov + u * abs(ov)
    rho = e_ov / abs(ov) + 2 * u
    tau = a * St + u * np.abs(t)
    e_q = a * Sq + (np.abs(yl) * tau).sum() + u * abs(q)
    e_delta = abs(lam) * e_ov + e_q + 2 * u * (abs(lam * ov) + abs(q)) + LD(lam_rel) * abs(lam * ov)
    ss = np.multiply.outer(s, s)
    ts, st = np.multiply.outer(t, s), np.multiply.outer(s, t)
    exact = H + (delta * ss - (ts + st))
    sa = np.abs(s)
    Q = np.abs(ts) + np.abs(st)
    bound = np.abs(ss) * (e_delta + 2 * rho * abs(delta)) + np.multiply.outer(tau, sa) + np.multiply.outer(sa, tau) + rho * Q \
        + 4 * u * (np.abs(H) + np.abs(delta * ss) + Q)
    return exact, np.maximum(bound, bound.T)                  # (equal up to the order of the longdouble sums behind them)


def overlap_cancellation(d, dg):
    """sum |d dg| / |sum d dg|: how much of the overlap's terms cancels (every bound and window above grows with it)."""
    terms = d.astype(LD) * dg.astype(LD)
    return float(np.abs(terms).sum() / abs(terms.sum())) if terms.sum() != 0 else float("inf")


def t_rounded(H0, dg, dtype=np.float32):
    """fp32: (t, undecided).  The batched kernel's t = H0*dg is a sum accumulated in double and rounded ONCE to fp32.  The
    products of two floats are exact in double, the double sum is within a St_i = (n + 2) 2^-53 sum_j |H0_ij dg_j| of the exact
    one in any order, and rounding is monotone: the device's t_i is the rounding of the exact sum (here: the longdouble sum,
    whose own n 2^-64 St_i the + 2 of a covers) unless a tie between two neighbouring floats lies within a St_i of it.
    Such rows are ``undecided``: a list of (row, the other candidate), the neighbour of t[row] across that tie."""
    assert np.dtype(dtype) == np.float32 and H0.dtype == np.float32 and dg.dtype == np.float32
    n = dg.size
    exact, S = exact_matvec(H0, dg)
    t = exact.astype(np.float32)
    w = (n + 2) * LD(2.0) ** -53 * S
    undecided = []
    for other in (np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))):
        tie = (t.astype(LD) + other.astype(LD)) / 2
        for i in np.nonzero(np.abs(exact - tie) <= w)[0]:
            undecided.append((int(i), other[i]))
    return t, undecided


def replay_update_undecided(H0, d, dg, t, undecided, H_new, **kw):
    """``replay_update`` over the 2^k values t can have when k of its rows are undecided (``t_rounded``); the first that
    reproduces H_new, else the last failure."""
    assert len(undecided) <= UNDECIDED_CAP, undecided
    r = None
    for mask in range(1 << len(undecided)):
        tt = t.copy()
        for k, (i, other) in enumerate(undecided):
            if mask >> k & 1:
                tt[i] = other
        r = replay_update(H0, d, dg, tt, H_new, **kw)
        if r.ok:
            return r
    return r


def batch_start(orc, n, dtype, k, b, quadratic=False):
    """start of instance b on trajectory k (``orc``: the oracle module; this one stays free of it)."""
    x = orc.pcg_fill(n, BATCH_SEEDS[k] + b)
    return (x - 0.5 if quadratic else x).astype(dtype)


def batch_matrix(orc, n, b, dtype, r=8):
    """A_b = D_b + U_b U_b'/r (positive definite, symmetric bit for bit), a different one per instance."""
    dvec = 1.0 + (9.0 + 30.0 * b) * orc.pcg_fill(n, 20 + b)
    U = (orc.pcg_fill(n * r, 40 + b) - 0.5).reshape(n, r, order="F")
    A = (U @ U.T) / r
    A[np.diag_indices(n)] += dvec
    return np.ascontiguousarray((0.5 * (A + A.T)).astype(dtype))


def batch_steps(n):
    """steps a trajectory is followed for: the first is the update of H = I, the later ones of a dense H."""
    return 2 if n >= 512 else 3
