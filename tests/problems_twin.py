"""CPU twin of the built-in objectives (csrc/dzo_problems.hip, csrc/dzo_rosen.h): launch shapes, probe points at which
every operation is exact, longdouble references with the magnitude sums, and error bounds read off the kernels operation
by operation.  A helper module for tests/test_problems_twin.py (which checks it against the oracle, a second
implementation, and checks that the bounds reject planted errors) and tests/test_gpu_problems.py.  Not a conftest, no
fixtures.

Kinds: ROSEN (chained Rosenbrock), QCHAIN (chained quadratic), QUAD (dense quadratic), LSE (log-sum-exp).

Launch shapes (dzo_common.h stream_grid, kBlock = 256, waves of 64, at most kMaxPartialBlocks = 2048 blocks)
-------------------------------------------------------------------------------------------------------------
``stream_grid(n, e) = clamp(ceil(n / (256 e)), 1, min(8 CUs, 2048))``.  N = 16 bytes / sizeof(T) (2 in fp64, 4 in fp32).

* ROSEN objective and gradient: grid = stream_grid(n, 2 N); a thread takes ONE vector of N elements per trip, so a trip
  covers grid * 256 * N elements; the n % N elements behind the last whole vector (the ragged tail) go to the first
  threads of block 0, one element each, after the loop.
* QCHAIN, LSE (max, sums, gradient), the decorators (sumsq, grad_decorate, box_clamp): grid = stream_grid(n, 4); a thread
  takes one element per trip, a trip covers grid * 256 elements.
* QUAD: block j takes column j (n < 65535 here): thread t walks i = t N + k 256 N in the vector form (n % N == 0), i = t +
  k 256 in the scalar form.
* The one-block finish kernels: thread t adds partials t, t + 256, ...

Exact probes
------------
At the probe points every operation of a kernel is exact (small dyadic numbers), so the value does not depend on the
order of the sums and the device must return these bits: see ``chain_probe``, ``quad_probe``, ``lse_probe``.

Bounds of the values: (k u_T + m u_64) S and how k and m are counted
----------------------------------------------------------------------
u_T = 2^-53 (fp64) or 2^-24 (fp32), u_64 = 2^-53, gamma(k, u) = k u / (1 - k u).  Every kernel adds its terms in fp64 (a
term computed in T converts exactly).  A sum whose longest chain of additions has m links has an error of at most
gamma(m, u_64) times the sum of the absolute values of its terms, whatever the order; a term that carries k roundings in T
on the longest path through its expression is off by at most ((1 + u_T)^k - 1) times the magnitude of its parts.  All terms
of the chain kinds are sums of squares, so the magnitude sum S is the value itself there.

k, read off dzo_rosen.h:

* rosen_term = fma(100 t2, t2, t1 t1), t1 = 1 - xi, t2 = fma(-xi, xi, xn): one subtraction, two fmas, two products.  The part
  100 t2^2 carries the rounding of t2 twice, of the product 100 t2 and of the outer fma: 4.  The part t1^2 carries the
  subtraction twice, the product and the outer fma: 4.  k = 4.
* qchain_term = fma(hk p, p, (hm d) d), p = xn - xi, d = xi - 1, hk = 1/2 or 0, hm = lambda / 2 (both scalings exact):
  hk p^2 carries p twice and the fma: 3; hm d^2 carries d twice, two products and the fma: 5.  k = 5.  lambda is used as
  (T)lambda by device and oracle; the twin takes it rounded to T (the cases use values that fp32 holds exactly).
* QUAD: the products live inside fp64 fmas (exact for fp32 operands, part of the link's one rounding in fp64): k = 0.

m, read off the kernels (block_sum = wave tree of 6 levels, then the 4 wave sums added in order):

* ROSEN: ceil(nvec / (grid 256)) trips of N additions, 1 for the tail term, 6 + 4, and the finish kernel: ceil(grid / 256) +
  6 + 4.
* QCHAIN and the two sums of LSE: ceil(n / (grid 256)) + 6 + 4, finish ceil(grid / 256) + 6 + 4.
* QUAD: column sum ceil(n / (256 N)) N + 6 + 4 links, one rounding for c_j x_j, finish ceil(n / 256) + 6 + 4.
  S = 1/2 sum_j |x_j| sum_i |A[i, j] x[i]|.

In fp32 dzo_problem_eval rounds the fp64 result to float: + u_T (|f| + error so far).

The gradient of QUAD: element j within (n + 1) u_64 sum_i |A[i, j] x[i]| + u_T |g_j| (n links at most, the rounding to T).
The gradients of the chain kinds are elementwise with the oracle's expressions: bit for bit against the oracle.

Log-sum-exp: f = mx + log(se) + (lambda / 2) sq
-----------------------------------------------
* mx: a maximum, exact.  d_i = x_i - mx is formed in T: off by at most u_T |d_i|, which changes exp by the factor
  exp(+-u_T |d_i|); exp and log in fp64 are within 1 ulp = 2 u_64 (the HIP math API's table for double precision); a result
  below the normal range is off by at most 2^-1075 more.  So a term e_i = exp(d_i) is off by e_i r_i + 2^-1075,
  1 + r_i = exp(u_T |d_i|) (1 + 2 u_64); se is off by E_se = (1 + gamma(m, u_64)) sum_i (e_i r_i + 2^-1075) + gamma(m, u_64) se.
* log(se) is off by -log(1 - E_se / se) + 2 u_64 |log se|.
* sq = sum (x_i - c_i)^2: the difference in T (twice), the square inside an fp64 fma: sq ((1 + u_T)^2 (1 + gamma(m, u_64)) - 1).
* (0.5 lambda) sq: one product; the two additions: 2 u_64 times the sum of the magnitudes of what is added.
* lambda in fp32.  include/dzo.h says only that scalars cross the ABI as double and names the objective "lambda/2 |x-c|^2"; it
  does not say whether an fp32 problem rounds lambda to float.  lse_finish_kernel and lse_grad_kernel use the double, the
  oracle its float rounding.  The header does not settle it, so the twin takes lambda as given and every fp32 bound of the
  lambda term carries the relative 2^-24 (u_lambda); neither side is changed.
* Gradient g_i = (T)(e_i / se + lambda (x_i - c_i)): the softmax part is off by the factor (1 + r_i)(1 + u_64) / (1 - E_se / se)
  (exp, division, the sum), the lambda part by (1 + u_T)(1 + u_64)(1 + u_lambda) (difference in T, product, lambda), the
  addition by u_64 of the magnitudes, the rounding to T by u_T |g_i| plus half the smallest subnormal of T.

L2 decorator: f + lambda2 ss, ss = sum x_i^2 (sumsq_kernel: fp64 fma chain, m as for QCHAIN; l2_finish_kernel)
-----------------------------------------------------------------------------------------------------------------
fp64: result + lambda2 ss in fp64: one product, one addition.  fp32 (l2_finish_kernel's to_f32 form): (float)f +
(float)lambda2 * (float)ss in float arithmetic: the base value rounded to float, lambda2 and ss rounded to float, one float
product, one float addition (5 roundings in T, of which the ss part carries 3 and the addition).

The reference's own error: sums are pairwise trees in longdouble (u_ld = 2^-64): at most (levels + 8) u_ld S, added to
every bound (8 covers the operations of a term, exp and log).
"""
import collections
import functools

import numpy as np

LD = np.longdouble
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
U64, U32, ULD = LD(2) ** -53, LD(2) ** -24, LD(2) ** -64
U = {F64: U64, F32: U32}
HALF_SUBNORMAL = {F64: LD(2) ** -1075, F32: LD(2) ** -150}
ULP_EXP, ULP_LOG = 1, 1                        # HIP math API, double precision: exp and log within 1 ulp
BLOCK, WAVE, WAVES, MAX_BLOCKS = 256, 64, 4, 2048
VEC = {F64: 2, F32: 4}
ROSEN, QCHAIN, QUAD, LSE = "rosen", "qchain", "quad", "lse"
KINDS = (ROSEN, QCHAIN, QUAD, LSE)
K_T = {ROSEN: 4, QCHAIN: 5, QUAD: 0}
PROBE_LAMBDA = 0.25                            # chained quadratic probes
QCHAIN_LAMBDA = 0.375                          # dense points of the chained quadratic (exact in fp32)
LSE_LAMBDA = 1e-2                              # not a float: the fp32 bounds carry u_lambda

_CHAIN_SIZES = (2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
SIZES = {
    ROSEN: _CHAIN_SIZES,
    QCHAIN: (1,) + _CHAIN_SIZES,
    LSE: (1,) + _CHAIN_SIZES,
    QUAD: (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 258, 1023, 1024, 1025, 1026, 1792, 1793, 2047, 2048, 2049),
}
DECORATOR_SIZES = (1, 255, 256, 257, 1023, 1025)
Value = collections.namedtuple("Value", "f S bound")


def gamma(k, u):
    return LD(k) * u / (1 - LD(k) * u)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------ launch shapes
def stream_grid(n, elems_per_thread, cus):
    return max(1, min(_cdiv(n, BLOCK * elems_per_thread), min(8 * cus, MAX_BLOCKS)))


def launch(kind, dtype, n, cus):
    """(grid, elements a thread takes per trip) of the streaming kernels of a kind ("decor": the decorators)"""
    N = VEC[np.dtype(dtype)]
    if kind == ROSEN:
        return stream_grid(n, 2 * N, cus), N
    assert kind in (QCHAIN, LSE, "decor")
    return stream_grid(n, 4, cus), 1


def capped_size(kind, dtype, cus):
    """the size at which the grid cap is reached, plus 3 (fp64) or 5 (fp32): a ragged tail and the start of another trip"""
    dtype = np.dtype(dtype)
    per_thread = 2 * VEC[dtype] if kind == ROSEN else 4
    return min(8 * cus, MAX_BLOCKS) * BLOCK * per_thread + (3 if dtype == F64 else 5)


def seams(kind, dtype, n, cus):
    """{name: index of the first element behind the seam} of every seam of a kind's kernels that lies inside 0 < s < n"""
    dtype = np.dtype(dtype)
    N = VEC[dtype]
    out = {}
    if kind == QUAD:                                   # the column loop, in both its forms
        cand = {"vector": N, "vector_mid": (n // 2) // N * N, "wave_scalar": WAVE, "wave_vector": WAVE * N,
                "trip_scalar": BLOCK, "trip_vector": BLOCK * N, "trip_last": (n - 1) // (BLOCK * N) * (BLOCK * N),
                "finish_unroll": 7 * BLOCK}
    else:
        grid, e = launch(kind, dtype, n, cus)
        trip = grid * BLOCK * e
        cand = {"vector": N, "vector_mid": (n // 2) // N * N, "wave": WAVE * e, "block": BLOCK * e, "trip": trip,
                "trip_last": (n - 1) // trip * trip, "tail": n // N * N if n % N else 0}
    for name, s in cand.items():
        if 0 < s < n:
            out[name] = s
    return out


def probe_positions(kind, dtype, n, cus):
    """first and last element, the last element with a right neighbour, both sides of every seam"""
    pos = {0, n - 1, n - 2}
    for s in seams(kind, dtype, n, cus).values():
        pos |= {s - 1, s}
    return sorted(p for p in pos if 0 <= p < n)


def probe_pairs(dtype, n):
    """(p, q) for the two-element probe of QUAD: p and q in different vectors, waves and trips of the column loop"""
    N = VEC[np.dtype(dtype)]
    cand = [(0, N), (N - 1, N), (1, WAVE * N + 1), (WAVE - 1, WAVE), (0, BLOCK), (BLOCK * N - 1, BLOCK * N), (2, n - 1), (n - 2, n - 1)]
    return sorted({(p, q) for p, q in cand if 0 <= p < q < n})


def term_block(kind, dtype, n, cus):
    """the block whose partial receives the term attributed to element i (the order of the objective kernels)"""
    dtype = np.dtype(dtype)
    i = np.arange(n, dtype=np.int64)
    if kind == QUAD:
        return i
    grid, e = launch(kind, dtype, n, cus)
    owner = (i // e) % (grid * BLOCK) // BLOCK
    if kind == ROSEN:
        owner[n // e * e:] = 0                         # the ragged tail: block 0
    return owner


def sum_depth(kind, dtype, n, cus):
    """m: the additions on the longest path of a value's sum (see the module docstring)"""
    dtype = np.dtype(dtype)
    N = VEC[dtype]
    if kind == QUAD:
        return (_cdiv(n, BLOCK * N) * N + 6 + WAVES, _cdiv(n, BLOCK) + 6 + WAVES)
    grid, e = launch(kind, dtype, n, cus)
    trips = _cdiv(_cdiv(n, e), grid * BLOCK)
    return trips * e + (1 if kind == ROSEN else 0) + 6 + WAVES + _cdiv(grid, BLOCK) + 6 + WAVES


# ------------------------------------------------------------------------------ longdouble sums
def tree_sum(v, axis=-1):
    """(pairwise sum along the axis in longdouble, levels of the tree)"""
    v = np.moveaxis(np.asarray(v, dtype=LD), axis, -1)
    levels = 0
    while v.shape[-1] > 1:
        m = v.shape[-1]
        s = v[..., 0:m - 1:2] + v[..., 1:m:2]
        v = np.concatenate([s, v[..., m - 1:]], axis=-1) if m % 2 else s
        levels += 1
    return (v[..., 0] if v.shape[-1] else np.zeros(v.shape[:-1], dtype=LD)), levels


def _ref_error(levels, S):
    return (levels + 8) * ULD * S


def _value_bound(kind, dtype, n, cus, f, S, levels):
    uT = U[dtype]
    E = S * ((1 + uT) ** K_T[kind] * (1 + gamma(sum_depth(kind, dtype, n, cus), U64)) - 1)
    if dtype == F32:
        E = E + uT * (abs(f) + E)
    return E + _ref_error(levels, S)


# ------------------------------------------------------------------------------ chain kinds
def rosen_terms(x):
    """the n - 1 terms 100 (x[i+1] - x[i]^2)^2 + (1 - x[i])^2 of the inputs as they are, in longdouble"""
    xl = np.asarray(x).astype(LD)
    t1 = 1 - xl[:-1]
    t2 = xl[1:] - xl[:-1] * xl[:-1]
    return 100 * t2 * t2 + t1 * t1


def qchain_terms(x, lam):
    """the n terms attributed to the elements: lambda/2 (x[i] - 1)^2 + 1/2 (x[i+1] - x[i])^2 (the last one without a pair)"""
    xl = np.asarray(x).astype(LD)
    lam = LD(np.asarray(x).dtype.type(lam))
    d = xl - 1
    t = lam / 2 * d * d
    p = xl[1:] - xl[:-1]
    t[:-1] += p * p / 2
    return t


def chain_terms(kind, x, lam=QCHAIN_LAMBDA):
    return rosen_terms(x) if kind == ROSEN else qchain_terms(x, lam)


def chain_value(kind, x, cus, lam=QCHAIN_LAMBDA, terms=None):
    """Value of a chain kind at x; ``terms`` replaces the twin's own terms (the planted errors of the CPU test)"""
    x = np.asarray(x)
    t = chain_terms(kind, x, lam) if terms is None else terms
    f, levels = tree_sum(t)                            # every term is a sum of squares: S = f
    return Value(f, f, _value_bound(kind, x.dtype, x.size, cus, f, f, levels))


def chain_probe(kind, n, p):
    """x = 1 everywhere but x[p] = 1.5: (value, {index: gradient element}) -- every operation exact in fp32 and fp64.  All
    other gradient elements are zeros: +0, except element 0 of ROSEN, which is fma(-400, +0, -2 (+0)) = -0 (n > 1)."""
    left, right = p > 0, p + 1 < n
    if kind == ROSEN:
        f = 25.0 * left + 156.5 * right                # terms p - 1 (xi = 1, xn = 1.5) and p (xi = 1.5, xn = 1)
        g = {p: 751.0 * right + 100.0 * left}
        if left:
            g[p - 1] = -200.0
        if right:
            g[p + 1] = -250.0
    else:
        lam = PROBE_LAMBDA
        f = lam / 2 * 0.25 + 0.125 * left + 0.125 * right     # 0.03125 on the diagonal, 0.125 per pair
        g = {p: lam * 0.5 + 0.5 * left + 0.5 * right}
        if left:
            g[p - 1] = -0.5
        if right:
            g[p + 1] = -0.5
    return f, g


def chain_probe_gradient(kind, n, p, dtype):
    g = np.zeros(n, dtype=dtype)
    if kind == ROSEN and n > 1:
        g[0] = -0.0
    for i, v in chain_probe(kind, n, p)[1].items():
        g[i] = v
    return g


# ------------------------------------------------------------------------------ dense quadratic
def quad_value_gradient(cols, x):
    """cols[j, i] = element i of column j as the device holds it (A[i, j], column-major).  Returns (Value of 1/2 sum_j x_j c_j,
    g = c, the bounds of g's elements), c_j = sum_i cols[j, i] x[i].  No symmetry is assumed."""
    cols, x = np.asarray(cols), np.asarray(x)
    dtype, n = x.dtype, x.size
    xl = x.astype(LD)
    prod = cols.astype(LD) * xl[None, :]
    c, lv1 = tree_sum(prod)
    Sc, _ = tree_sum(np.abs(prod))
    f, lv2 = tree_sum(c * xl)
    S, _ = tree_sum(Sc * np.abs(xl))
    f, S = f / 2, S / 2
    m_col, m_fin = sum_depth(QUAD, dtype, n, 0)                # (no CU count in the dense quadratic's launch)
    E = S * ((1 + gamma(m_col, U64)) * (1 + U64) * (1 + gamma(m_fin, U64)) - 1)
    if dtype == F32:
        E = E + U32 * (abs(f) + E)
    gb = (n + 1) * U64 * Sc + U[dtype] * np.abs(c) + _ref_error(lv1, Sc)
    return Value(f, S, E + _ref_error(lv1 + lv2, S)), c, gb


def quad_probe(cols, p, q=None):
    """x = e_p (+ e_q): (f, g) as the device must return them, bit for bit: every column sum is one element or one rounded fp64
    addition of two, the value 1/2 (c_p + c_q) one more."""
    cols = np.asarray(cols)
    t = cols.dtype.type
    if q is None:
        return t(0.5) * cols[p, p], cols[:, p].copy()
    c = cols[:, p].astype(np.float64) + cols[:, q].astype(np.float64)
    return t(0.5 * (c[p] + c[q])), c.astype(cols.dtype)


# ------------------------------------------------------------------------------ log-sum-exp
def lse_parts(x, c, lam, cus, mx=None, drop=None):
    """The pieces of f = mx + log(se) + lambda/2 sq and the error of each.  ``mx``: a planted maximum; ``drop``: indices left
    out of se (the planted errors of the CPU test).  A planted maximum overflows as the device's would: exp above 709.78."""
    x, c = np.asarray(x), np.asarray(c)
    dtype, n = x.dtype, x.size
    uT, ulam = U[dtype], (U32 if dtype == F32 else LD(0))
    xl, cl = x.astype(LD), c.astype(LD)
    mx = xl.max() if mx is None else LD(mx)
    d = xl - mx
    with np.errstate(over="ignore", under="ignore"):
        e = np.where(d > LD(709.78), LD(np.inf), np.exp(d))
    keep = np.ones(n, dtype=bool)
    if drop is not None:
        keep[drop] = False
    grid, _ = launch(LSE, dtype, n, cus)
    gm = gamma(_cdiv(n, grid * BLOCK) + 6 + WAVES + _cdiv(grid, BLOCK) + 6 + WAVES, U64)
    r = np.exp(uT * np.abs(d)) * (1 + 2 * ULP_EXP * U64) - 1
    se, levels = tree_sum(e[keep])
    E_se = (1 + gm) * tree_sum((e * r + HALF_SUBNORMAL[F64])[keep])[0] + gm * se
    dl = xl - cl
    sq, _ = tree_sum(dl * dl)
    E_sq = sq * ((1 + uT) ** 2 * (1 + gm) - 1)
    P = collections.namedtuple("LseParts", "mx d e r se E_se sq E_sq gm levels dl uT ulam")
    return P(mx, d, e, r, se, E_se, sq, E_sq, gm, levels, dl, uT, ulam)


def lse_value(x, c, lam, cus, mx=None, drop=None):
    x = np.asarray(x)
    P = lse_parts(x, c, lam, cus, mx, drop)
    if not np.isfinite(P.se):
        return Value(LD(np.inf), LD(np.inf), LD(0))
    lg = np.log(P.se)
    lt = LD(lam) / 2 * P.sq
    f = P.mx + lg + lt
    E_log = -np.log1p(-P.E_se / P.se) + 2 * ULP_LOG * U64 * abs(lg)
    E_lt = (lt + LD(lam) / 2 * P.E_sq) * (1 + U64) * (1 + P.ulam) - lt
    S = abs(P.mx) + abs(lg) + lt
    E = E_log + E_lt + 2 * U64 * (S + E_log + E_lt)
    if x.dtype == F32:
        E = E + U32 * (abs(f) + E)
    return Value(f, S, E + _ref_error(P.levels, S + P.sq * LD(lam)))


def lse_gradient(x, c, lam, cus):
    """(g in longdouble, the bound of every element)"""
    x = np.asarray(x)
    P = lse_parts(x, c, lam, cus)
    sm = P.e / P.se
    lt = LD(lam) * P.dl
    g = sm + lt
    rho = (1 + P.r) * (1 + U64) / (1 - P.E_se / P.se) - 1
    E = sm * rho + HALF_SUBNORMAL[F64] / P.se + np.abs(lt) * ((1 + P.uT) * (1 + U64) * (1 + P.ulam) - 1)
    E = E + U64 * (sm + np.abs(lt) + E)
    E = E + P.uT * (np.abs(g) + E) + HALF_SUBNORMAL[x.dtype]
    return g, E + _ref_error(P.levels, sm + np.abs(lt))


def lse_probe(n, p, dtype):
    """x = c = -800 everywhere but x[p] = c[p] = 0: exp(-800) is exactly 0 in fp64, so se = 1, f = 0 and g = e_p, all zeros +0"""
    x = np.full(n, -800.0, dtype=dtype)
    x[p] = 0
    g = np.zeros(n, dtype=dtype)
    g[p] = 1
    return x, 0.0, g


# ------------------------------------------------------------------------------ L2 decorator
def l2_value(base, x, l2, cus):
    """Value of base + l2 sum x_i^2 as problem_eval_async forms it; ``base``: the Value of the undecorated objective, whose
    bound in fp32 already holds the rounding of the base value to float (which l2_finish_kernel performs)."""
    x = np.asarray(x)
    dtype, n = x.dtype, x.size
    xl = x.astype(LD)
    ss, levels = tree_sum(xl * xl)
    grid, _ = launch("decor", dtype, n, cus)
    gm = gamma(_cdiv(n, grid * BLOCK) + 6 + WAVES + _cdiv(grid, BLOCK) + 6 + WAVES, U64)
    uT = U[dtype]
    if dtype == F64:
        l2 = LD(l2)
        part = l2 * ss
        E_part = part * ((1 + gm) * (1 + U64) - 1)
    else:
        l2 = LD(np.float32(l2))
        part = l2 * ss
        E_part = part * ((1 + gm) * (1 + U32) ** 2 - 1)       # (float)ss, the float product ((float)lambda2 is the twin's l2)
    f = base.f + part
    S = base.S + abs(part)
    E = base.bound + E_part
    E = E + uT * (abs(base.f) + abs(part) + E)                 # the addition, in T
    return Value(f, S, E + _ref_error(levels, abs(part)))


# ------------------------------------------------------------------------------ dense points
_KIND_ID = {ROSEN: 1, QCHAIN: 2, QUAD: 3, LSE: 4}


@functools.lru_cache(maxsize=None)
def chain_point(kind, dtype, n):
    """x = u - 1/2, u uniform in [0, 1): (1 - x)^2 >= 1/4, so every term of either chain kind carries a floor and the planted
    errors of the CPU test are larger than the bounds at every size of SIZES in both element types"""
    x = (np.random.default_rng([_KIND_ID[kind], n]).random(n) - 0.5).astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def quad_buffer(dtype, n_max=2049):
    """n_max^2 entries u - 1/2; the matrix of size n is its first n^2 entries (one upload serves every size).  No symmetry:
    column j of it is not row j."""
    return (np.random.default_rng([_KIND_ID[QUAD], 0]).random(n_max * n_max) - 0.5).astype(dtype)


@functools.lru_cache(maxsize=None)
def quad_case(dtype, n):
    """(cols (n, n) with cols[j, i] = A[i, j], x): entries u - 1/2, x = u - 1/2 as the existing tests scale it"""
    dtype = np.dtype(dtype)
    cols = quad_buffer(dtype)[:n * n].reshape(n, n)
    x = (np.random.default_rng([_KIND_ID[QUAD], n]).random(n) - 0.5).astype(dtype)
    x.setflags(write=False)
    return cols, x


@functools.lru_cache(maxsize=None)
def quad_reference(dtype, n):
    return quad_value_gradient(*quad_case(dtype, n))


LSE_VARIANTS_ALL = ("random", "last_high")
LSE_VARIANTS_MORE = ("max_first", "max_last", "max_mid", "spread", "negative", "c_is_x", "lambda0")
LSE_MORE_SIZES = (257, 1025)


@functools.lru_cache(maxsize=None)
def lse_case(dtype, n, variant):
    """(x, c, lambda).  random: x = 3 (u - 1/2), c = u - 1/2, lambda = 1e-2 as the existing test; last_high: the same with 800
    added to the last element (a maximum that misses it overflows); the others as their names say."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([_KIND_ID[LSE], n])
    x = (rng.random(n) - 0.5) * 3
    c = rng.random(n) - 0.5
    lam = LSE_LAMBDA
    if variant == "last_high":
        x[-1] += 800
    elif variant == "max_first":
        x[0] = 2.0
    elif variant == "max_last":
        x[-1] = 2.0
    elif variant == "max_mid":
        x[n // 2] = 2.0
    elif variant == "spread":                          # maximum 0 and minimum -spread both present
        spread = 700.0 if dtype == F64 else 80.0
        x = -spread * rng.random(n)
        x[n // 3], x[(2 * n) // 3] = 0.0, -spread
    elif variant == "negative":
        x = x - 1000.0
    elif variant == "lambda0":
        lam = 0.0
    else:
        assert variant in ("random", "c_is_x")
    x = x.astype(dtype)
    c = x.copy() if variant == "c_is_x" else c.astype(dtype)
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c, lam


def lse_cases():
    """every (n, variant) of the dense log-sum-exp checks"""
    out = [(n, v) for n in SIZES[LSE] for v in LSE_VARIANTS_ALL]
    out += [(n, v) for n in LSE_MORE_SIZES for v in LSE_VARIANTS_MORE]
    return out


@functools.lru_cache(maxsize=None)
def lse_reference(dtype, n, variant, cus=256):
    x, c, lam = lse_case(dtype, n, variant)
    return lse_value(x, c, lam, cus), lse_gradient(x, c, lam, cus)


# ------------------------------------------------------------------------------ decorator cases
L2_LAMBDA = 0.05
BOX_CONFIGS = {
    # name: (l2, lo, hi).  "l2box": both decorators on a point clipped to the box; "hi1", "lo1", "pinch": no L2 term, so that
    # a gradient element can be a zero of either sign where the point sits on a bound (an L2 term 2 lambda x_i is not zero)
    "l2box": (L2_LAMBDA, 0.25, 0.75),
    "hi1": (0.0, 0.25, 1.0),
    "lo1": (0.0, 1.0, 1.5),
    "pinch": (0.0, 1.0, 1.0),
}
BOX_SITUATIONS = tuple((side, sign) for side in ("lo", "hi") for sign in ("positive", "negative", "+0", "-0"))


@functools.lru_cache(maxsize=None)
def box_point(dtype, n, config):
    """A point inside the box of a configuration with elements exactly on lo and on hi.  ROSEN's gradient at a run of ones is
    -0 at element 0 and +0 behind it, and +0 at a last element x[n-1] = x[n-2]^2: "hi1" starts 1, 1, 1, 1 (on hi) and ends
    0.5, 0.25 (on lo); "lo1" and "pinch" start with the run of ones on lo (and hi)."""
    dtype = np.dtype(dtype)
    _, lo, hi = BOX_CONFIGS[config]
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    x = mid + (np.random.default_rng([5, n]).random(n) - 0.5) * 3 * half    # a third of the elements beyond each bound
    x = np.clip(x, lo, hi).astype(dtype)
    if config != "l2box":
        x[:4] = 1.0
        if config == "hi1" and n >= 8:
            x[-2:] = (0.5, 0.25)
    x.setflags(write=False)
    return x


def box_situations(x, g, lo, hi):
    """which of BOX_SITUATIONS occur: g = the gradient before the box rule"""
    x, g = np.asarray(x), np.asarray(g)
    found = set()
    for side, on in (("lo", x == x.dtype.type(lo)), ("hi", x == x.dtype.type(hi))):
        for sign, m in (("positive", g > 0), ("negative", g < 0), ("+0", (g == 0) & ~np.signbit(g)), ("-0", (g == 0) & np.signbit(g))):
            if (on & m).any():
                found.add((side, sign))
    return found


def assert_box_situations_occur(dtype, gradient_before_box):
    """asserts that over DECORATOR_SIZES and BOX_CONFIGS every one of the eight BOX_SITUATIONS occurs at least once;
    ``gradient_before_box(n, l2, x)``: the chained Rosenbrock's gradient with its L2 term (the oracle's, in the tests)"""
    found = set()
    for n in DECORATOR_SIZES:
        for config, (l2, lo, hi) in BOX_CONFIGS.items():
            x = box_point(dtype, n, config)
            assert x.min() >= lo and x.max() <= hi, (n, config)
            found |= box_situations(x, gradient_before_box(n, l2, x), lo, hi)
    assert found == set(BOX_SITUATIONS), sorted(set(BOX_SITUATIONS) - found)


def box_rule(x, g, lo, hi):
    """UniformBoxGradientWrapper as grad_decorate_kernel applies it"""
    x, g = np.asarray(x), np.asarray(g)
    t = x.dtype.type
    out = g.copy()
    out[((x <= t(lo)) & (g >= 0)) | ((x >= t(hi)) & (g <= 0))] = 0
    return out


def clamp_case(dtype, n, lo, hi):
    """(x with a NaN, elements on and beyond both bounds and a -0; clamp(x, lo, hi) as box_clamp_kernel forms it)"""
    dtype = np.dtype(dtype)
    t = dtype.type
    x = ((np.random.default_rng([6, n]).random(n) - 0.5) * 4).astype(dtype)
    for i, v in enumerate((lo, hi, np.nan, -0.0, lo - 1, hi + 1)):
        x[(i * 37) % n] = v
    lo_t, hi_t = t(lo), t(hi)
    with np.errstate(invalid="ignore"):
        want = np.where(x < lo_t, lo_t, np.where(x > hi_t, hi_t, x)).astype(dtype)
    return x, want


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))
