"""CPU twin of the L1 vector primitives (csrc/dzo_vec.hip) and of the geometry their callers share (stream_loop, stream_grid,
block_sum, reduce_partials_all of csrc/dzo_common.h): every operation in numpy, in the precision and the ORDER the kernels use.
A helper module for tests/test_vec_twin.py (which checks it against things it does not depend on), tests/test_gpu_vec.py and
tests/test_gpu_flags.py (which check the device against it).  Not a conftest, no fixtures.

Geometry (restated from the kernels):

* a block has kBlock = 256 threads = 4 waves of 64; a 16-byte vector holds N = 2 fp64 / 4 fp32 elements;
* the grid is stream_grid(n, N * kUnroll): ceil(n / (256 * 4 * N)) blocks, at most min(8 * compute_units, 2048), at least 1;
* aligned operands (VEC): per trip, block b and thread t take the vectors  trip * grid * 1024 + b * 1024 + u * 256 + t,
  u = 0 .. 3; after the trips GLOBAL thread tid takes the one tail element  (n // N) * N + tid  if it is below n;
* operands off the 16-byte grid: global thread tid takes the elements tid, tid + grid * 256, ... (the same grid).
"""
import math

import numpy as np

import lowmode_twin as lt

K_BLOCK, K_WAVES, K_UNROLL, MAX_PARTIAL_BLOCKS = 256, 4, 4, 2048
K_ROW_OWN = 62                      # dzo_lbfgs_plan.h: vectors of a wave-row that the wave owns (the point pass and the pair pass)
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
U64 = 2.0 ** -53                    # unit roundoff of the fp64 accumulation


def vec_n(dtype):
    return 16 // np.dtype(dtype).itemsize


def grid_cap(compute_units):
    return min(8 * int(compute_units), MAX_PARTIAL_BLOCKS)


def grid(n, dtype, compute_units):
    """stream_grid(n, Vec16<T>::N * kUnroll)."""
    per_block = K_BLOCK * vec_n(dtype) * K_UNROLL
    return int(max(1, min((int(n) + per_block - 1) // per_block, grid_cap(compute_units))))


def second_trip_size(dtype, compute_units):
    """The smallest tested size whose grid-stride loop makes a second trip: a full grid, one more block, one more vector and
    a one-element tail."""
    N = vec_n(dtype)
    return grid_cap(compute_units) * 1024 * N + 1024 * N + N + 1


# ------------------------------------------------------------------------------ who reads which element, in which order
def partition(n, dtype, compute_units, aligned=True):
    """The sequential steps of stream_loop, for all threads at once: yields (idx, mask), int64 / bool arrays of grid * 256
    entries (thread tid = block * 256 + thread); at this step thread tid consumes element idx[tid] where mask[tid]."""
    n = int(n)
    N = vec_n(dtype)
    g = grid(max(n, 1), dtype, compute_units)
    nthreads = g * K_BLOCK
    tid = np.arange(nthreads, dtype=np.int64)
    if not aligned:
        for i0 in range(0, n, nthreads):
            idx = tid + i0
            yield idx, idx < n
        return
    b, t = tid // K_BLOCK, tid % K_BLOCK
    nvec = n // N
    base = b * (K_BLOCK * K_UNROLL)
    while base[0] < nvec:                       # (the loop bound is per block; a block past the end yields empty masks)
        for u in range(K_UNROLL):
            v = base + u * K_BLOCK + t
            for j in range(N):
                yield v * N + j, v < nvec
        base = base + nthreads * K_UNROLL
    tail = nvec * N + tid
    yield tail, tail < n


def chain_length(n, dtype, compute_units, aligned=True):
    """Longest per-thread chain of partition()."""
    return sum(1 for _ in partition(n, dtype, compute_units, aligned))


# ------------------------------------------------------------------------------ the two-stage sum
def _wave_sum_all(v):
    """wave_sum_all on an array [..., 64]: xor 32, 16, 8, 4, 2, 1 (a + b == b + a bit for bit, so every lane holds the same value)."""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    return v


def _block_sum(acc):
    """block_sum on [blocks, 256]: the wave butterfly, then the four wave sums added from +0 in wave order."""
    w = _wave_sum_all(acc.reshape(-1, K_WAVES, 64))[..., 0]
    r = np.zeros(w.shape[0])
    for k in range(K_WAVES):
        r = r + w[:, k]
    return r


def reduce_partials(partials):
    """reduce_partials_all: thread t adds t, t + 256, ... from +0, then the butterfly, then the four wave sums."""
    partials = np.asarray(partials, dtype=np.float64)
    v = np.zeros(K_BLOCK)
    for i0 in range(0, partials.size, K_BLOCK):
        chunk = partials[i0:i0 + K_BLOCK]
        v[:chunk.size] = v[:chunk.size] + chunk
    return float(_block_sum(v.reshape(1, K_BLOCK))[0])


def dot(x, y, compute_units, aligned=True):
    """dzo_dot's fp64 result, bit for bit (finite inputs in the normal range)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape and x.ndim == 1
    dtype, n = x.dtype, x.size
    g = grid(max(n, 1), dtype, compute_units)
    acc = np.zeros(g * K_BLOCK)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        for idx, mask in partition(n, dtype, compute_units, aligned):
            if not mask.any():
                continue
            i = np.where(mask, idx, 0)
            if dtype == F64:
                new = lt.fma64(xd[i], yd[i], acc)
            else:
                # two 24-bit significands: the product is exact in fp64, so acc + x * y rounds once and has the fma's bits
                new = acc + xd[i] * yd[i]
            acc = np.where(mask, new, acc)
        return reduce_partials(_block_sum(acc.reshape(g, K_BLOCK)))


def norm2(x, compute_units, aligned=True):
    """dzo_norm2: the sum of squares, rounded to T."""
    ss = dot(x, x, compute_units, aligned)
    return float(np.float32(ss)) if x.dtype == F32 else ss


def norm(x, compute_units, aligned=True):
    """dzo_nrm2: sqrt of the fp64 sum; fp32: rounded to float first, then sqrtf."""
    ss = dot(x, x, compute_units, aligned)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float32(ss))) if x.dtype == F32 else float(np.sqrt(np.float64(ss)))


def inv_norm(x, compute_units, aligned=True):
    """dzo_inv_norm: 1 / sqrt(ss) in T."""
    ss = dot(x, x, compute_units, aligned)
    with np.errstate(all="ignore"):
        if x.dtype == F32:
            return float(np.float32(1.0) / np.sqrt(np.float32(ss)))
        return float(np.float64(1.0) / np.sqrt(np.float64(ss)))


def exact_dot(x, y):
    """(sum x_i y_i correctly rounded, sum |x_i y_i|) from the exact products (error-free product, math.fsum)."""
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if np.asarray(x).dtype == F64:
        p, e = lt._two_prod(xd, yd)
        terms = np.concatenate([p, e])
    else:
        terms = xd * yd                          # exact
    return math.fsum(terms.tolist()), math.fsum(np.abs(xd * yd).tolist())


def dot_bound(n, dtype, compute_units, aligned, scale):
    """gamma_k * sum |x_i y_i| (test_vec_twin.test_twin_dot_against_the_exact_sum has the derivation)."""
    g = grid(max(n, 1), dtype, compute_units)
    k = chain_length(n, dtype, compute_units, aligned) + 6 + 4 + (g + K_BLOCK - 1) // K_BLOCK + 6 + 4
    return k * U64 / (1.0 - k * U64) * scale, k


# ------------------------------------------------------------------------------ elementwise references
def _fma(a, b, c, dtype):
    """dfma in T on arrays.  Outside the emulation's range -- an operand that is not finite, or a zero product -- the product
    is exact, so a * b + c rounds once (in fp64 for fp32 operands, then once more to fp32 from an exact or special value)."""
    dtype = np.dtype(dtype)
    a, b, c = (np.atleast_1d(np.asarray(v, dtype=dtype)) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):
        r = lt.fma64(a, b, c) if dtype == F64 else lt.fma32(a, b, c)
        wide = a.astype(np.float64) * b.astype(np.float64) if dtype == F32 else a * b
        special = ~np.isfinite(a) | ~np.isfinite(b) | ~np.isfinite(c) | (wide == 0)
        if dtype == F64:
            # products near the subnormal range: the error-free product loses its low part there, so the caller keeps them
            # exact (the special-value tests scale by a power of two)
            special |= np.abs(wide) < 1e-250
        plain = (wide + c).astype(dtype)
    return np.where(special, plain, r).astype(dtype)


def axpy(alpha, x, y):
    """y <- fma((T)alpha, x, y)."""
    return _fma(x.dtype.type(alpha), x, y, x.dtype)


def trial_point(t, d, x):
    """dst <- fma((T)t, d, x)."""
    return _fma(x.dtype.type(t), d, x, x.dtype)


def axpby(alpha, x, beta, y):
    """y <- fma((T)alpha, x, (T)beta * y): beta * y is rounded first."""
    T = x.dtype.type
    with np.errstate(all="ignore"):
        by = (T(beta) * y).astype(x.dtype)
    return _fma(T(alpha), x, by, x.dtype)


def scal(alpha, x):
    """x <- (T)alpha * x (rmul!, and scale! in and out of place)."""
    with np.errstate(all="ignore"):
        return (x.dtype.type(alpha) * x).astype(x.dtype)


scale = scal


def fill(n, value, dtype):
    with np.errstate(all="ignore"):
        return np.full(int(n), np.dtype(dtype).type(value), dtype=dtype)


def negate(x):
    """(T)-1 * x: the sign flips, zeros and infinities included; a NaN stays a NaN."""
    return scal(-1.0, x)


def copy(x):
    return np.array(x, copy=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def other_nan(dtype):
    """A NaN of the other sign and another payload than numpy's default quiet NaN."""
    dt = np.dtype(dtype)
    u = np.array([np.nan], dtype=dt).view({8: np.uint64, 4: np.uint32}[dt.itemsize])
    u ^= u.dtype.type((1 << (dt.itemsize * 8 - 1)) | 5)
    return u.view(dt)[0]


def isequal(a, b):
    """Base.isequal on arrays: bitwise equal, or both NaN."""
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def same(a, b):
    """Elementwise results agree: the same bits, a NaN matching any NaN (payloads are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and isequal(a, b)


# ------------------------------------------------------------------------------ where a flag or a store can go wrong
def positions(n, dtype, compute_units=256):
    """Element indices below n at the seams of stream_loop's geometry, ascending, without duplicates."""
    n = int(n)
    N = vec_n(dtype)
    nvec = n // N
    want = [0, N - 1, N,                        # first element, end of the first vector, the second lane's vector
            64 * N, 3 * 64 * N,                 # first lane of wave 1, wave 3
            256 * N,                            # u = 1
            1024 * N - 1, 1024 * N]             # last element of block 0, first of block 1
    if nvec >= 1:
        want += [(nvec - 1) * N, nvec * N - 1]  # the last full vector
    want += list(range(nvec * N, n))            # the scalar tail
    want.append(grid(n, dtype, compute_units) * 1024 * N)     # first element of the second trip (below n only past the cap)
    want.append(n - 1)
    return sorted({p for p in want if 0 <= p < n})


def sizes(dtype, compute_units=256, second_trip=True):
    """The sizes tests/test_gpu_vec.py runs."""
    N = vec_n(dtype)
    s = [1, 2, 3, N - 1, N + 1, 64 * N - 1, 64 * N + 1, 256 * N - 1, 256 * N + 1,
         1024 * N - 1, 1024 * N, 1024 * N + 1, 1024 * N + N + 1, 2 * 1024 * N + 1]
    if second_trip:
        s.append(second_trip_size(dtype, compute_units))
    return sorted({v for v in s if v >= 1})


def offsets(dtype):
    """Element offsets of an operand's view from its 16-byte aligned base."""
    return list(range(vec_n(dtype)))


def alignments(dtype, operands, full=True):
    """Offset tuples, one offset per operand: all aligned, all off by the same offset, each operand off alone by every offset,
    and (fp32) all off by different offsets.  full=False: all aligned and one mixed combination (the second-trip size)."""
    offs = offsets(dtype)[1:]
    zero = (0,) * operands
    if not full:
        return [zero, tuple(offs[i % len(offs)] if i != 1 else 0 for i in range(operands))]
    out = [zero] + [(o,) * operands for o in offs]
    if operands > 1:
        out += [tuple(o if i == k else 0 for i in range(operands)) for k in range(operands) for o in offs]
        if len(offs) > 1:
            out.append(tuple(offs[i % len(offs)] for i in range(operands)))
    return out


# ------------------------------------------------------------------------------ the flag tests' cases (tests/test_gpu_flags.py)
FLAG_LARGE = 100_003


def flag_sizes(dtype):
    """Sizes of the optimizer paths: those of sizes() up to two blocks and a tail, and n = 100 003 (several blocks, ragged in
    both dtypes)."""
    return sizes(dtype, second_trip=False) + [FLAG_LARGE]


def whole_vector_sizes(dtype):
    """Sizes for the passes that take whole 16-byte vectors only (the pair ring's single-pass step, the fused AdGD pass; both
    from 4 N elements on): the smallest, one wave-row of 62 vectors and one vector more, one block of four rows and one vector
    more, the streaming kernels' block and two blocks and a vector, and a large one."""
    N = vec_n(dtype)
    return [4 * N, K_ROW_OWN * N, (K_ROW_OWN + 1) * N, 4 * K_ROW_OWN * N, (4 * K_ROW_OWN + 1) * N, 1024 * N, (2 * 1024 + 1) * N, FLAG_LARGE + 1]


def row_positions(n, dtype):
    """positions() and the seams of the fused passes' wave-rows: a wave owns kRowOwn = 62 consecutive vectors of a row, a
    block four rows, so 62 N - 1 / 62 N are the last element of row 0 and the first of row 1 (another wave), 4 * 62 N the
    first row of the second block; the ragged last vector is in positions() already."""
    N = vec_n(dtype)
    extra = [K_ROW_OWN * N - 1, K_ROW_OWN * N, 4 * K_ROW_OWN * N - 1, 4 * K_ROW_OWN * N]
    return sorted(set(positions(n, dtype)) | {p for p in extra if p < n})


def window(n, p, width=1):
    return [i for i in range(p - width, p + width + 1) if 0 <= i < n]


def window_start(n, p, dtype):
    """Window probe: chained Rosenbrock at its minimiser x = 1 with x[p] moved by 1e-3."""
    x = np.ones(n, dtype=dtype)
    x[p] += np.dtype(dtype).type(1e-3)
    return x


def one_hot_start(n, p, dtype):
    """One-hot probe: log-sum-exp with c = 0 at x = -800, x[p] = 0: every other weight exp(-800) underflows to zero."""
    x = np.full(n, -800.0, dtype=dtype)
    x[p] = 0.0
    return x
