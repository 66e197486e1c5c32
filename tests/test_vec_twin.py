"""tests/vec_twin.py against things it does not depend on (no GPU):

1. the twin's dot against the correctly rounded sum of the exact products, within a derived bound;
2. the partition of [0, n) among the threads: every index consumed exactly once, at every tested size, aligned and not;
3. the elementwise references on special values;
4. positions(): the table of seams, derived from the geometry;
5. the probes tests/test_gpu_flags.py starts from do on the CPU oracle what that module's docstring says, for every (n, p).
"""
import math

import numpy as np
import pytest

import vec_twin as vt
from oracle import oracle as orc

DTYPES = ["float64", "float32"]
CUS = 256                                                      # the MI355X; a small device (CUS_SMALL) makes further trips at small n
CUS_SMALL = 1


def _data(n, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)


# ------------------------------------------------------------------------------ 1. the sum
def _dot_cases():
    out = []
    for d in DTYPES:
        for n in vt.sizes(d, second_trip=False):
            out.append((d, n, CUS))
        N = vt.vec_n(d)
        out.append((d, vt.second_trip_size(d, CUS_SMALL), CUS_SMALL))          # two trips of an 8-block grid
        out.append((d, 3 * 8 * 1024 * N + 5 * N + 1, CUS_SMALL))               # four trips, the last one partial
        out.append((d, 300 * 1024 * N + 3, 64))                                # 300 partials: two strided rounds of the finish
    return out


@pytest.mark.parametrize("dtype,n,cus", _dot_cases())
@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "scalar"])
def test_twin_dot_against_the_exact_sum(dtype, n, cus, aligned):
    """Bound.  Every product x_i y_i enters the result through a chain of rounded fp64 operations, each of relative error at
    most u = 2^-53: the fused multiply-adds of its thread's chain from its own position on (at most L = the chain length: the
    product itself is exact inside the fma, in fp32 because 24 + 24 bits fit), 6 additions of the wave butterfly, at most 4 of
    the four wave sums, at most ceil(grid / 256) of the finishing thread's strided sum over the block partials, 6 of the
    second butterfly and 4 of its wave sums.  With k = L + 6 + 4 + ceil(grid / 256) + 6 + 4 the computed sum is
    sum x_i y_i (1 + theta_i), |theta_i| <= gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1), hence
    |computed - exact| <= gamma_k sum |x_i y_i|.  The reference is math.fsum over the error-free products (correctly rounded:
    another u |exact|, covered by comparing with one more u sum |x_i y_i|)."""
    x, y = _data(n, dtype, 7 * n + cus)
    got = vt.dot(x, y, cus, aligned)
    exact, scale = vt.exact_dot(x, y)
    bound, k = vt.dot_bound(n, dtype, cus, aligned, scale)
    print(dtype, n, cus, aligned, "k", k, "err", abs(got - exact), "bound", bound)
    assert abs(got - exact) <= bound + vt.U64 * scale
    # the chain is what the header says: at most 2 * 4 * N + 1 steps on the MI355X at every tested size
    if cus == CUS and aligned:
        assert vt.chain_length(n, dtype, cus) <= 2 * 4 * vt.vec_n(dtype) + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_twin_reductions_on_small_exact_cases(dtype):
    cus = CUS
    assert vt.dot(np.zeros(0, dtype), np.zeros(0, dtype), cus) == 0.0 and not math.copysign(1.0, vt.dot(np.zeros(0, dtype), np.zeros(0, dtype), cus)) < 0
    assert vt.inv_norm(np.zeros(0, dtype), cus) == math.inf and vt.norm(np.zeros(0, dtype), cus) == 0.0
    x = np.arange(1, 2050, dtype=dtype)                        # integers: every partial sum is exact, any order gives the same
    want = float(sum(i * i for i in range(1, 2050)))
    for aligned in (True, False):
        assert vt.dot(x, x, cus, aligned) == want
        assert vt.norm2(x, cus, aligned) == float(np.dtype(dtype).type(want))
    three = np.array([3.0, 4.0], dtype=dtype)
    assert vt.norm(three, cus) == 5.0 and vt.inv_norm(three, cus) == float(np.dtype(dtype).type(1.0) / np.dtype(dtype).type(5.0))
    # the order is the device's: lanes 0 and 1 hold (1e16, 1) and (-1e16, 1); each chain loses its 1 before the butterfly
    big = np.array([1e16, 1.0, -1e16, 1.0])
    # (off the 16-byte grid every lane holds one element, and the butterfly adds lanes 0 and 2 first: nothing is lost)
    assert vt.dot(big, np.ones(4), cus) == 0.0 and vt.dot(big, np.ones(4), cus, aligned=False) == 2.0
    assert vt.dot(np.array([1e16, -1e16, 1.0, 1.0]), np.ones(4), cus) == 2.0


# ------------------------------------------------------------------------------ 2. coverage
def _coverage_cases():
    out = []
    for d in DTYPES:
        out += [(d, n, CUS) for n in vt.sizes(d, CUS)] + [(d, vt.FLAG_LARGE, CUS)]
        out += [(d, n, CUS_SMALL) for n in (vt.second_trip_size(d, CUS_SMALL), 3 * 8 * 1024 * vt.vec_n(d) + 5 * vt.vec_n(d) + 1)]
    return out


@pytest.mark.parametrize("dtype,n,cus", _coverage_cases())
@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "scalar"])
def test_every_index_is_consumed_exactly_once(dtype, n, cus, aligned):
    count = np.zeros(n, dtype=np.int64)
    g = vt.grid(n, dtype, cus)
    steps = 0
    for idx, mask in vt.partition(n, dtype, cus, aligned):
        assert idx.shape == mask.shape == (g * vt.K_BLOCK,)
        taken = idx[mask]
        assert taken.size == 0 or (taken.min() >= 0 and taken.max() < n)
        count += np.bincount(taken, minlength=n)
        steps += 1
    assert np.all(count == 1), np.flatnonzero(count != 1)[:5]
    N = vt.vec_n(dtype)
    if aligned:
        trips = -(-(n // N) // (g * 1024))
        assert steps == trips * 4 * N + 1
        if cus == CUS:
            assert trips == (2 if n == vt.second_trip_size(dtype, CUS) else 1 if n >= N else 0)
    else:
        assert steps == -(-n // (g * vt.K_BLOCK))


def test_grid_restates_stream_grid():
    for d, N in (("float64", 2), ("float32", 4)):
        assert vt.vec_n(d) == N
        assert vt.grid(0, d, CUS) == 1 and vt.grid(1, d, CUS) == 1 and vt.grid(1024 * N, d, CUS) == 1 and vt.grid(1024 * N + 1, d, CUS) == 2
        assert vt.grid(2048 * 1024 * N, d, CUS) == 2048 and vt.grid(10 ** 9, d, CUS) == 2048 and vt.grid(10 ** 9, d, 304) == 2048
        assert vt.grid(10 ** 9, d, 64) == 512 and vt.grid(10 ** 9, d, 1) == 8
    assert vt.second_trip_size("float64", CUS) == 4_194_304 + 2048 + 3 and vt.second_trip_size("float32", CUS) == 8_388_608 + 4096 + 5


# ------------------------------------------------------------------------------ 3. elementwise
@pytest.mark.parametrize("dtype", DTYPES)
def test_elementwise_references(dtype):
    dt = np.dtype(dtype)
    T = dt.type
    tiny = np.finfo(dt).smallest_subnormal
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 1.5], dtype=dt)
    ones = np.ones_like(sp)
    neg = vt.negate(sp)
    assert np.isnan(neg[0]) and np.array_equal(np.signbit(neg[1:]), ~np.signbit(sp[1:])) and np.array_equal(np.abs(neg[1:]), np.abs(sp[1:]))
    assert vt.same(vt.axpy(2.0, sp, ones), (T(2) * sp + ones).astype(dt))                    # the product by a power of two is exact
    assert vt.same(vt.axpy(1.0, np.array([-0.0], dt), np.array([-0.0], dt)), np.array([-0.0], dt))      # fma(1, -0, -0) = -0
    assert np.signbit(vt.axpy(1.0, np.array([-0.0], dt), np.array([-0.0], dt))[0])
    assert np.all(np.isnan(vt.axpby(1.0, ones, 0.0, np.full_like(sp, np.nan))))                # 0 * NaN is formed
    assert vt.same(vt.axpby(1.0, ones, 0.0, ones), ones)
    assert vt.fill(3, 0.1, dt)[0] == T(0.1) and vt.fill(3, 1e300, np.float32)[0] == np.inf and vt.fill(3, 1e-300, np.float32)[0] == 0
    # one rounding, not two: a * x + y where the product's low bits decide
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(4096).astype(dt), rng.standard_normal(4096).astype(dt)
    a = T(0.37)
    exact = x.astype(np.longdouble) * np.longdouble(a) + y.astype(np.longdouble)       # (fp32: exact in the 64-bit significand)
    got = vt.axpy(float(a), x, y)
    assert np.all(np.abs(got.astype(np.longdouble) - exact) <= np.spacing(np.abs(got)).astype(np.longdouble) / 2 * (1 + 2.0 ** -9))
    assert np.any(got != (a * x + y).astype(dt))                # and it differs from the twice-rounded form somewhere
    assert vt.isequal(sp, sp.copy()) and not vt.isequal(np.array([0.0], dt), np.array([-0.0], dt))
    other_nan = sp.copy(); other_nan[0] = vt.other_nan(dt)
    assert np.isnan(other_nan[0]) and np.signbit(other_nan[0]) != np.signbit(sp[0]) and vt.bits(other_nan)[0] != vt.bits(sp)[0] and vt.isequal(sp, other_nan)
    assert orc.isequal(sp, other_nan) and not orc.isequal(np.array([0.0], dt), np.array([-0.0], dt))


# ------------------------------------------------------------------------------ 4. positions
def test_positions_are_the_seams_of_the_geometry():
    for d, N in (("float64", 2), ("float32", 4)):
        assert vt.positions(1, d) == [0] and vt.positions(N - 1, d)[-1] == N - 2
        n = 2 * 1024 * N + 1
        assert vt.positions(n, d) == [0, N - 1, N, 64 * N, 192 * N, 256 * N, 1024 * N - 1, 1024 * N, 2048 * N - N, 2048 * N - 1, 2048 * N]
        n = 1024 * N + N + 1                                    # a full vector in block 1 and a one-element tail
        assert vt.positions(n, d)[-4:] == [1024 * N - 1, 1024 * N, 1024 * N + N - 1, 1024 * N + N]
        assert set(range((n // N) * N, n)) <= set(vt.positions(n, d)) and n - 1 in vt.positions(n, d)
        n = 1024 * N - 1                                        # N - 1 tail elements, each on its own
        assert set(range(1024 * N - N, n)) <= set(vt.positions(n, d))
        big = vt.second_trip_size(d, CUS)
        assert 2048 * 1024 * N in vt.positions(big, d) and big - 1 in vt.positions(big, d)
        assert 2048 * 1024 * N not in vt.positions(big, d, 64) and 512 * 1024 * N in vt.positions(big, d, 64)
        for n in vt.sizes(d):
            p = vt.positions(n, d)
            assert p == sorted(set(p)) and p[0] == 0 and p[-1] == n - 1 and all(0 <= q < n for q in p)
        # who consumes a position: the partition agrees with the table's reasons
        owner = {}
        for step, (idx, mask) in enumerate(vt.partition(2 * 1024 * N + 1, d, CUS)):
            for tid in np.flatnonzero(mask & np.isin(idx, [64 * N, 192 * N, 256 * N, 1024 * N, 2048 * N])):
                owner[int(idx[tid])] = (step, int(tid))
        assert owner[64 * N] == (0, 64) and owner[192 * N] == (0, 192) and owner[256 * N] == (N, 0)
        assert owner[1024 * N] == (0, 256) and owner[2048 * N] == (4 * N, 0)


# ------------------------------------------------------------------------------ 5. the probes of the flag tests
def _probe_cases():
    return [(d, n) for d in DTYPES for n in sorted(set(vt.flag_sizes(d) + vt.whole_vector_sizes(d)))]


def _moved(after, before):
    return np.flatnonzero(vt.bits(after) != vt.bits(before)).tolist()


@pytest.mark.parametrize("dtype,n", _probe_cases())
def test_probe_preconditions_hold_on_the_oracle(dtype, n):
    """What tests/test_gpu_flags.py says about its probes, on the CPU oracle, for every (n, p) it uses.

    Window probe: the gradient of the chained Rosenbrock function (and of the chained quadratic) at x = 1, x[p] += 1e-3 is
    non-zero exactly on {p - 1, p, p + 1}; the first L-BFGS step (step length 1) is not stuck, needs several halvings on
    Rosenbrock (so the later-trial kernels run) and moves exactly those elements; each of the next two steps moves elements
    of a window one element wider on each side (a move below half an ulp leaves an element where it was), and is not stuck.
    The same holds for three AdGD steps.  One-hot probe: the gradient of log-sum-exp (c = 0,
    lambda = 0) at x = -800, x[p] = 0 is exactly e_p, and the step moves element p alone.  Stuck probe: at x = 1 the gradient
    is zero and the optimizer is stuck from its construction."""
    dt = np.dtype(dtype)
    if dt == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        chains = [orc.Problem(orc.ROSENBROCK_CHAIN, n, dt), orc.Problem(orc.QUADRATIC_CHAIN, n, dt, lam=0.05)] if n >= 2 else []
        ones = np.ones(n, dt)
        for prob in chains:
            assert not prob.grad(ones).any()
            ref = orc.LBFGS(prob, ones.copy(), 1.0, 3)
            assert ref.is_stuck
            ref.step()
            assert ref.is_stuck and np.array_equal(ref.current_point, ones) and ref.iteration_count == 0
        if n >= 2:
            ref = orc.AdGD(chains[0], ones.copy(), 0.1)
            ref.step()
            assert ref.is_stuck and np.array_equal(ref.current_point, ones)
        lse = orc.Problem(orc.LSE, n, dt, c=np.zeros(n, dt), lam=0.0)
        for p in vt.row_positions(n, dt):
            x0 = vt.window_start(n, p, dt)
            for prob in chains:
                g = prob.grad(x0)
                assert np.flatnonzero(g).tolist() == vt.window(n, p), (p, np.flatnonzero(g))
                ref = orc.LBFGS(prob, x0.copy(), 1.0, 3)
                for it in range(3):
                    x = np.array(ref.current_point)
                    ref.step()
                    assert not ref.is_stuck and 1 <= ref.last_trials <= 20, (p, it, ref.last_trials)
                    moved = _moved(ref.current_point, x)
                    assert moved == vt.window(n, p) if it == 0 else (moved and set(moved) <= set(vt.window(n, p, it + 1))), (p, it, moved)
                    if it == 0 and prob is chains[0]:
                        assert ref.last_trials >= 2, (p, ref.last_trials)
            if n >= 2:
                ref = orc.AdGD(chains[0], x0.copy(), 0.1)
                for it in range(3):
                    x = np.array(ref.current_point)
                    ref.step()
                    moved = _moved(ref.current_point, x)
                    assert not ref.is_stuck, (p, it)
                    assert moved == vt.window(n, p) if it == 0 else (moved and set(moved) <= set(vt.window(n, p, it + 1))), (p, it, moved)
            x0 = vt.one_hot_start(n, p, dt)
            e_p = np.zeros(n, dt); e_p[p] = 1.0
            assert np.array_equal(lse.grad(x0), e_p), p
            ref = orc.LBFGS(lse, x0.copy(), 1.0, 3)
            ref.step()
            assert not ref.is_stuck and _moved(ref.current_point, x0) == [p], p
            assert np.array_equal(lse.grad(np.array(ref.current_point)), e_p), p
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cls", ["BFGS", "GradientDescent"])
def test_dense_probe_preconditions_hold_on_the_oracle(cls, dtype):
    """The dense searches (n <= 1025): the one-hot probe moves p alone in one step and does not terminate; the window probe
    moves exactly the window in its first step (along the gradient) and runs three steps without terminating; at x = 1 the
    optimizer terminates and keeps its point."""
    dt = np.dtype(dtype)
    make = getattr(orc, cls)
    for n in [n for n in vt.flag_sizes(dt) if n <= 1025]:
        lse = orc.Problem(orc.LSE, n, dt, c=np.zeros(n, dt), lam=0.0)
        rosen = orc.Problem(orc.ROSENBROCK_CHAIN, n, dt)
        for p in vt.positions(n, dt):
            x0 = vt.one_hot_start(n, p, dt)
            ref = make(lse, x0.copy(), 1.0)
            ref.set_max_increases(8)                           # (f is unbounded below along -e_p: see tests/test_gpu_flags.py)
            ref.step()
            assert not ref.has_terminated and ref.iteration_count == 1 and _moved(ref.current_point, x0) == [p], (n, p)
            if n >= 2:
                x0 = vt.window_start(n, p, dt)
                ref = make(rosen, x0.copy(), 1.0)
                for it in range(3):
                    ref.step()
                    assert not ref.has_terminated and ref.iteration_count == it + 1, (n, p, it)
                    assert it > 0 or _moved(ref.current_point, x0) == vt.window(n, p), (n, p)
        if n >= 2:
            ones = np.ones(n, dt)
            ref = make(rosen, ones.copy(), 1.0)
            ref.step()
            assert ref.has_terminated and np.array_equal(ref.current_point, ones), n
