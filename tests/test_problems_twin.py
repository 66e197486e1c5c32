"""tests/problems_twin.py against things it does not depend on, without a GPU: the oracle as a second implementation (values
within the twin's bounds, gradients bit for bit or within bound), the probes' exact values, the case lists, and -- what the
bounds are for -- planted errors of the kinds a reduction kernel makes, each of which must fall outside the bound."""
import numpy as np
import pytest

import problems_twin as tw
from oracle import oracle as orc

DTYPES = [np.float64, np.float32]
ORC_KIND = {tw.ROSEN: orc.ROSENBROCK_CHAIN, tw.QCHAIN: orc.QUADRATIC_CHAIN, tw.QUAD: orc.QUADRATIC, tw.LSE: orc.LSE}
CUS = 256                      # the case lists and depths below are those of a 256-CU device; another count where stated


def _within(got, value):
    return abs(tw.LD(got) - value.f) <= value.bound


# ------------------------------------------------------------------------------ case lists
@pytest.mark.parametrize("cus", [256, 304, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_positions_hold_both_sides_of_every_seam(dtype, cus):
    dt = np.dtype(dtype)
    N = tw.VEC[dt]
    cap = min(8 * cus, 2048)
    for kind in (tw.ROSEN, tw.QCHAIN, tw.LSE):
        per_thread = 2 * N if kind == tw.ROSEN else 4
        n = tw.capped_size(kind, dtype, cus)
        assert n == cap * 256 * per_thread + (3 if dt == tw.F64 else 5)
        e = N if kind == tw.ROSEN else 1
        assert tw.launch(kind, dtype, n, cus) == (cap, e) and tw.launch(kind, dtype, n - 8, cus) == (cap, e)
        trip = cap * 256 * e                                   # elements of one grid-stride trip
        assert n > trip * (2 if kind == tw.ROSEN else 4)       # the capped size starts one trip more than the grid was sized for
        pos = set(tw.probe_positions(kind, dtype, n, cus))
        want = {0, n - 1, n - 2, N - 1, N, 64 * e - 1, 64 * e, 256 * e - 1, 256 * e, trip - 1, trip}
        last_seam = (n - 1) // trip * trip
        want |= {last_seam - 1, last_seam, n // N * N - 1, n // N * N}      # the last trip's seam, the first of the ragged tail
        assert n % N != 0 and want <= pos, (kind, sorted(want - pos))
    for kind in tw.KINDS:                                      # small sizes: nothing out of range, ends always there
        for n in tw.SIZES[kind]:
            pos = tw.probe_positions(kind, dtype, n, cus)
            assert pos == sorted(set(pos)) and pos[0] == 0 and pos[-1] == n - 1 and all(0 <= p < n for p in pos)
            if n % N and n > N and kind != tw.QUAD:
                assert n // N * N in pos
    pos = set(tw.probe_positions(tw.QUAD, dtype, 2049, cus))
    assert {N - 1, N, 63, 64, 64 * N - 1, 64 * N, 255, 256, 256 * N - 1, 256 * N, 1791, 1792, 2047, 2048} <= pos
    for p, q in tw.probe_pairs(dtype, 2049):
        assert p // N != q // N
    assert any(p // (256 * N) != q // (256 * N) for p, q in tw.probe_pairs(dtype, 2049))


def test_term_blocks_and_depths_follow_the_kernels():
    # ROSEN fp64, n = 1025: two blocks, vectors 0..255 to block 0, 256..511 to block 1, the tail element's term (none: 1024 is last)
    own = tw.term_block(tw.ROSEN, np.float64, 1025, CUS)
    assert tw.launch(tw.ROSEN, np.float64, 1025, CUS) == (2, 2)
    assert own[0] == 0 and own[511] == 0 and own[512] == 1 and own[1023] == 1 and own[1024] == 0
    # QCHAIN n = 1025: grid 2, element i in block (i % 512) // 256
    own = tw.term_block(tw.QCHAIN, np.float32, 1025, CUS)
    assert list(own[[0, 255, 256, 511, 512, 1024]]) == [0, 0, 1, 1, 0, 0]
    assert tw.sum_depth(tw.QCHAIN, np.float32, 1025, CUS) == 3 + 10 + 1 + 10
    assert tw.sum_depth(tw.ROSEN, np.float64, 1023, CUS) == 2 * 2 + 1 + 10 + 1 + 10
    assert tw.sum_depth(tw.QUAD, np.float32, 2049, CUS) == (3 * 4 + 10, 9 + 10)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_eight_box_situations_occur(dtype):
    tw.assert_box_situations_occur(dtype, lambda n, l2, x: orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype, l2=l2).grad(x))
    found = set()
    for n in tw.DECORATOR_SIZES:
        for config, (l2, lo, hi) in tw.BOX_CONFIGS.items():
            x = tw.box_point(dtype, n, config)
            assert x.min() >= lo and x.max() <= hi
            g = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype, l2=l2).grad(x)       # before the box rule
            here = tw.box_situations(x, g, lo, hi)
            found |= here
            if config == "l2box" and n >= 255:
                assert {("lo", "positive"), ("lo", "negative"), ("hi", "positive"), ("hi", "negative")} <= here
            boxed = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype, l2=l2, box_gradient=(lo, hi)).grad(x)
            assert tw.same_bits(boxed, tw.box_rule(x, g, lo, hi))
    assert found == set(tw.BOX_SITUATIONS)


# ------------------------------------------------------------------------------ probes
def _chain_problem(kind, n, dtype, lam):
    return orc.Problem(ORC_KIND[kind], n, dtype, lam=lam)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [tw.ROSEN, tw.QCHAIN])
def test_oracle_returns_the_chain_probes_exactly(kind, dtype):
    small_cus = 8                                              # the capped size of an 8-CU device: 64 blocks
    for n in tw.SIZES[kind] + (tw.capped_size(kind, dtype, small_cus),):
        p_ref = _chain_problem(kind, n, dtype, tw.PROBE_LAMBDA)
        x = np.ones(n, dtype=dtype)
        assert p_ref.eval(x) == 0.0
        for p in tw.probe_positions(kind, dtype, n, small_cus):
            x[p] = 1.5
            f, _ = tw.chain_probe(kind, n, p)
            assert p_ref.eval(x) == f, (n, p)
            assert tw.same_bits(p_ref.grad(x), tw.chain_probe_gradient(kind, n, p, dtype)), (n, p)
            x[p] = 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_returns_the_end_probe_at_the_capped_size_of_a_256_cu_device(dtype):
    n = tw.capped_size(tw.ROSEN, np.float64, 256)
    assert n == 2_097_155
    x = np.ones(n, dtype=dtype)
    x[n - 1] = 1.5
    assert tw.chain_probe(tw.ROSEN, n, n - 1)[0] == 25.0
    assert orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype).eval(x) == 25.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_returns_the_dense_probes_exactly(dtype):
    for n in (1, 2, 5, 64, 257, 1025):
        cols, _ = tw.quad_case(dtype, n)
        if n > 1:
            assert not np.array_equal(cols, cols.T)            # nothing symmetric to hide behind
        p_ref = orc.Problem(orc.QUADRATIC, n, dtype, A=cols.T)  # A[i, j] = cols[j, i]
        for p in tw.probe_positions(tw.QUAD, dtype, n, CUS):
            x = np.zeros(n, dtype=dtype)
            x[p] = 1
            f, g = tw.quad_probe(cols, p)
            assert p_ref.eval(x) == f and np.array_equal(p_ref.grad(x), g), (n, p)
            if n > 1:
                assert not np.array_equal(g, cols[p, :])       # g_j = A[:, j].x, not A[j, :].x
        for p, q in tw.probe_pairs(dtype, n):
            x = np.zeros(n, dtype=dtype)
            x[p] = x[q] = 1
            f, g = tw.quad_probe(cols, p, q)
            # (the oracle adds in a wider type and rounds once: the same value unless the fp64 sum of two elements is inexact)
            assert abs(p_ref.eval(x) - f) <= np.spacing(abs(f)) and np.all(np.abs(p_ref.grad(x) - g) <= np.spacing(np.abs(g)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_returns_the_lse_probes_exactly(dtype):
    for n in tw.SIZES[tw.LSE] + (tw.capped_size(tw.LSE, dtype, 8),):
        for p in tw.probe_positions(tw.LSE, dtype, n, 8):
            x, f, g = tw.lse_probe(n, p, dtype)
            p_ref = orc.Problem(orc.LSE, n, dtype, c=x, lam=tw.PROBE_LAMBDA)
            assert p_ref.eval(x) == f and tw.same_bits(p_ref.grad(x), g), (n, p)
        x = np.full(n, 0.75, dtype=dtype)                      # all equal: se = n exactly
        v = tw.lse_value(x, x, tw.PROBE_LAMBDA, CUS)
        assert abs(v.f - (tw.LD(0.75) + np.log(tw.LD(n)))) <= 4 * tw.ULD * v.S
        p_ref = orc.Problem(orc.LSE, n, dtype, c=x, lam=tw.PROBE_LAMBDA)
        assert _within(p_ref.eval(x), v)
        assert tw.same_bits(p_ref.grad(x), np.full(n, np.float64(1) / np.float64(n)).astype(dtype))


# ------------------------------------------------------------------------------ oracle against twin, dense points
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [tw.ROSEN, tw.QCHAIN])
def test_oracle_chain_values_lie_within_the_twin_bound(kind, dtype):
    for n in tw.SIZES[kind]:
        x = tw.chain_point(kind, dtype, n)
        v = tw.chain_value(kind, x, CUS)
        assert _within(_chain_problem(kind, n, dtype, tw.QCHAIN_LAMBDA).eval(x), v), n
        assert v.bound <= (8 * tw.U[np.dtype(dtype)] + 60 * tw.U64) * v.S        # the form (k u_T + m u_64) S with small k, m


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_dense_quadratic_lies_within_the_twin_bound(dtype):
    for n in tw.SIZES[tw.QUAD]:
        cols, x = tw.quad_case(dtype, n)
        v, g, gb = tw.quad_reference(dtype, n)
        p_ref = orc.Problem(orc.QUADRATIC, n, dtype, A=cols.T)
        assert _within(p_ref.eval(x), v), n
        assert np.all(np.abs(p_ref.grad(x).astype(tw.LD) - g) <= gb), n
        assert np.allclose(g.astype(np.float64), cols.astype(np.float64) @ x.astype(np.float64), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_lse_lies_within_the_twin_bound(dtype):
    for n, variant in tw.lse_cases():
        x, c, lam = tw.lse_case(dtype, n, variant)
        v, (g, gb) = tw.lse_reference(dtype, n, variant)
        p_ref = orc.Problem(orc.LSE, n, dtype, c=c, lam=lam)
        assert _within(p_ref.eval(x), v), (n, variant)
        assert np.all(np.abs(p_ref.grad(x).astype(tw.LD) - g) <= gb), (n, variant)
        assert np.isfinite(float(v.f)) and abs(float(g.sum()) - 1 - lam * float((x.astype(tw.LD) - c.astype(tw.LD)).sum())) <= 1e-5
    x, c, lam = tw.lse_case(dtype, 1, "random")
    assert orc.Problem(orc.LSE, 1, dtype, c=c, lam=0.0).eval(x) == x[0] and tw.lse_value(x, c, 0.0, CUS).f == x[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_l2_values_lie_within_the_twin_bound(dtype):
    # the oracle's norm2 is a sequential sum in T (n roundings); its wide-accumulator form rounds once, as the device's sum does
    orc.set_dot_mode(orc.DOT_WIDE)
    try:
        for n in tw.DECORATOR_SIZES:
            x = tw.box_point(dtype, n, "l2box")
            base = tw.chain_value(tw.ROSEN, x, CUS) if n > 1 else tw.Value(tw.LD(0), tw.LD(0), tw.LD(0))
            v = tw.l2_value(base, x, tw.L2_LAMBDA, CUS)
            assert _within(orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype, l2=tw.L2_LAMBDA).eval(x), v), n
            assert v.f > base.f or n == 0
        n = 257
        x = tw.chain_point(tw.QCHAIN, dtype, n)
        v = tw.l2_value(tw.chain_value(tw.QCHAIN, x, CUS), x, tw.L2_LAMBDA, CUS)
        assert _within(orc.Problem(orc.QUADRATIC_CHAIN, n, dtype, lam=tw.QCHAIN_LAMBDA, l2=tw.L2_LAMBDA).eval(x), v)
        cols, x = tw.quad_case(dtype, n)
        v = tw.l2_value(tw.quad_reference(dtype, n)[0], x, tw.L2_LAMBDA, CUS)
        assert _within(orc.Problem(orc.QUADRATIC, n, dtype, A=cols.T, l2=tw.L2_LAMBDA).eval(x), v)
        x, c, lam = tw.lse_case(dtype, n, "random")
        v = tw.l2_value(tw.lse_reference(dtype, n, "random")[0], x, tw.L2_LAMBDA, CUS)
        assert _within(orc.Problem(orc.LSE, n, dtype, c=c, lam=lam, l2=tw.L2_LAMBDA).eval(x), v)
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


def test_clamp_case_follows_numpy_clip():
    for dtype in DTYPES:
        for n in tw.DECORATOR_SIZES:
            for lo, hi in ((-0.5, 0.75), (0.25, 0.25)):
                x, want = tw.clamp_case(dtype, n, lo, hi)
                assert tw.same_bits(orc.box_clamp(x.copy(), lo, hi), want)
                ok = ~np.isnan(x)
                assert np.array_equal(want[ok], np.clip(x[ok], lo, hi)) and np.isnan(want[~ok]).all()
            if n >= 255:
                assert np.isnan(x).sum() == 1


# ------------------------------------------------------------------------------ the bounds reject what they are for
# Sizes at which a planted error is smaller than the bound in fp32 would be listed here as covered by the probes only (at most
# three per kind).  With the points of problems_twin (x = u - 1/2 for the chain kinds, entries u - 1/2 for the dense quadratic,
# x = 3 (u - 1/2) for log-sum-exp) there are none.
PROBES_ONLY = {tw.ROSEN: (), tw.QCHAIN: (), tw.QUAD: (), tw.LSE: ()}


def _outside(planted, value):
    return not abs(tw.LD(planted) - value.f) <= value.bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [tw.ROSEN, tw.QCHAIN])
def test_chain_bounds_reject_planted_errors(kind, dtype):
    dt = np.dtype(dtype)
    N = tw.VEC[dt]
    for n in tw.SIZES[kind]:
        if n in PROBES_ONLY[kind]:
            continue
        x = tw.chain_point(kind, dtype, n)
        t = tw.chain_terms(kind, x)
        v = tw.chain_value(kind, x, CUS)
        planted = {"last term dropped": t[:-1]}
        own = tw.term_block(kind, dtype, n, CUS)[:t.size]
        planted["one block's partial left out"] = t[own != own.max()] if own.max() > 0 else t[:0]
        if kind == tw.ROSEN:
            xl = x.astype(tw.LD)
            if n > N:                                          # the term of a vector's last element with 0 for its right neighbour
                i = N - 1
                seam = t.copy()
                seam[i] = 100 * (0 - xl[i] * xl[i]) ** 2 + (1 - xl[i]) ** 2
                planted["right neighbour 0 at a vector seam"] = seam
            if n % N and n // N * N + 1 < n:                   # the first term of the ragged tail, twice
                planted["tail's first term twice"] = np.concatenate([t, t[n // N * N:n // N * N + 1]])
            elif n % N:                                        # the tail holds no term of its own: the last whole vector's, twice
                planted["tail's first term twice"] = np.concatenate([t, t[-1:]])
        for what, terms in planted.items():
            assert _outside(tw.tree_sum(terms)[0], v), (n, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_quadratic_bounds_reject_planted_errors(dtype):
    for n in tw.SIZES[tw.QUAD]:
        if n in PROBES_ONLY[tw.QUAD]:
            continue
        cols, x = tw.quad_case(dtype, n)
        v, g, gb = tw.quad_reference(dtype, n)
        xl = x.astype(tw.LD)
        part = g * xl
        assert _outside((part.sum() - part[n - 1]) / 2, v), n                       # one block's partial left out
        if n > 1:
            g_short = g - cols[:, n - 1].astype(tw.LD) * xl[n - 1]                 # the last term of every column sum dropped
            assert _outside((g_short * xl).sum() / 2, v), n
            assert np.all(np.abs(g_short - g) > gb), n
            g_rows = cols.T.astype(tw.LD) @ xl                                     # rows instead of columns
            assert (np.abs(g_rows - g) > gb).mean() > 0.9, n


@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_bounds_reject_planted_errors(dtype):
    for n in tw.SIZES[tw.LSE]:
        if n in PROBES_ONLY[tw.LSE] or n == 1:                 # (n = 1: one term, nothing to drop; f = x0 is checked exactly)
            continue
        x, c, lam = tw.lse_case(dtype, n, "random")
        v = tw.lse_reference(dtype, n, "random")[0]
        assert _outside(tw.lse_value(x, c, lam, CUS, drop=[n - 1]).f, v), n         # the last term dropped
        own = tw.term_block(tw.LSE, dtype, n, CUS)
        if own.max() > 0:
            assert _outside(tw.lse_value(x, c, lam, CUS, drop=np.nonzero(own == own.max())[0]).f, v), n
        # a maximum that ignores the last element: the value is shift invariant, so it shows only where exp overflows
        x, c, lam = tw.lse_case(dtype, n, "last_high")
        v = tw.lse_reference(dtype, n, "last_high")[0]
        assert np.isfinite(float(v.f)) and _outside(tw.lse_value(x, c, lam, CUS, mx=x[:-1].max()).f, v), n
