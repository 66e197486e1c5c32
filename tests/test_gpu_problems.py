"""The built-in objectives on the device (csrc/dzo_problems.hip) against tests/problems_twin.py, in fp64 and fp32.

1. Exact probes, bit for bit: points at which every operation is exact, so that a value does not depend on the order of the
   sums -- one raised element on a flat chain, unit vectors and pairs of them on a matrix without symmetry, one zero among
   -800s for log-sum-exp -- moved across every seam of the kernels (vector, wave, block, grid-stride trip, ragged tail, the
   finish kernel's unrolled loop), at the small edge sizes and at the size where the device's grid cap is reached.
2. Dense points against a longdouble reference within bounds derived from the kernels' arithmetic (the twin's docstring);
   gradients of the chain kinds bit for bit against the oracle, the others element by element within bound.
3. The L2 and box decorators and box_clamp at their own edge sizes, with elements exactly on the bounds.
4. Determinism, and two handles used alternately.

Every figure is printed before it is asserted (pytest -s shows them); the last test prints the worst error/bound per kind."""
import functools

import numpy as np
import pytest

import problems_twin as tw
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
DZO_KIND = {tw.ROSEN: dzo.ROSENBROCK_CHAIN, tw.QCHAIN: dzo.QUADRATIC_CHAIN, tw.QUAD: dzo.QUADRATIC, tw.LSE: dzo.LSE}
ORC_KIND = {tw.ROSEN: orc.ROSENBROCK_CHAIN, tw.QCHAIN: orc.QUADRATIC_CHAIN, tw.QUAD: orc.QUADRATIC, tw.LSE: orc.LSE}
WORST = {}                 # (kind, dtype, "value" | "gradient") -> (ratio, n)
EXACT = {}                 # (kind, dtype) -> probe cases that were bit-exact


@functools.lru_cache(maxsize=None)
def _cus():
    return dzo.device_info()["compute_units"]


def _ratio(kind, dtype, what, n, err, bound):
    """the worst err / bound of a check (scalars or arrays), printed and recorded; a zero bound with a zero error counts as 0"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=tw.LD)), np.atleast_1d(np.asarray(bound, dtype=tw.LD))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0, err / bound)
    r = float(np.max(r))
    print(f"RATIO {kind} {dtype} {what} n={n} {r:.3f}")
    key = (kind, str(dtype), what)
    if r > WORST.get(key, (-1.0, 0))[0]:
        WORST[key] = (r, n)
    return r


def _set(arr, p, v):
    arr.view(p, 1).upload(np.array([v], dtype=arr.dtype))


def _probe_sizes(kind, dtype, which):
    return tw.SIZES[kind] if which == "small" else (tw.capped_size(kind, dtype, _cus()),)


# ------------------------------------------------------------------------------ 1. exact probes
@pytest.mark.parametrize("which", ["small", "capped"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [tw.ROSEN, tw.QCHAIN])
def test_chain_probes_are_exact(kind, dtype, which):
    dt = np.dtype(dtype)
    for n in _probe_sizes(kind, dt, which):
        dev = dzo.Problem(DZO_KIND[kind], n, dt, lam=tw.PROBE_LAMBDA)
        ref = orc.Problem(ORC_KIND[kind], n, dt, lam=tw.PROBE_LAMBDA)
        x = np.ones(n, dtype=dt)
        dx, dg = dzo.DeviceArray.from_host(x), dzo.DeviceArray(n, dt)
        assert dev(dx) == 0.0 and tw.same_bits(dev.gradient_(dg, dx).to_host(), ref.grad(x)), n
        if which == "capped":                                  # the finish kernel's unrolled loop needs more than 1792 partials
            grid = tw.launch(kind, dt, n, _cus())[0]
            print(f"capped {kind} {dtype}: n = {n}, {grid} blocks")
            assert grid == min(8 * _cus(), 2048) and n <= 4_200_000
        for p in tw.probe_positions(kind, dt, n, _cus()):
            _set(dx, p, 1.5)
            x[p] = 1.5
            f, _ = tw.chain_probe(kind, n, p)
            assert dev(dx) == f, (n, p)
            assert tw.same_bits(dev.gradient_(dg, dx).to_host(), ref.grad(x)), (n, p)
            _set(dx, p, 1.0)
            x[p] = 1.0
            EXACT[(kind, dtype)] = EXACT.get((kind, dtype), 0) + 1


@functools.lru_cache(maxsize=None)
def _quad_device_buffer(dtype):
    return dzo.DeviceArray.from_host(tw.quad_buffer(np.dtype(dtype)))


def _quad_problem(dtype, n):
    """the device problem on the first n^2 entries of the shared buffer: element i of column j at j n + i"""
    return dzo.Problem(dzo.QUADRATIC, n, dtype, A=_quad_device_buffer(dtype).view(0, (n, n)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_quadratic_probes_are_exact(dtype):
    dt = np.dtype(dtype)
    for n in tw.SIZES[tw.QUAD]:
        cols, _ = tw.quad_case(dt, n)
        dev = _quad_problem(dt, n)
        dx, dg = dzo.DeviceArray.zeros(n, dt), dzo.DeviceArray(n, dt)
        for p in tw.probe_positions(tw.QUAD, dt, n, _cus()):
            _set(dx, p, 1.0)
            f, g = tw.quad_probe(cols, p)
            assert dev(dx) == f, (n, p)
            g_dev = dev.gradient_(dg, dx).to_host()
            assert tw.same_bits(g_dev, g), (n, p)              # column sums: g_j = A[:, j].x = cols[j, p] ...
            assert n == 1 or not np.array_equal(g_dev, cols[p, :])     # ... not A[j, :].x
            _set(dx, p, 0.0)
            EXACT[(tw.QUAD, dtype)] = EXACT.get((tw.QUAD, dtype), 0) + 1
        for p, q in tw.probe_pairs(dt, n):
            _set(dx, p, 1.0)
            _set(dx, q, 1.0)
            f, g = tw.quad_probe(cols, p, q)
            assert dev(dx) == f, (n, p, q)
            assert tw.same_bits(dev.gradient_(dg, dx).to_host(), g), (n, p, q)
            _set(dx, p, 0.0)
            _set(dx, q, 0.0)
            EXACT[(tw.QUAD, dtype)] = EXACT.get((tw.QUAD, dtype), 0) + 1


@pytest.mark.parametrize("which", ["small", "capped"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_probes_are_exact(dtype, which):
    dt = np.dtype(dtype)
    for n in _probe_sizes(tw.LSE, dt, which):
        dx, dg = dzo.DeviceArray.from_host(np.full(n, -800.0, dtype=dt)), dzo.DeviceArray(n, dt)
        dev = dzo.Problem(dzo.LSE, n, dt, c=dx, lam=tw.PROBE_LAMBDA)      # c is x itself
        for p in tw.probe_positions(tw.LSE, dt, n, _cus()):
            _set(dx, p, 0.0)
            _, f, g = tw.lse_probe(n, p, dt)
            assert dev(dx) == f, (n, p)                        # a maximum that misses p overflows; a term visited twice gives log 2
            assert tw.same_bits(dev.gradient_(dg, dx).to_host(), g), (n, p)
            _set(dx, p, -800.0)
            EXACT[(tw.LSE, dtype)] = EXACT.get((tw.LSE, dtype), 0) + 1
        # all elements equal: se = n exactly, g = 1 / n rounded once in fp64 and once to T
        x = np.full(n, 0.75, dtype=dt)
        dx.upload(x)
        v = tw.lse_value(x, x, tw.PROBE_LAMBDA, _cus())
        assert _ratio(tw.LSE, dtype, "value", n, abs(tw.LD(dev(dx)) - v.f), v.bound) <= 1, n
        assert tw.same_bits(dev.gradient_(dg, dx).to_host(), np.full(n, np.float64(1) / np.float64(n)).astype(dt)), n


# ------------------------------------------------------------------------------ 2. dense points
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [tw.ROSEN, tw.QCHAIN])
def test_chain_values_within_bound_and_gradients_bit_for_bit(kind, dtype):
    dt = np.dtype(dtype)
    for n in tw.SIZES[kind]:
        x = tw.chain_point(kind, dt, n)
        dev = dzo.Problem(DZO_KIND[kind], n, dt, lam=tw.QCHAIN_LAMBDA)
        ref = orc.Problem(ORC_KIND[kind], n, dt, lam=tw.QCHAIN_LAMBDA)
        dx = dzo.DeviceArray.from_host(x)
        v = tw.chain_value(kind, x, _cus())
        assert _ratio(kind, dtype, "value", n, abs(tw.LD(dev(dx)) - v.f), v.bound) <= 1, n
        same = tw.same_bits(dev.gradient_(dzo.DeviceArray(n, dt), dx).to_host(), ref.grad(x))
        _ratio(kind, dtype, "gradient", n, 0 if same else 2, 1)
        assert same, n


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_quadratic_within_bound_element_by_element(dtype):
    dt = np.dtype(dtype)
    for n in tw.SIZES[tw.QUAD]:
        _, x = tw.quad_case(dt, n)
        v, g, gb = tw.quad_reference(dt, n)
        dev = _quad_problem(dt, n)
        dx = dzo.DeviceArray.from_host(x)
        assert _ratio(tw.QUAD, dtype, "value", n, abs(tw.LD(dev(dx)) - v.f), v.bound) <= 1, n
        g_dev = dev.gradient_(dzo.DeviceArray(n, dt), dx).to_host().astype(tw.LD)
        assert _ratio(tw.QUAD, dtype, "gradient", n, np.abs(g_dev - g), gb) <= 1, n


@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_within_bound_element_by_element(dtype):
    dt = np.dtype(dtype)
    for n, variant in tw.lse_cases():
        x, c, lam = tw.lse_case(dt, n, variant)
        v, (g, gb) = tw.lse_reference(dt, n, variant, _cus())
        dev = dzo.Problem(dzo.LSE, n, dt, c=c, lam=lam)
        dx = dzo.DeviceArray.from_host(x)
        assert _ratio(tw.LSE, dtype, "value", n, abs(tw.LD(dev(dx)) - v.f), v.bound) <= 1, (n, variant)
        g_dev = dev.gradient_(dzo.DeviceArray(n, dt), dx).to_host().astype(tw.LD)
        assert _ratio(tw.LSE, dtype, "gradient", n, np.abs(g_dev - g), gb) <= 1, (n, variant)
    x, c, _ = tw.lse_case(dt, 1, "random")                      # n = 1, lambda = 0: f = x0 exactly
    assert dzo.Problem(dzo.LSE, 1, dt, c=c, lam=0.0)(dzo.DeviceArray.from_host(x)) == x[0]


# ------------------------------------------------------------------------------ 3. decorators
def _decorator_sizes(dtype):
    return tw.DECORATOR_SIZES + (tw.capped_size(tw.QCHAIN, dtype, _cus()),)      # sumsq, grad_decorate, box_clamp: stream_grid(n, 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_l2_value_within_bound_on_the_chained_rosenbrock(dtype):
    dt = np.dtype(dtype)
    for n in _decorator_sizes(dt):
        x = tw.box_point(dt, n, "l2box")
        base = tw.chain_value(tw.ROSEN, x, _cus()) if n > 1 else tw.Value(tw.LD(0), tw.LD(0), tw.LD(0))
        v = tw.l2_value(base, x, tw.L2_LAMBDA, _cus())
        dev = dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt, l2=tw.L2_LAMBDA)
        got = dev(dzo.DeviceArray.from_host(x))
        assert _ratio("l2", dtype, "value", n, abs(tw.LD(got) - v.f), v.bound) <= 1, n


@pytest.mark.parametrize("config", list(tw.BOX_CONFIGS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_l2_and_box_gradient_bit_for_bit(dtype, config):
    dt = np.dtype(dtype)
    l2, lo, hi = tw.BOX_CONFIGS[config]
    found = set()
    for n in _decorator_sizes(dt):
        x = tw.box_point(dt, n, config)
        ref = orc.Problem(orc.ROSENBROCK_CHAIN, n, dt, l2=l2, box_gradient=(lo, hi))
        dev = dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt, l2=l2, box_gradient=(lo, hi))
        g_dev = dev.gradient_(dzo.DeviceArray(n, dt), dzo.DeviceArray.from_host(x)).to_host()
        assert tw.same_bits(g_dev, ref.grad(x)), n
        found |= tw.box_situations(x, orc.Problem(orc.ROSENBROCK_CHAIN, n, dt, l2=l2).grad(x), lo, hi)
    want = {"l2box": {("lo", "positive"), ("lo", "negative"), ("hi", "positive"), ("hi", "negative")},
            "hi1": {("hi", "-0"), ("hi", "+0"), ("lo", "+0")}, "lo1": {("lo", "-0"), ("lo", "+0")},
            "pinch": {("lo", "-0"), ("hi", "-0"), ("lo", "+0"), ("hi", "+0")}}[config]
    assert want <= found, sorted(want - found)


@pytest.mark.parametrize("dtype", DTYPES)
def test_box_clamp_bit_for_bit(dtype):
    dt = np.dtype(dtype)
    for n in _decorator_sizes(dt):
        for lo, hi in ((-0.5, 0.75), (0.25, 0.25)):            # the second: lo == hi
            x, want = tw.clamp_case(dt, n, lo, hi)
            dx = dzo.DeviceArray.from_host(x)
            assert dzo.box_clamp_(dx, lo, hi)
            got = dx.to_host()
            assert tw.same_bits(got, want), (n, lo, hi)
            assert np.isnan(got).sum() == np.isnan(x).sum()    # a NaN stays a NaN


def _kind_case(kind, dt, n):
    """(device problem keyword arguments, oracle's, x, the undecorated Value) of a kind at a dense point"""
    if kind == tw.QUAD:
        cols, x = tw.quad_case(dt, n)
        return dict(A=_quad_device_buffer(dt).view(0, (n, n))), dict(A=cols.T), x, tw.quad_reference(dt, n)[0]
    if kind == tw.LSE:
        x, c, lam = tw.lse_case(dt, n, "random")
        return dict(c=c, lam=lam), dict(c=c, lam=lam), x, tw.lse_reference(dt, n, "random", _cus())[0]
    x = tw.chain_point(kind, dt, n)
    kw = dict(lam=tw.QCHAIN_LAMBDA)
    return kw, kw, x, tw.chain_value(kind, x, _cus())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", tw.KINDS)
def test_l2_on_every_kind(kind, dtype):
    """the base evaluation's partials are consumed before sumsq_kernel reuses the scratch"""
    dt, n = np.dtype(dtype), 257
    kw, _, x, base = _kind_case(kind, dt, n)
    v = tw.l2_value(base, x, tw.L2_LAMBDA, _cus())
    dev = dzo.Problem(DZO_KIND[kind], n, dt, l2=tw.L2_LAMBDA, **kw)
    dx = dzo.DeviceArray.from_host(x)
    assert _ratio("l2", dtype, "value", n, abs(tw.LD(dev(dx)) - v.f), v.bound) <= 1
    plain = dzo.Problem(DZO_KIND[kind], n, dt, **kw)
    assert abs(tw.LD(plain(dx)) - base.f) <= base.bound and dev(dx) == dev(dx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decorators_on_the_dense_quadratic(dtype):
    """grad_decorate_kernel is elementwise: from the device's own undecorated gradient its result follows bit for bit (one fma
    with lambda + lambda in T, then the box rule)"""
    dt, n = np.dtype(dtype), 257
    l2, lo, hi = tw.L2_LAMBDA, -0.25, 0.25
    cols, x = tw.quad_case(dt, n)
    x = np.clip(x, lo, hi)
    A = _quad_device_buffer(dt).view(0, (n, n))
    dx = dzo.DeviceArray.from_host(x)
    g0 = dzo.Problem(dzo.QUADRATIC, n, dt, A=A).gradient_(dzo.DeviceArray(n, dt), dx).to_host()
    want = g0.copy()
    orc.axpy(float(dt.type(l2) + dt.type(l2)), x, want)        # want = fma(2 lambda, x, g0) in T
    found = tw.box_situations(x, want, lo, hi)
    assert {("lo", "positive"), ("lo", "negative"), ("hi", "positive"), ("hi", "negative")} <= found
    want = tw.box_rule(x, want, lo, hi)
    got = dzo.Problem(dzo.QUADRATIC, n, dt, A=A, l2=l2, box_gradient=(lo, hi)).gradient_(dzo.DeviceArray(n, dt), dx).to_host()
    assert tw.same_bits(got, want)


# ------------------------------------------------------------------------------ 4. determinism and independence
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_twice_and_two_handles_used_alternately(dtype):
    dt, n = np.dtype(dtype), 1025
    alone = {}
    handles = {}
    for kind in tw.KINDS:
        kw, _, x, _ = _kind_case(kind, dt, n)
        dev = dzo.Problem(DZO_KIND[kind], n, dt, **kw)
        dx, dg = dzo.DeviceArray.from_host(x), dzo.DeviceArray(n, dt)
        f, g = dev(dx), dev.gradient_(dg, dx).to_host()
        assert dev(dx) == f and tw.same_bits(dev.gradient_(dg, dx).to_host(), g), kind
        alone[kind], handles[kind] = (f, g), (dev, dx, dg)
    for a, b in ((tw.ROSEN, tw.LSE), (tw.QUAD, tw.QCHAIN), (tw.LSE, tw.QUAD)):
        for _ in range(3):
            for kind in (a, b):
                dev, dx, dg = handles[kind]
                assert dev(dx) == alone[kind][0] and tw.same_bits(dev.gradient_(dg, dx).to_host(), alone[kind][1]), (a, b, kind)


def test_report():
    """the worst error/bound per kind and dtype and the number of bit-exact probe cases (run after the tests above)"""
    for key in sorted(WORST):
        print("WORST", *key, "%.3f at n=%d" % WORST[key])
    for key in sorted(EXACT):
        print("EXACT", *key, EXACT[key])
    assert all(r <= 1 for r, _ in WORST.values())
